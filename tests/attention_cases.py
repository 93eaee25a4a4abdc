"""Shared by tests/test_attention_cases_cpu.py and tests/test_gpu_encoder_cores.py (not a test module): seeded inputs for the encoders'
attention cores and the BEATs positional convolution, their float64 references, the per-element error bound the GPU kernels are held to,
and an fp32 / 16-bit emulation of the kernels' softmax arithmetic with named mutants.  Pure torch on the CPU.

The bound is DERIVED, not measured.  With u the unit roundoff of the operand type T (2^-11 for f16, 2^-8 for bf16), p the exact softmax row
and A = sum_j p_j |v_j| (float64):

    attention   |out - ref| <= 4 u A + S 2^-24 max_j |v_j|
                  2 u   P is rounded to T once, and enters both the numerator (P V) and the denominator (the row sum of the ROUNDED P)
                  1 u   the output is rounded to T
                  1 u   left for the fp32 accumulation of q.k and P.V and for the hardware exp2; it holds as long as the exponent's fp32
                        argument error stays below u, i.e. max |score| <= 128 in log2 units: the builders assert that
                  S 2^-24 max|v|   P values in (or flushed from) T's subnormal range carry an ABSOLUTE error of up to 2^-24 each
    posconv     |out - ref| <= K 2^-24 B + 2^-20 (1 + |pre-activation|),   B = sum |x16| |w16|,  K = 48 taps
                  first term: any fp32 summation order of the K products; second: the erf of csrc/mra_common.h (Abramowitz-Stegun 7.1.26,
                  absolute error 1.5e-7, with a hardware reciprocal), the bias add and the final fp32 add.

The plain fp32 / T emulation of the kernels' arithmetic (``emulate``) sits at <= 0.36 of the attention bound on every family below (hd = 88,
S in {2, 122, 257}, both dtypes: tests/test_attention_cases_cpu.py), so a kernel above 1.0 has a defect, not noise; the mutants show which
family exposes which defect (``pad1`` needs ``negative``, ``scale`` needs ``peaked``)."""
import math

import torch
import torch.nn.functional as F

from mraudio_amd.models.beats import relative_position_bucket

LOG2E = 1.4426950408889634
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
MAX_LOG2_SCORE = 128.0

# The mask and fragment boundaries of the ViT core (16-key fragments; 257 = 16 fragments + 1 key): every query points at one of these keys.
ONEHOT_TARGETS = (0, 15, 16, 255, 256)
VIT_FAMILIES = ("mild", "peaked", "negative", "constant", "onehot_last") + tuple(f"onehot@{t}" for t in ONEHOT_TARGETS)
BEATS_FAMILIES = ("mild", "peaked", "negative", "constant", "onehot@0", "onehot_last")


def families_for(S: int, names=VIT_FAMILIES):
    """The families that exist at sequence length S (a one-hot target must be a key)."""
    return [k for k in names if not k.startswith("onehot@") or int(k.split("@")[1]) < S]


def _seed(kind: str, S: int, hd: int, dtype) -> int:
    return (sum(ord(c) * (i + 1) for i, c in enumerate(kind)) * 1009 + S * 7919 + hd * 31 + (0 if dtype == torch.float16 else 1)) % (2 ** 31)


def make_qkv(kind: str, units: int, S: int, hd: int, dtype=torch.float16, seed=None):
    """q, k, v [units, S, hd], already rounded to ``dtype`` (so the reference sees exactly what the kernel sees).

    mild         q, k, v ~ 0.75 N(0, 1): near-uniform rows
    peaked       q and k x 3: median row maximum ~0.57 at S = 257
    negative     q = 0.3 noise + a, k = 0.3 noise - a with a shared a ~ 2 N(0, 1): every valid score is far below zero, so a zero-score
                 padding key left unmasked would win the softmax
    constant     all keys equal: uniform rows whatever the query, the output is the mean of v
    onehot@t / onehot_last   every query is the same vector and key t (S - 1) equals it, the other keys are small"""
    g = torch.Generator().manual_seed(_seed(kind, S, hd, dtype) if seed is None else seed)
    q = torch.randn(units, S, hd, generator=g) * 0.75
    k = torch.randn(units, S, hd, generator=g) * 0.75
    v = torch.randn(units, S, hd, generator=g) * 0.75
    if kind == "mild":
        pass
    elif kind == "peaked":
        q, k = q * 3, k * 3
    elif kind == "negative":
        a = torch.randn(units, 1, hd, generator=g) * 2.0
        q, k = q * 0.3 + a, k * 0.3 - a
    elif kind == "constant":
        k = torch.randn(units, 1, hd, generator=g).expand(units, S, hd).clone()
    elif kind.startswith("onehot"):
        t = S - 1 if kind == "onehot_last" else int(kind.split("@")[1])
        assert 0 <= t < S, (kind, S)
        q = torch.randn(units, 1, hd, generator=g).expand(units, S, hd).clone()
        k = k * 0.05
        k[:, t] = q[:, 0]
    else:
        raise ValueError(kind)
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    worst = (q.float() @ k.float().transpose(-1, -2)).abs().max().item() * LOG2E / math.sqrt(hd)
    assert worst <= MAX_LOG2_SCORE, (kind, S, hd, worst)
    return q, k, v


# ---- float64 references and bounds --------------------------------------------------------------------------------------------
def attention_ref(q, k, v, bias=None):
    """softmax(q k^T / sqrt(hd) [+ bias]) v in float64 over [..., S, hd] inputs (bias [..., S, S]).  Returns (out, bound, p) with the
    per-element bound of the module docstring for the inputs' dtype."""
    u = U[q.dtype]
    S, hd = q.shape[-2], q.shape[-1]
    q, k, v = q.double(), k.double(), v.double()
    s = q @ k.transpose(-1, -2) / math.sqrt(hd)
    if bias is not None:
        s = s + bias.double()
    assert s.abs().max().item() * LOG2E <= MAX_LOG2_SCORE, s.abs().max().item() * LOG2E
    p = torch.softmax(s, -1)
    out = p @ v
    A = p @ v.abs()
    bound = 4 * u * A + S * 2.0 ** -24 * v.abs().amax(-2, keepdim=True)
    return out, bound, p


def beats_gate(src, gw, gb, ga):
    """The gate of the relative-position bias as mraudio_amd/models/beats.py computes it, in float64: src [n, heads, P, 64] (the q
    projection for BEATs, the layer input's head slice for WavLM), gw [8, 64], gb [8], ga [heads] -> [n, heads, P, 1]."""
    n, h, p, _ = src.shape
    u = (src.double() @ gw.double().t() + gb.double()).view(n, h, p, 2, 4).sum(-1)
    a, b = torch.sigmoid(u).chunk(2, dim=-1)
    return a * (b * ga.double().view(1, h, 1, 1) - 1.0) + 2.0


def beats_position_bias(E, P: int, num_buckets: int = 320, max_distance: int = 800):
    """[heads, P, P] float64: E[bucket(j - i)][h] with the bucket of mraudio_amd/models/beats.py; E [num_buckets, heads]."""
    pos = torch.arange(P)
    b = relative_position_bucket(pos[None, :] - pos[:, None], num_buckets, max_distance)
    return E.double()[b].permute(2, 0, 1)


def beats_attention_ref(q, k, v, gate_src, E, gw, gb, ga):
    """BEATs' core in float64: softmax(q k^T / 8 + G E[bucket(j - i)]) v over [n, heads, P, 64] inputs."""
    bias = beats_gate(gate_src, gw, gb, ga) * beats_position_bias(E, q.shape[-2])[None]
    return attention_ref(q, k, v, bias)


def posconv_ref(x, w_eff, b, groups: int = 16):
    """x + gelu(conv1d(f16(x), f16(W_eff), b, padding = taps / 2, groups)[..., :P]) in float64: x [n, P, D] fp32, w_eff [D, D / groups, taps],
    b [D].  x and the weight are rounded to f16 as the kernel stages them; the residual x is not.  Returns (out, bound)."""
    n, P, D = x.shape
    taps = w_eff.shape[-1]
    x16 = x.half().double().transpose(1, 2)
    w16 = w_eff.half().double()
    pre = F.conv1d(x16, w16, b.double(), padding=taps // 2, groups=groups)[..., :P].transpose(1, 2)
    B = F.conv1d(x16.abs(), w16.abs(), None, padding=taps // 2, groups=groups)[..., :P].transpose(1, 2)
    out = x.double() + 0.5 * pre * (1.0 + torch.erf(pre / math.sqrt(2.0)))
    K = w_eff.shape[1] * taps
    bound = K * 2.0 ** -24 * B + 2.0 ** -20 * (1.0 + pre.abs())
    return out, bound


# ---- the kernels' arithmetic in plain fp32 / T torch, and its mutants ---------------------------------------------------------
MUTANTS = ("pad1", "scale", "drop_last")


def emulate(q, k, v, bias=None, mutant=None):
    """The attention cores' arithmetic: fp32 scores of the T operands, exp2(fma(s, sl2, -mx sl2)) (with a bias: the fp32 score
    s sl2 + bias log2(e), then exp2(score - max)), P rounded to T, the row sum of the ROUNDED P, fp32 P V, the output rounded to T.
    Mutants: ``pad1`` one zero padding key (score 0, value 0) left unmasked; ``scale`` sl2 x 1.01; ``drop_last`` the last key masked."""
    T = q.dtype
    hd = q.shape[-1]
    sl2 = torch.tensor(LOG2E / math.sqrt(hd) * (1.01 if mutant == "scale" else 1.0), dtype=torch.float32)
    s = q.float() @ k.float().transpose(-1, -2)
    vv = v
    if bias is not None:
        s = s * sl2 + (bias.double() * LOG2E).float()
    if mutant == "pad1":
        s = torch.cat([s, torch.zeros_like(s[..., :1])], -1)
        vv = torch.cat([v, torch.zeros_like(v[..., :1, :])], -2)
    if mutant == "drop_last":
        s = s.clone()
        s[..., -1] = -3.0e38
    mx = s.max(-1, keepdim=True).values
    e = torch.exp2(s - mx) if bias is not None else torch.exp2(s * sl2 - mx * sl2)
    P = e.to(T)
    l = P.float().sum(-1, keepdim=True)
    return ((P.float() @ vv.float()) / l).to(T)


def worst_ratio(out, ref, bound) -> float:
    """max over every element of |out - ref| / bound (inf for a non-finite output)."""
    d = (out.double() - ref).abs()
    if not torch.isfinite(d).all():
        return float("inf")
    return (d / bound).max().item()


# ---- the kernels' buffer layouts ----------------------------------------------------------------------------------------------
HD_PAD = 96


def pack_vit_qkv(q, k, v):
    """[n, heads, S, hd] x 3 -> the ViT core's [n * S, 3, heads, 96] with zero columns hd .. 95."""
    n, h, S, hd = q.shape
    out = torch.zeros(n, S, 3, h, HD_PAD, dtype=q.dtype)
    for i, t in enumerate((q, k, v)):
        out[:, :, i, :, :hd] = t.transpose(1, 2)
    return out.view(n * S, 3 * h * HD_PAD)


def unpack_ctx(ctx, n: int, heads: int):
    """[n * S, heads * hd] -> [n, heads, S, hd]."""
    rows, w = ctx.shape
    return ctx.view(n, rows // n, heads, w // heads).transpose(1, 2)


def pack_beats_qkv(q, k, v):
    """[n, heads, P, 64] x 3 -> BEATs' [n * P, 3 * dim] (q | k | v thirds, heads side by side)."""
    n, h, P, hd = q.shape
    return torch.cat([t.transpose(1, 2).reshape(n * P, h * hd) for t in (q, k, v)], dim=1).contiguous()


def make_units(kinds, heads: int, S: int, hd: int, dtype):
    """One frame (chunk) per family: q, k, v [len(kinds), heads, S, hd]."""
    parts = [make_qkv(kind, heads, S, hd, dtype) for kind in kinds]
    return tuple(torch.stack([p[i] for p in parts]) for i in range(3))


# ---- BEATs parameters of the core ---------------------------------------------------------------------------------------------
def beats_core_params(heads: int, seed: int = 5, bias_scale: float = 1.0, num_buckets: int = 320):
    """Seeded gate parameters and bias table in the scales of BEATs.init_seeded_: grep_linear N(0, 0.1), grep_a 1 + N(0, 0.3), the table
    N(0, 0.5) x bias_scale (clamped to +-20).  ``bias_scale = PEAKED_BIAS_SCALE`` peaks the rows by the bias alone (mean row maximum > 0.4)."""
    g = torch.Generator().manual_seed(seed)
    return {"E": (torch.randn(num_buckets, heads, generator=g) * 0.5 * bias_scale).clamp(-20.0, 20.0), "gw": torch.randn(8, 64, generator=g) * 0.1,
            "gb": torch.randn(8, generator=g) * 0.1, "ga": 1.0 + torch.randn(heads, generator=g) * 0.3}


# N(0, 0.5) x 12 = N(0, 6), clamped to +-20: G < 3.2 keeps |G E| log2(e) below 93, inside the 128 of the bound (the whole-encoder test's x 20 is not)
PEAKED_BIAS_SCALE = 12.0


def make_posconv(n: int, P: int, D: int = 768, groups: int = 16, taps: int = 128, seed: int = 11):
    """x [n, P, D] fp32 with |x| up to ~4, the effective weight [D, D / groups, taps] at weight-norm gain 2 per tap (unit-scale
    pre-activations, as BEATs.init_seeded_ makes them) and the bias [D]."""
    g = torch.Generator().manual_seed(seed * 1000 + P * 4 + n)
    x = (torch.randn(n, P, D, generator=g) * 1.3).clamp(-4.0, 4.0)
    gw = torch.Generator().manual_seed(seed)
    w = torch.randn(D, D // groups, taps, generator=gw)
    w = (2.0 + 0.2 * torch.randn(1, 1, taps, generator=gw)) * w / w.norm(dim=(0, 1), keepdim=True)
    b = torch.randn(D, generator=gw) * 0.02
    return x, w, b
