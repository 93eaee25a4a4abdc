"""Shared by tests/test_multi_query_cpu.py and tests/test_gpu_multi_query.py (not a test module): seeded inputs for the cross core of the
multi-prompt forward (several prompts' query blocks over ONE K/V stream per encoder item), the float64 reference, the per-element bound
and an fp32 / 16-bit emulation of the core's tile-wise online softmax with named mutants.  Pure torch on the CPU.

Shapes: q [enc_items * P, heads, 32, 64] (chain item n = i * P + p: encoder item i, prompt slot p), k, v [enc_items, heads, kv, 64].
K / V differ per encoder item and q differs per prompt slot, so a wrong index cannot pass.

The bound is the one of tests/attention_cases.py with S := kv (derived there, not measured):

    |out - ref| <= 4 u sum_j p_j |v_j| + kv 2^-24 max_j |v_j|

The emulation (``emulate``) does what csrc/attention.hip does: 32-key tiles, fp32 scores in log2 units, a running maximum with an fp32
rescale of O and l, P rounded to the operand type T per tile for P V, l summed from the fp32 P, the output rounded to T.  It sits below
half of the bound on every family (tests/test_multi_query_cpu.py), so a kernel above 1.0 has a defect.  Mutants and the family that
exposes each:
    kv_next     K / V of encoder item i + 1              -> every family (``mild`` is asserted)
    q_next      q of prompt slot p + 1                   -> ``mild`` / ``peaked`` (not ``constant``: uniform rows whatever the query)
    tail        tail keys left unmasked: the staging clamps the token index, so the last key is counted once per padding row
                                                         -> ``constant`` / ``mild`` at kv % 32 != 0, kv > 1 (not ``onehot@kv-1``)"""
import math

import torch

from attention_cases import LOG2E, MAX_LOG2_SCORE, U, worst_ratio  # noqa: F401  (re-exported for the tests)

Q_ROWS, HD, TILE = 32, 64, 32
BASE_FAMILIES = ("mild", "peaked", "negative", "constant")
MUTANTS = ("kv_next", "q_next", "tail")


def families_for(kv: int):
    """mild, peaked, negative, constant and onehot@t for t in {0, 31, 32, kv - 1} where t < kv."""
    ts = sorted({t for t in (0, 31, 32, kv - 1) if 0 <= t < kv})
    return list(BASE_FAMILIES) + [f"onehot@{t}" for t in ts]


def _seed(kind: str, enc_items: int, P: int, heads: int, kv: int, dtype) -> int:
    return (sum(ord(c) * (i + 1) for i, c in enumerate(kind)) * 1009 + kv * 7919 + P * 131 + enc_items * 17 + heads * 3
            + (0 if dtype == torch.float16 else 1)) % (2 ** 31)


def make_multi(kind: str, enc_items: int, P: int, heads: int, kv: int, dtype=torch.float16):
    """q [enc_items * P, heads, 32, 64], k, v [enc_items, heads, kv, 64], already rounded to ``dtype``.  The families of
    attention_cases.make_qkv, with whatever a family shares between q and k shared per encoder item:

    mild / peaked   independent noise (x 3 on q and k for peaked)
    negative        q = 0.3 noise + a, k = 0.3 noise - a with a ~ 2 N(0, 1) per (encoder item, head)
    constant        all keys of an (encoder item, head) equal
    onehot@t        every query of an encoder item is base + 0.05 noise (the noise differs per prompt slot and row), key t equals base,
                    the other keys are small"""
    g = torch.Generator().manual_seed(_seed(kind, enc_items, P, heads, kv, dtype))
    N = enc_items * P
    q = torch.randn(N, heads, Q_ROWS, HD, generator=g) * 0.75
    k = torch.randn(enc_items, heads, kv, HD, generator=g) * 0.75
    v = torch.randn(enc_items, heads, kv, HD, generator=g) * 0.75
    if kind == "mild":
        pass
    elif kind == "peaked":
        q, k = q * 3, k * 3
    elif kind == "negative":
        a = torch.randn(enc_items, heads, 1, HD, generator=g) * 2.0
        q, k = q * 0.3 + a.repeat_interleave(P, 0), k * 0.3 - a
    elif kind == "constant":
        k = torch.randn(enc_items, heads, 1, HD, generator=g).expand(enc_items, heads, kv, HD).clone()
    elif kind.startswith("onehot@"):
        t = int(kind.split("@")[1])
        assert 0 <= t < kv, (kind, kv)
        base = torch.randn(enc_items, heads, 1, HD, generator=g)
        q = base.repeat_interleave(P, 0) + 0.05 * torch.randn(N, heads, Q_ROWS, HD, generator=g)
        k = k * 0.05
        k[:, :, t] = base[:, :, 0]
    else:
        raise ValueError(kind)
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    worst = (q.float() @ k.float().repeat_interleave(P, 0).transpose(-1, -2)).abs().max().item() * LOG2E / math.sqrt(HD)
    assert worst <= MAX_LOG2_SCORE, (kind, kv, worst)
    return q, k, v


def multi_ref(q, k, v, P: int):
    """softmax(q k^T / 8) v in float64, chain item n over the K / V of encoder item n // P.  Returns (out [N, heads, 32, 64], bound)."""
    u = U[q.dtype]
    kv = k.shape[-2]
    qd, kd, vd = q.double(), k.double().repeat_interleave(P, 0), v.double().repeat_interleave(P, 0)
    s = qd @ kd.transpose(-1, -2) / math.sqrt(HD)
    p = torch.softmax(s, -1)
    out = p @ vd
    bound = 4 * u * (p @ vd.abs()) + kv * 2.0 ** -24 * vd.abs().amax(-2, keepdim=True)
    return out, bound


def emulate(q, k, v, P: int, mutant=None):
    """The core's arithmetic in fp32 / T torch (module docstring).  ``mutant``: one of MUTANTS, or None."""
    T = q.dtype
    N, enc_items, kv = q.shape[0], k.shape[0], k.shape[-2]
    item = torch.arange(N) // P
    if mutant == "kv_next":
        item = (item + 1) % enc_items
    qq = q
    if mutant == "q_next":   # prompt slot p + 1 of the same encoder item
        n = torch.arange(N)
        qq = q[(n // P) * P + (n % P + 1) % P]
    kk, vv = k[item].float(), v[item].float()
    sl2 = torch.tensor(LOG2E / math.sqrt(HD), dtype=torch.float32)
    m = torch.full((N, q.shape[1], Q_ROWS, 1), -1e30, dtype=torch.float32)
    l = torch.zeros_like(m)
    o = torch.zeros(N, q.shape[1], Q_ROWS, HD, dtype=torch.float32)
    for t0 in range(0, kv, TILE):
        tok = torch.arange(t0, t0 + TILE)
        src = tok.clamp(max=kv - 1)          # the staging clamps the token index: padding rows repeat the last key
        s = (qq.float() @ kk[:, :, src].transpose(-1, -2)) * sl2
        if mutant != "tail":
            s = torch.where(tok >= kv, torch.tensor(-float("inf")), s)
        m_new = torch.maximum(m, s.amax(-1, keepdim=True))
        alpha = torch.exp2(m - m_new)
        p = torch.exp2(s - m_new)
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + p.to(T).float() @ vv[:, :, src]
        m = m_new
    return (o / l).to(T)


# ---- the debug entry's buffer layouts -------------------------------------------------------------------------------------------
def pack_rows(x):
    """[N, heads, 32, 64] -> the core's [N][32][heads * 64]."""
    n, h, r, d = x.shape
    return x.transpose(1, 2).reshape(n, r, h * d).contiguous()


def unpack_rows(x, heads: int):
    """[N][32][heads * 64] -> [N, heads, 32, 64]."""
    n, r, w = x.shape
    return x.view(n, r, heads, w // heads).transpose(1, 2)
