"""Shared by tests/test_lm_step_cases_cpu.py and tests/test_gpu_lm_step.py (not a test module): the case tables, seeded inputs rounded to the
operand type, the float64 reference, DERIVED bounds and the fp32 emulation (with named mutants) of the launches of csrc/lm_step.hip behind
``mra_lm_step`` / ``mra_debug_lm_skinny``.  Pure torch on the CPU.  Conventions as tests/decode_attn_cases.py: u32 = 2^-24, u = U[T] (2^-11 f16,
2^-8 bf16), every bound worst case and first order, nothing fitted to GPU output; a sum whose order is not fixed here is bounded as a sum in
ANY order at one u32 per link.  The per-launch reference is float64 on the ROUNDED operands.

---- one launch ------------------------------------------------------------------------------------------------------------------------------
Prologue (its own launch): ms = mean x^2 (K fmas and a tree: K links), rs = rsqrt(ms + eps) (the division, the sum, rsqrtf to 2 ulp), so rs
carries a relative error of (K / 2 + 8) u32 -- the square root halves the sum's K u32 -- and xn = (x rs) g two more roundings:
    e_xn[k] = (K / 2 + 10) u32 |xn_k|                                        (no norm: x is exact, e_xn = 0)
Product y_n = sum_k xn_k w_nk: K fmas over the lanes' chunks and a butterfly, at most K links; xn is fp32, w exact:
    e_y[n]  = sum_k e_xn[k] |w_nk| + (K + 8) u32 sum_k |xn_k| |w_nk|  =  (K + 8 + K / 2 + 10) u32 sum_k |xn_k w_nk|   -- the (K + c) u32 sum |x w| form
LoRA: u_j = sum_k A_jk xn_k as the product above, e_u[j] = (K + 8 + K / 2 + 10) u32 sum_k |A_jk xn_k|; t_n = sum_j u_j B_nj (R fmas), then one
fma with the scale:
    e_l[n]  = |s| (sum_j e_u[j] |B_nj| + (R + 2) u32 sum_j |u_j B_nj|) + 2 u32 |s t_n|
    e[n]    = e_y[n] + e_l[n]                                                 error of the fp32 value the epilogue starts from
Epilogues, v the fp32 value before the store, then ONE rounding to T:  b = e_v + u (|v| + e_v) + 2^-25 [f16: the subnormal spacing]
    plain     v = y                         e_v = e               (fp32 output: b = e_v, no rounding)
    residual  v = y + r                     e_v = e + u32 |v|
    SwiGLU    v = silu(g) up                e_v = (|up| + e_up) (1.1 e_g + 8 u32 |silu g|) + |silu g| e_up + u32 |v|
              (|silu'| <= 1.1; expf to 2 ulp, the sum, the division and the product: 8 u32 taken)
    rotary    v = y c + o s, o = -+ y[partner]    e_v = |c| e + |s| e[partner] + 3 u32 (|y c| + |o s|)       (cos / sin are exact fp32 operands)

---- the chain ------------------------------------------------------------------------------------------------------------------------------
(1) The worst-case forward bound, ``step_with_bound``: the float64 definition with, next to every value, a bound on |kernel's value -
reference's value| pushed through every operation by the rules above with the input error added: |W| e_x through a product; through rsqrt,
with d = (2 sum |x| e_x + sum e_x^2) / K,  e_rs = d / (2 (ms + eps - d)^1.5) + (K / 2 + 8) u32 rs  (no bound at all once d >= ms + eps);
silu by |silu'| <= 1.1; a rounding adds u on EACH side, since the reference rounds too: E' = e + u (|r| + e) + u |r|; through the attention
e_z[s] = |scale| (sum_d e_q |k_s| + (|q| + e_q) e_k[s]) + (D + 2) u32 |scale| sum |q k| (only the new slot's k / v carry an error, every
older slot is the same bits on both sides) and with E = max_s e_z every softmax weight moves by at most a factor exp(2 E):
    e_out[d] = (exp(2 E) - 1) sum_s p_s |v_sd| + exp(2 E) p_slot e_v[d] + 2 (S + 40) u32 sum_s p_s |v_sd|
This bound is VACUOUS, and tests/test_lm_step_cases_cpu.py evaluates it to show that: on a 2-layer Llama of hidden 256 the relative bound
is, bf16 (f16): 7.9e-3 (1.1e-3) behind the rounding of q, 4.6e-2 (7.0e-3) on the attention output (one 16-bit ulp on q and k moves a
softmax weight by percents in the worst case), 0.29 (0.045) behind |W_o|'s row sums, and at the second norm d >= ms + eps in bf16 (0.19 of
the rows in f16, gone a layer later): no finite bound reaches any of the 780 logits in either type.
(2) So the chain is held in two ways.  By COMPOSITION (tests/test_gpu_lm_step.py): the step's launches are issued one at a time through the
debug entries on the chain's ACTUAL intermediates, every launch is inside its bound above against float64 of its own inputs, and
``mra_lm_step``'s logits, residual rows and cache slots are the composition's, bit for bit.  And against the DEFINITION, ``lm_step_ref`` in
float64 on the same cache and tokens, at every step, under a stated MARGIN (not a derived bound):
    max |logit - reference| <= CHAIN_ULPS U[T] max |reference logits|,      CHAIN_ULPS = 4
Where it comes from: both sides round at the same places, so apart from fp32 arithmetic (1e-6 of the scale) they differ only where an fp32
difference straddles a 16-bit rounding boundary; such a flip moves ONE element by one ulp (<= 2 u |v|), and through the final norm and the
head a flipped element k of the residual stream moves logit v by 2 u |xn_k w_vk| -- 2 u times one of the K terms of that logit.  The
chance of a flip per rounded value is about (fp32 error) / (16-bit ulp), 1e-4 .. 1e-2 here, over roughly 1e4 rounded values per step: a
few flips per step, each worth a fraction of u on the logit scale.  Four ulps of the largest logit leave room for that and stay far below
any wiring error (each step mutant misses the margin, by a factor of 4 .. 90 in bf16 and 30 .. 720 in f16: asserted in the CPU test).  Measured on the MI355X over
every one of the 23 steps of the eight model-level cases (after the margin was set): worst 1.14 U[f16] and 1.04 U[bf16] of the scale, 0.29 and
0.26 of the margin (5.4e-4 and 4.3e-3 absolute on a scale of 1.35).

Mutants (emulation, ``mutant=``): the list of ``mraudio_amd.models.lm_step.MUTANTS`` plus ``argmax_tie_highest``."""
import functools
import math

import torch

from mraudio_amd.models import lm_step as LS
from train_kernel_cases import F16_SUB, U, U32, _gen, ratio  # noqa: F401

F32, F64 = torch.float32, torch.float64
DTYPES = (torch.float16, torch.bfloat16)
PLAIN, RES, SWIGLU, ROPE = 0, 1, 2, 3
CB = 16                                        # LM_CB of csrc/kernels.h: columns per workgroup (the rotary form: D)
NS = (CB - 1, CB, CB + 1, 2 * CB + CB // 2)    # one column block - 1, exact, + 1, 2.5 blocks
EPS = 1e-6
MUTANTS = LS.MUTANTS + ("argmax_tie_highest",)
HEAD_V = (1, 63, 64, 65, 260, 2200)
CHAIN_ULPS = 4                                 # the stated margin of the chain against lm_step_ref in float64 (docstring, "the chain" (2))


def chain_margin(ref_logits, dtype) -> float:
    return CHAIN_ULPS * U[dtype] * ref_logits.abs().max().item()


def up256(n: int) -> int:
    return (n + 255) // 256 * 256


def skinny_workspace_bytes(B: int, K: int) -> int:
    """include/mra.h mra_debug_lm_skinny: up(4 B K) + 3 up(64 B)."""
    return up256(4 * B * K) + 3 * up256(4 * B * 16)


def skinny_cases():
    """dict(epi, B, K, N (per segment), R (per segment), norm, f32, pitch[, D, Hq, Hkv]).  B in {1, 2, 3, 8}, K in {8, 64, 72, 264, 1032}, N around
    the column block, one to three segments of different N, R in {0, 3, 8, 16}, pitched W and x, every epilogue, D and Hq / Hkv of the rotary form."""
    c = []
    add = lambda epi, B, K, N, R, norm, f32=False, pitch=False, **kw: c.append(dict(epi=epi, B=B, K=K, N=N, R=R, norm=norm, f32=f32, pitch=pitch, **kw))
    add(PLAIN, 1, 8, (15,), (0,), False)
    add(PLAIN, 2, 64, (16, 17), (3, 0), True, pitch=True)
    add(PLAIN, 3, 72, (17, 40, 15), (8, 16, 0), True, f32=True)
    add(PLAIN, 8, 264, (40,), (16,), False, pitch=True)
    add(PLAIN, 3, 1032, (16,), (0,), True, f32=True, pitch=True)
    add(RES, 1, 72, (17,), (3,), False, pitch=True)
    add(RES, 8, 1032, (40,), (0,), False)
    add(RES, 2, 264, (16,), (8,), False)
    add(RES, 3, 8, (15,), (16,), False, pitch=True)
    add(SWIGLU, 1, 264, (40, 40), (0, 0), True)
    add(SWIGLU, 3, 64, (15, 15), (8, 3), True, pitch=True)
    add(SWIGLU, 8, 72, (17, 17), (16, 0), True)
    add(SWIGLU, 2, 1032, (16, 16), (3, 8), False, pitch=True)
    add(SWIGLU, 2, 8, (17, 17), (0, 16), True)
    for B, K, D, Hq, Hkv, R, pitch in ((3, 72, 64, 4, 4, (8, 0, 3), True), (1, 264, 128, 4, 2, (0, 0, 0), False), (2, 64, 64, 4, 1, (16, 16, 16), True),
                                       (8, 1032, 128, 2, 2, (3, 8, 0), False), (3, 8, 128, 4, 1, (0, 3, 16), True), (2, 264, 64, 2, 1, (8, 8, 8), False)):
        add(ROPE, B, K, (Hq * D, Hkv * D, Hkv * D), R, True, pitch=pitch, D=D, Hq=Hq, Hkv=Hkv)
    return c


def case_id(c) -> str:
    return f"{('plain', 'res', 'swiglu', 'rope')[c['epi']]}-B{c['B']}-K{c['K']}-N{'_'.join(map(str, c['N']))}-R{'_'.join(map(str, c['R']))}" \
           f"{'-norm' if c['norm'] else ''}{'-f32' if c['f32'] else ''}{'-pitch' if c['pitch'] else ''}"


def make_case(c, dtype):
    """Seeded operands of a launch, rounded to ``dtype`` (adapters, cos / sin fp32).  x [B, ldx], W_s [N_s, ldw] are the padded buffers; the
    padding holds NaN (never read)."""
    g = _gen(c["epi"], c["B"], c["K"], sum(c["N"]), sum(c["R"]), dtype == torch.float16)
    B, K = c["B"], c["K"]
    ldx, ldw = (K + 16, K + 8) if c["pitch"] else (K, K)
    t = {"ldx": ldx, "ldw": ldw}
    x = torch.full((B, ldx), float("nan"))
    x[:, :K] = torch.randn(B, K, generator=g)
    t["x"] = x.to(dtype)
    t["gain"] = (1 + 0.3 * torch.randn(K, generator=g)).to(dtype) if c["norm"] else None
    t["W"], t["A"], t["Bw"], t["scale"] = [], [], [], []
    for N, R in zip(c["N"], c["R"]):
        W = torch.full((N, ldw), float("nan"))
        W[:, :K] = torch.randn(N, K, generator=g) / math.sqrt(K)
        t["W"].append(W.to(dtype))
        t["A"].append(torch.randn(R, K, generator=g) / math.sqrt(K) if R else None)
        t["Bw"].append(torch.randn(N, R, generator=g) * 0.5 if R else None)
        t["scale"].append(2.0 / R if R else 0.0)
    if c["epi"] == RES:
        t["res"] = torch.randn(B, c["N"][0], generator=g).to(dtype)
    if c["epi"] == ROPE:
        D = c["D"]
        rows = 40
        t["slot"], t["Smax"], t["pos_offset"] = 5, 9, 3
        t["position"] = torch.tensor([(7 * b + 4) % (rows - 4) for b in range(B)], dtype=torch.int32)      # + 3: unequal to the slot, different per row
        inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
        ang = torch.arange(rows).float()[:, None] * inv[None, :]
        t["cos"], t["sin"] = torch.cat([ang.cos(), ang.cos()], 1).contiguous(), torch.cat([ang.sin(), ang.sin()], 1).contiguous()
    return t


def _launch(c, t, ct, mutant=None):
    """The fp value every output element has in front of its store, in ``ct``: dict(out=[per segment], k=, v=) -- the definition of the launch."""
    B, K = c["B"], c["K"]
    x = t["x"][:, :K].to(ct)
    if c["norm"]:
        x = LS.rms_ref(x, t["gain"], EPS, mutant)
    ys = [LS.linear_ref(x, W[:, :K], A, Bw, s, None if mutant == "lora_after_rotation" else mutant)
          for W, A, Bw, s in zip(t["W"], t["A"], t["Bw"], t["scale"])]
    if c["epi"] == PLAIN:
        return dict(out=ys)
    if c["epi"] == RES:
        return dict(out=[ys[0] if mutant == "residual_dropped" else ys[0] + t["res"].to(ct)])
    if c["epi"] == SWIGLU:
        return dict(out=[LS.swiglu_ref(ys[0], ys[1], mutant)])
    D, Hq, Hkv = c["D"], c["Hq"], c["Hkv"]
    pos = t["position"].long() + t["pos_offset"]
    if mutant == "position_from_slot":
        pos = torch.full_like(pos, t["slot"])
    cos, sin = t["cos"][pos].to(ct), t["sin"][pos].to(ct)
    if mutant == "lora_after_rotation":
        base = [x @ W[:, :K].to(ct).T for W in t["W"][:2]]
        q = LS.rope_ref(base[0].view(B, Hq, D), cos, sin) + (ys[0] - base[0]).view(B, Hq, D)
        k = LS.rope_ref(base[1].view(B, Hkv, D), cos, sin) + (ys[1] - base[1]).view(B, Hkv, D)
    else:
        q, k = LS.rope_ref(ys[0].view(B, Hq, D), cos, sin, mutant), LS.rope_ref(ys[1].view(B, Hkv, D), cos, sin, mutant)
    return dict(out=[q.reshape(B, Hq * D)], k=k, v=ys[2].view(B, Hkv, D))


@functools.lru_cache(maxsize=None)
def _reference(ci: int, dtype):
    c = skinny_cases()[ci]
    t = make_case(c, dtype)
    return c, t, _launch(c, t, F64), bounds(c, t, dtype)


def reference(ci: int, dtype):
    """(case, tensors, float64 values, bounds), computed once and shared; leave them unchanged."""
    return _reference(ci, dtype)


def emulate(ci: int, dtype, mutant=None):
    """The launch in fp32 with its one rounding (fp32 output: none), as the kernels compute it up to the order of their sums."""
    c, t, _, _ = reference(ci, dtype)
    got = _launch(c, t, F32, mutant)
    rd = (lambda v: v) if c["f32"] else (lambda v: v.to(dtype))
    out = dict(out=[rd(v) for v in got["out"]])
    if c["epi"] == ROPE:
        out["k"], out["v"] = got["k"].to(dtype), got["v"].to(dtype)
        out["slot"] = t["slot"]
        if mutant == "slot_from_position":
            out["slot"] = int(t["position"][0]) + t["pos_offset"]
    return out


def bounds(c, t, dtype):
    """Per-element bounds of the docstring for every output of the launch: dict(out=[...], k=, v=), float64."""
    B, K = c["B"], c["K"]
    u = U[dtype]
    x = t["x"][:, :K].to(F64)
    cn = 0.0
    if c["norm"]:
        x = LS.rms_ref(x, t["gain"], EPS)
        cn = K / 2 + 10
    ca = K + 8 + cn
    es, ys = [], []
    for W, A, Bw, s in zip(t["W"], t["A"], t["Bw"], t["scale"]):
        Wd = W[:, :K].to(F64)
        y = x @ Wd.T
        e = ca * U32 * (x.abs() @ Wd.abs().T)
        if A is not None:
            Ad, Bd = A.to(F64), Bw.to(F64)
            uu = x @ Ad.T
            e_u = ca * U32 * (x.abs() @ Ad.abs().T)
            tt = uu @ Bd.T
            e = e + abs(s) * (e_u @ Bd.abs().T + (Bd.shape[1] + 2) * U32 * (uu.abs() @ Bd.abs().T)) + 2 * U32 * (s * tt).abs()
            y = y + s * tt
        es.append(e)
        ys.append(y)
    sub = F16_SUB if dtype == torch.float16 else 0.0

    def store(v, e):
        return e if c["f32"] else e + u * (v.abs() + e) + sub

    if c["epi"] == PLAIN:
        return dict(out=[store(y, e) for y, e in zip(ys, es)])
    if c["epi"] == RES:
        v = ys[0] + t["res"].to(F64)
        return dict(out=[store(v, es[0] + U32 * v.abs())])
    if c["epi"] == SWIGLU:
        g, up = ys
        sg = g * torch.sigmoid(g)
        v = sg * up
        return dict(out=[store(v, (up.abs() + es[1]) * (1.1 * es[0] + 8 * U32 * sg.abs()) + sg.abs() * es[1] + U32 * v.abs())])
    D, Hq, Hkv = c["D"], c["Hq"], c["Hkv"]
    pos = t["position"].long() + t["pos_offset"]
    cos, sin = t["cos"][pos].to(F64)[:, None, :], t["sin"][pos].to(F64)[:, None, :]

    def rot(y, e, H):
        y, e = y.view(B, H, D), e.view(B, H, D)
        h = D // 2
        o, eo = torch.cat([-y[..., h:], y[..., :h]], -1), torch.cat([e[..., h:], e[..., :h]], -1)
        v = y * cos + o * sin
        return v, cos.abs() * e + sin.abs() * eo + 3 * U32 * ((y * cos).abs() + (o * sin).abs())

    q, eq = rot(ys[0], es[0], Hq)
    k, ek = rot(ys[1], es[1], Hkv)
    return dict(out=[store(q, eq).reshape(B, Hq * D)], k=store(k, ek), v=store(ys[2].view(B, Hkv, D), es[2].view(B, Hkv, D)))


def ratios(ci: int, dtype, got) -> float:
    """The worst |got - reference| / bound over every output of the launch (``got`` as ``emulate`` returns it)."""
    c, _, ref, bnd = reference(ci, dtype)
    worst = max(ratio(g, r, b) for g, r, b in zip(got["out"], ref["out"], bnd["out"]))
    if c["epi"] == ROPE:
        worst = max(worst, ratio(got["k"], ref["k"], bnd["k"]), ratio(got["v"], ref["v"], bnd["v"]))
    return worst


# ---- the head's argmax ------------------------------------------------------------------------------------------------------------------------
def argmax_case(V: int, B: int = 3):
    """fp32 logits [B, V] with planted ties (the maximum at two or three indices) in every row, a NaN in the last row (and a second NaN behind it)."""
    g = _gen(V, B, 17)
    z = torch.randn(B, V, generator=g)
    for b in range(B):
        hi = z[b].max() + 1.0
        for i in {(5 * b + 3) % V, (V - 1 - b) % V, (V // 2 + b) % V}:
            z[b, i] = hi
    if V > 2:
        z[B - 1, (V // 3) + 1] = float("nan")
        z[B - 1, V - 1] = float("nan")
    return z


# ---- the chain: the worst-case forward bound (vacuous; kept so that the claim can be checked) --------------------------------------------------
def _lin_b(x, ex, mod):
    """(value, bound) of a (possibly adapted) linear on x [B, K] with input bound ex, float64."""
    W, A, Bw, s = LS.split_linear(mod)
    Wd = W.to(F64)
    K = Wd.shape[1]
    ca = 1.01 * (K + 8) * U32
    y = x @ Wd.T
    e = ex @ Wd.abs().T + ca * ((x.abs() + ex) @ Wd.abs().T)
    if A is not None:
        Ad, Bd = A.to(F64), Bw.to(F64)
        uu = x @ Ad.T
        e_u = ex @ Ad.abs().T + ca * ((x.abs() + ex) @ Ad.abs().T)
        tt = uu @ Bd.T
        e = e + abs(s) * (e_u @ Bd.abs().T + 1.01 * (Bd.shape[1] + 2) * U32 * ((uu.abs() + e_u) @ Bd.abs().T)) + 2 * U32 * (abs(s) * (tt.abs() + e_u @ Bd.abs().T))
        y = y + s * tt
    return y, e


def _rms_b(x, ex, gain, eps):
    K = x.shape[-1]
    g = gain.to(F64)
    ms = (x * x).mean(-1, keepdim=True)
    rs = torch.rsqrt(ms + eps)
    d = (2 * (x.abs() * ex).sum(-1, keepdim=True) + (ex * ex).sum(-1, keepdim=True)) / K
    room = ms + eps - d
    e_rs = torch.where(room > 0, d / (2 * room.clamp_min(1e-300) ** 1.5), torch.full_like(d, float("inf"))) + 1.01 * (K / 2 + 8) * U32 * rs
    xn = x * rs * g
    e = g.abs() * ((x.abs() + ex) * e_rs + rs * ex)
    return xn, e + 3 * U32 * (xn.abs() + e)


def _rd_b(v, e, dtype):
    """Both sides round: (rounded reference, e + u (|r| + e) + u |r|)."""
    u = U[dtype]
    sub = 2 * F16_SUB if dtype == torch.float16 else 0.0
    return v.to(dtype).to(F64), e + u * (v.abs() + e) + u * v.abs() + sub


@torch.no_grad()
def step_with_bound(llm, tokens, cache, mask, positions, slot, dtype, rope, trace=None):
    """``lm_step_ref`` in float64 with ``dtype`` roundings, carrying the worst-case bound of the docstring: (logits, bound on the kernel's
    logits).  ``trace`` (a list) receives (stage, max bound / max |value|) per stage of the first layer.  ``cache`` is written."""
    w = LS.walk(llm)
    B, Hq, Hkv, D = tokens.shape[0], w["Hq"], w["Hkv"], w["D"]
    G, S = Hq // Hkv, slot + 1
    h = w["embed"][tokens.long()].to(F64)
    eh = torch.zeros_like(h)
    pos = positions.long()
    cos, sin = rope[0][pos].to(F64)[:, None, :], rope[1][pos].to(F64)[:, None, :]
    on = mask[:, :S].to(torch.bool)
    note = (lambda name, v, e: trace.append((name, (e.max() / v.abs().max()).item()))) if trace is not None else (lambda *a: None)

    def rot(y, e, H):
        y, e = y.view(B, H, D), e.view(B, H, D)
        hh = D // 2
        o, eo = torch.cat([-y[..., hh:], y[..., :hh]], -1), torch.cat([e[..., hh:], e[..., :hh]], -1)
        return y * cos + o * sin, cos.abs() * e + sin.abs() * eo + 3 * U32 * (((y.abs() + e) * cos.abs()) + ((o.abs() + eo) * sin.abs()))

    for l, rec in enumerate(w["layers"]):
        xn, exn = _rms_b(h, eh, rec["norm1"], w["eps"])
        (q, eq), (k, ek), (v, ev) = (_lin_b(xn, exn, rec[n]) for n in ("q", "k", "v"))
        q, eq = _rd_b(*rot(q, eq, Hq), dtype)
        k, ek = _rd_b(*rot(k, ek, Hkv), dtype)
        v, ev = _rd_b(v.view(B, Hkv, D), ev.view(B, Hkv, D), dtype)
        cache[l, 0, :, :, slot], cache[l, 1, :, :, slot] = k.to(cache.dtype), v.to(cache.dtype)
        idx = torch.arange(Hq) // G
        kf, vf = cache[l, 0, :, :, :S].to(F64)[:, idx], cache[l, 1, :, :, :S].to(F64)[:, idx]        # [B, Hq, S, D]
        vf = torch.where(on[:, None, :, None], vf, torch.zeros((), dtype=F64))
        kf = torch.where(on[:, None, :, None], kf, torch.zeros((), dtype=F64))
        sc = abs(rec["scale"])
        z = rec["scale"] * torch.einsum("bhd,bhsd->bhs", q, kf)
        ez = sc * torch.einsum("bhd,bhsd->bhs", eq, kf.abs()) + 1.01 * (D + 2) * U32 * sc * torch.einsum("bhd,bhsd->bhs", q.abs() + eq, kf.abs())
        ez[:, :, slot] += sc * ((q.abs() + eq) * ek[:, idx]).sum(-1)
        z = torch.where(on[:, None, :], z, torch.full((), float("-inf"), dtype=F64))
        ez = torch.where(on[:, None, :], ez, torch.zeros((), dtype=F64))
        p = torch.softmax(z, -1)
        E = ez.max(-1, keepdim=True).values                                                        # [B, Hq, 1]
        pav = torch.einsum("bhs,bhsd->bhd", p, vf.abs())
        ao = torch.einsum("bhs,bhsd->bhd", p, vf)
        eao = torch.expm1(2 * E) * pav + torch.exp(2 * E) * p[:, :, slot, None] * ev[:, idx] + 2 * (S + 40) * U32 * pav
        ao, eao = _rd_b(ao, eao, dtype)
        o, eo = _lin_b(ao.reshape(B, Hq * D), eao.reshape(B, Hq * D), rec["o"])
        if l == 0:
            note("q", q, eq), note("attention output", ao, eao), note("o product", o, eo)
        h, eh = _rd_b(h + o, eh + eo + U32 * ((h + o).abs() + eh + eo), dtype)
        if l == 0:
            note("residual stream behind the attention", h, eh)
        xn, exn = _rms_b(h, eh, rec["norm2"], w["eps"])
        if l == 0:
            note("second norm", xn, exn)
        (g, eg), (up, eu) = _lin_b(xn, exn, rec["gate"]), _lin_b(xn, exn, rec["up"])
        sg = g * torch.sigmoid(g)
        act = sg * up
        eact = (up.abs() + eu) * (1.1 * eg + 8 * U32 * (sg.abs() + 1.1 * eg)) + sg.abs() * eu + U32 * act.abs()
        act, eact = _rd_b(act, eact, dtype)
        dn, edn = _lin_b(act, eact, rec["down"])
        h, eh = _rd_b(h + dn, eh + edn + U32 * ((h + dn).abs() + eh + edn), dtype)
    xn, exn = _rms_b(h, eh, w["final_norm"], w["eps"])
    Wd = w["head"].to(F64)
    K = Wd.shape[1]
    return xn @ Wd.T, exn @ Wd.abs().T + 1.01 * (K + 8) * U32 * ((xn.abs() + exn) @ Wd.abs().T)


# ---- tiny Llamas --------------------------------------------------------------------------------------------------------------------------------
def tiny_llama(kv_heads: int, head_dim: int, vocab: int = 97, layers: int = 2, heads: int = 4, seed: int = 0, lora: bool = False, **cfg_kw):
    """A CPU fp32 ``LlamaForCausalLM`` (hidden = heads * head_dim, RMSNorm gains 1 + 0.3 N(0, 1)); ``lora``: every linear adapted, B non-zero."""
    import transformers as tf

    torch.manual_seed(seed)
    cfg = tf.LlamaConfig(vocab_size=vocab, hidden_size=heads * head_dim, intermediate_size=2 * heads * head_dim + 8, num_hidden_layers=layers,
                         num_attention_heads=heads, num_key_value_heads=kv_heads, max_position_embeddings=512, pad_token_id=0, bos_token_id=1,
                         eos_token_id=2, **cfg_kw)
    llm = tf.LlamaForCausalLM(cfg).eval().requires_grad_(False)
    for n, prm in llm.named_parameters():            # gains away from one, so that a misplaced gain shows
        if "norm" in n:
            prm.data.add_(0.3 * torch.randn(prm.shape))
    if lora:
        add_adapters(llm, seed)
    return llm


def add_adapters(llm, seed: int = 0, r: int = 8):
    from mraudio_amd.models.lora import ADAPTER, apply_lora, lora_modules

    apply_lora(llm, r=r, alpha=16, dropout=0.05)
    g = torch.Generator().manual_seed(seed + 99)
    for m in lora_modules(llm).values():
        Bw = m.lora_B[ADAPTER].weight
        Bw.data.copy_((torch.randn(Bw.shape, generator=g) * 0.05).to(Bw.dtype))
    llm.eval().requires_grad_(False)
    return llm


def prefix(B: int, S0: int, hidden: int, seed: int = 12):
    """[B, S0, hidden] rows and a 0 / 1 mask: left padding in row 1, holes inside row 2 (B >= 3)."""
    g = torch.Generator().manual_seed(seed)
    e = torch.randn(B, S0, hidden, generator=g) * 0.5
    m = torch.ones(B, S0, dtype=torch.long)
    if B > 1:
        m[1, :S0 // 8 + 1] = 0
        m[1, (2 * S0) // 3] = 0
    if B > 2:
        m[2, S0 // 30 + 1: S0 // 30 + 3] = 0
        m[2, S0 // 2: S0 // 2 + 3] = 0
    return e, m
