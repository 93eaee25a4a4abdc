"""Shared by tests/test_self_attn_bwd_cases_cpu.py and tests/test_gpu_self_attn_bwd.py (not a test module): the attention backward core
(``attn_bwd_mfma_kernel``, csrc/backward.hip) in the masked SELF-attention form of ``mra_qformer_backward`` -- Q, K, V in place in the packed
``[items][S][3 H]`` rows of the QKV GEMM, dQ | dK | dV into rows of the same layout, an int64 ``[items][S]`` key mask, q_rows = kv_len = S.
Seeded inputs (the families, masks and packing of tests/qformer_kernel_cases.py plus an upstream gradient), the float64 reference, a DERIVED
per-element bound, a plain fp32 / T emulation of the kernel's arithmetic and named mutants.  Pure torch on the CPU.

Shapes: q, k, v, o, d_o, dq, dk, dv [items, heads, S, 64]; mask [items, S] int64 or None; lse [items, heads, S] in log2 units, mask included.

---- reference (float64 on the rounded operands) -----------------------------------------------------------------------------------------
    s = q k^T / 8 + (1 - m) * -10000       p = softmax(s)       o = p v       lse = logsumexp(s) log2(e)
    dP = dO v^T      delta = sum_d dO o      dS = p (dP - delta) / 8      dQ = dS k      dK = dS^T q      dV = p^T dO
The mask acts on keys only: a query row whose own key is masked still receives dQ and contributes to dK / dV.

---- bound (per element, worst case, first order; u = U[T], u32 = 2^-24; nothing here was fitted to GPU output) ---------------------------
The kernel recomputes p = exp2(fl(fl(acc sl2) + mt) - lse) from the fp32 score accumulator ``acc``, sl2 = fl(0.125 fl(log2 e)) and the
mask term mt = fl((1 - m) fl(-10000 fl(log2 e))).  Error of the exp2 argument, in log2 units, with y = s log2(e) (mask included):
    64 u32 sl2 (|q| . |k|)    fp32 accumulation of the 64 products of a score, any order
    3 u32 |y|                 sl2 (1 rounding), the product (1), the mask add (1)
    u32 |y - lse|             the subtraction
    e_lse                     the lse handed in: u32 |lse| for the float64 value rounded to fp32, qformer_kernel_cases.attn_ref's lse_bound
                              when attn_kernel wrote it
    2^-10 on items whose mask is all zero: there every y is near -14427, where fp32 numbers are 2^-10 apart; the constant
                              fl(-10000 fl(log2 e)) (two roundings of a 14427) differs from the reference's -10000 log2(e) by up to that, and
                              unlike in the forward it does not cancel against an lse that was computed elsewhere
    rp = 2^(that sum) - 1 + 2 u32 (v_exp_f32: 1 ulp per AMD's ISA documents, taken as 2 u32), and 2^-126 absolute (no fp32 subnormals leave it).
On masked keys of an item with attended keys p is exactly 0 on both sides (exp2 of -14427), whatever rp says.
    dP      64 u32 (|dO| . |v|)
    delta   (u + 72 u32) sum_d |dO| |o|: the kernel reads O rounded to T (u), adds 8 products per lane in sequence and crosses 8 lanes (72 covers
            any order of the 64 products and their roundings); when O is attn_kernel's, + sum_d |dO| ctx_bound
    dS      |dS| (rp + 3 u32) + p / 8 (e_dP + e_delta)        (the subtraction, the product; the factor 1/8 is exact)
    P, dS rounded to T before the MFMAs: u each, + 2^-25 (half the spacing of f16 subnormals)
    each product (dV = P^T dO, dK = dS^T q, dQ = dS k): the operand's error matrix against |the other operand|, + (S + 8) u32 of the product of
            magnitudes for the fp32 accumulation of up to S terms in any order (dQ crosses the key blocks through fp32 LDS adds: 32 + ceil(S / 32)
            <= S + 8 links), + u (|ref| + bound) + 2^-25 [f16] for the one rounding of the output.

---- emulation and mutants ---------------------------------------------------------------------------------------------------------------
``emulate`` does what the kernel does in fp32 / T torch (tests/multi_train_cases.emulate_bwd plus the additive mask in fp32 log2 units).
    mask_ignored     no mask term                                              ragged / holes / zero_row
    mask_item0       item 0's mask row for every item                          ragged
    mask_block0      key block kb takes the mask term of block 0 (tok % 32)     S >= 33, ragged / holes / zero_row
    qblock0          dK / dV from the first query block only                   S >= 33
    round2_dropped   key blocks 4 and up never processed                       S >= 129
    qclamp_counted   the clamped copies of the last query row counted into dK / dV     S % 32 != 0
    masked_q_zero    dS zeroed on query rows whose own key is masked            ragged / holes / zero_row
(``ragged`` and ``holes`` have a zero only from S = 33 on: the 32 query columns are always attended.)"""
import math
from types import SimpleNamespace

import torch

import qformer_kernel_cases as K
from qformer_kernel_cases import HD, LOG2E, MASK_ADD, MASK_KINDS, U, U32, worst_ratio  # noqa: F401  (re-exported for the tests)

BWD_S = (32, 33, 41, 64, 65, 129, 160, 161, 257, 448)
FAMILIES = ("mild", "peaked")
MUTANTS = ("mask_ignored", "mask_item0", "mask_block0", "qblock0", "round2_dropped", "qclamp_counted", "masked_q_zero")
MAX_S = 448            # ceil(S / 32) <= 14 query blocks: what the kernel's LDS holds
ZERO_ROW_ARG = 2.0 ** -10
EXP_FLUSH = 2.0 ** -126
DELTA_DEPTH = 72


def make_grad(items: int, heads: int, S: int, dtype):
    """The upstream gradient d_o [items, heads, S, 64]: seeded 0.5 N(0, 1), rounded to ``dtype``."""
    g = torch.Generator().manual_seed(977 * S + 31 * heads + 7 * items + (0 if dtype == torch.float16 else 1))
    return (torch.randn(items, heads, S, HD, generator=g) * 0.5).to(dtype)


def bwd_ref(q, k, v, d_o, mask):
    """float64 reference with its intermediates (module docstring)."""
    qd, kd, vd, gd = q.double(), k.double(), v.double(), d_o.double()
    s = qd @ kd.transpose(-1, -2) / math.sqrt(HD)
    if mask is not None:
        s = s + ((1 - mask).double() * MASK_ADD)[:, None, None, :]
    p = torch.softmax(s, -1)
    o = p @ vd
    lse = torch.logsumexp(s, -1) * LOG2E
    dP = gd @ vd.transpose(-1, -2)
    delta = (gd * o).sum(-1, keepdim=True)
    dS = p * (dP - delta) / 8
    return SimpleNamespace(s=s, p=p, o=o, lse=lse, dP=dP, delta=delta, dS=dS, dq=dS @ kd, dk=dS.transpose(-1, -2) @ qd, dv=p.transpose(-1, -2) @ gd)


def bwd_bound(q, k, v, d_o, mask, r, lse_err=None, ctx_err=None):
    """(dq, dk, dv) bounds of the module docstring around the reference ``r``.  lse_err [items, heads, S] / ctx_err [items, heads, S, 64]: the
    bounds of an lse / a context that attn_kernel computed; None: the float64 values rounded once (to fp32 / to T)."""
    T = q.dtype
    u, sub = U[T], K.sub_abs(T)
    items, _, S, _ = q.shape
    qa, ka, va, ga = q.double().abs(), k.double().abs(), v.double().abs(), d_o.double().abs()
    y = r.s * LOG2E
    zero_row = torch.zeros(items, dtype=torch.float64) if mask is None else (mask.sum(-1) == 0).double()
    e_lse = U32 * r.lse.abs() if lse_err is None else lse_err
    e_arg = U32 * (64 * (LOG2E / 8) * (qa @ ka.transpose(-1, -2)) + 3 * y.abs() + (y - r.lse[..., None]).abs()) + e_lse[..., None] \
        + ZERO_ROW_ARG * zero_row[:, None, None, None]
    rp = torch.exp2(e_arg) - 1.0 + 2 * U32
    e_p = r.p * rp + EXP_FLUSH
    e_dP = 64 * U32 * (ga @ va.transpose(-1, -2))
    e_delta = (u + DELTA_DEPTH * U32) * (ga * r.o.abs()).sum(-1, keepdim=True)
    if ctx_err is not None:
        e_delta = e_delta + (ga * ctx_err).sum(-1, keepdim=True)
    e_dS = r.dS.abs() * (rp + 3 * U32) + r.p / 8 * (e_dP + e_delta) + EXP_FLUSH * (r.dP - r.delta).abs() / 8
    e_p16 = e_p + u * (r.p + e_p) + sub
    e_dS16 = e_dS + u * (r.dS.abs() + e_dS) + sub
    acc = (S + 8) * U32

    def out(err, ref):
        return err + u * (ref.abs() + err) + sub

    bq = out(e_dS16 @ ka + acc * (r.dS.abs() @ ka), r.dq)
    bk = out(e_dS16.transpose(-1, -2) @ qa + acc * (r.dS.abs().transpose(-1, -2) @ qa), r.dk)
    bv = out(e_p16.transpose(-1, -2) @ ga + acc * (r.p.transpose(-1, -2) @ ga), r.dv)
    return bq, bk, bv


def build(kind: str, items: int, heads: int, S: int, dtype, mask_kind: str, chained: bool = False):
    """One case without its S x S intermediates: inputs (q, k, v, d_o in T, mask), what the core is handed (o in T, lse fp32: the float64
    values rounded once), the float64 gradients ``ref`` = (dq, dk, dv) and their bounds ``bound``.  ``chained``: also ``chained_bound``, for an o
    and an lse that attn_kernel computed (its ctx and lse bounds from qformer_kernel_cases.attn_ref added)."""
    q, k, v = K.make_attn(kind, items, heads, S, dtype)
    d_o = make_grad(items, heads, S, dtype)
    mask = K.make_mask(mask_kind, items, S)
    r = bwd_ref(q, k, v, d_o, mask)
    c = SimpleNamespace(q=q, k=k, v=v, d_o=d_o, mask=mask, o=r.o.to(dtype), lse=r.lse.float(), ref=(r.dq, r.dk, r.dv),
                        bound=bwd_bound(q, k, v, d_o, mask, r), key=(kind, items, heads, S, dtype, mask_kind))
    if chained:
        _, ctx_bound, _, lse_bound = K.attn_ref(q, k, v, mask)
        c.chained_bound = bwd_bound(q, k, v, d_o, mask, r, lse_err=lse_bound, ctx_err=ctx_bound)
    return c


def emulate(q, k, v, o, d_o, lse, mask, mutant=None):
    """The kernel's arithmetic in fp32 / T torch: delta = sum_d dO O in fp32 from the 16-bit rows, fp32 scores and dP of the 16-bit operands,
    P = exp2(s sl2 + mt - lse) with the fp32 mask term mt per key, dS = P (dP - delta) / 8, P and dS rounded to T before the dV / dK / dQ
    products, fp32 accumulation, one rounding to T.  o in T, lse fp32.  Returns dq, dk, dv in T; keys a mutant never stores come out zero."""
    T = q.dtype
    items, _, S, _ = q.shape
    f32 = torch.float32
    qf, kf, vf, gf = q.float(), k.float(), v.float(), d_o.float()
    sl2 = torch.tensor(0.125, dtype=f32) * torch.tensor(LOG2E, dtype=f32)
    delta = (gf * o.float()).sum(-1, keepdim=True)
    mt = torch.zeros(items, S, dtype=f32)
    if mask is not None and mutant != "mask_ignored":
        m = mask[:1].expand(items, -1) if mutant == "mask_item0" else mask
        mt = (1.0 - m.to(f32)) * (torch.tensor(MASK_ADD, dtype=f32) * torch.tensor(LOG2E, dtype=f32))
        if mutant == "mask_block0":
            mt = mt[:, torch.arange(S) % 32]
    y = (qf @ kf.transpose(-1, -2)) * sl2 + mt[:, None, None, :]
    p = torch.exp2(y - lse.float()[..., None])
    ds = p * (gf @ vf.transpose(-1, -2) - delta) * torch.tensor(0.125, dtype=f32)
    if mutant == "masked_q_zero" and mask is not None:
        ds = ds * mask.to(f32)[:, None, :, None]
    p16, ds16 = p.to(T).float(), ds.to(T).float()
    keys = min(S, 128) if mutant == "round2_dropped" else S
    rows = min(S, 32) if mutant == "qblock0" else S
    dq = ds16[..., :keys] @ kf[:, :, :keys]
    dk = ds16[:, :, :rows].transpose(-1, -2) @ qf[:, :, :rows]
    dv = p16[:, :, :rows].transpose(-1, -2) @ gf[:, :, :rows]
    if mutant == "qclamp_counted":
        extra = (S + 31) // 32 * 32 - S
        dk = dk + extra * (ds16[:, :, S - 1:].transpose(-1, -2) @ qf[:, :, S - 1:])
        dv = dv + extra * (p16[:, :, S - 1:].transpose(-1, -2) @ gf[:, :, S - 1:])
    if keys < S:
        dk[:, :, keys:] = 0.0
        dv[:, :, keys:] = 0.0
    return dq.to(T), dk.to(T), dv.to(T)


def ratios(got, ref, bound):
    """Worst |d| / bound of (dq, dk, dv), each over every element."""
    return tuple(worst_ratio(g, r, b) for g, r, b in zip(got, ref, bound))


def pack_rows(x):
    """[items, heads, S, 64] -> [items, S, heads * 64] (the context's layout)."""
    n, h, S, d = x.shape
    return x.transpose(1, 2).reshape(n, S, h * d).contiguous()


def unpack_dqkv(dqkv, heads: int):
    """[items, S, 3 * heads * 64] -> (dq, dk, dv), each [items, heads, S, 64]."""
    n, S, _ = dqkv.shape
    t = dqkv.view(n, S, 3, heads, HD).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]
