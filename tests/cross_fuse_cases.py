"""Shared by tests/test_cross_fuse_cases_cpu.py and tests/test_gpu_cross_fuse.py (not a test module): the fused query launch of the folded
cross-attention (csrc/fold.hip fold_query_kernel, ``mra_debug_fold_query``) -- seeded inputs rounded to the operand type, float64 references,
DERIVED bounds and an fp32 emulation with named mutants.  Pure torch on the CPU.  Notation and assumptions as tests/gemm_cases.py
(u32 = 2^-24, u = U[T], an MFMA no worse than a chain of fp32 additions of its exact products).

The launch computes, per head h of 64 dims, over the M = items x 32 compact query rows behind a strided row view of x [items][32 + L][H]:
    phase 1   Q_h  = T(x W_q,h^T + b_q,h)      K = H in 64-deep steps           gemm_cases row 1 (EPI_OP): eK = (H + 1) u32 (|x| |W_q|^T + |b_q|)
    phase 2   Q'_h = T(Q_h W_k,h)              K = 64, one step                 gemm_cases row 9 (EPI_OP): e2 = 65 u32 |Q_h| |W_k,h|^T
and writes q_prime [items][h 32 + q][E].  Q_h never leaves the kernel, so two input kinds hold the two phases to their rows' bounds:

"generic"  random x, W_q, b_q, W_k.  Reference: float64 throughout, Q NOT rounded.  Phase 1's EPI_OP bound
               dQ = round_bound(Q, eK, T)
           is what the Q the kernel holds may be off by; it passes through phase 2 as dQ |W_k|^T, and phase 2's own accumulation sees
           |Q_h| <= |Q| + dQ:
               |Q' - ref| <= round_bound(ref, dQ |W_k|^T + 65 u32 (|Q| + dQ) |W_k|^T, T).
           A dropped bias (|b_q| ~ 0.5 against dQ ~ 1e-3) is far outside.
"grid"     x on a 2^-3 grid in [-2, 2], W_q on a 2^-5 grid in [-1, 1], b_q on a 2^-8 grid: every product is a multiple of 2^-8 and every partial
           sum stays below 2^12, so phase 1's fp32 accumulator is EXACT in any order and Q_h = T(x W_q^T + b_q) is known bit for bit (eK = 0).
           Reference: float64 over that rounded Q_h, and the bound is phase 2's alone,
               |Q' - ref| <= round_bound(ref, 65 u32 |Q_h| |W_k|^T, T).
           A kernel that feeds phase 2 the unrounded accumulator differs by the 64 rounding errors of a row of Q_h (each up to u |Q|), which this
           bound does not hold: the mutant "q_not_rounded" is outside it.

Shapes (the smallest the tiles allow): 12 heads x 32 queries, H = 768, E = 704 (a multiple of 64 and of 176, NOT of 128: the last 128-column
block of phase 2 is half); items 1, 3, 5 -- 96 and 160 rows leave a ragged last 128-row tile, and a row tile straddles items of the strided
view; L = 0 and 9 (rows 32 .. of an item hold NaN: no view addresses them).

---- the context GEMM on the 64 x 64 tile with 128-deep K steps ("cross_fuse" bit 4; mra_gemm_desc.k128) ---------------------------------------
ctx[m][h 64 + d] = T(U_h[m] W_v,h[d]^T + b_v[h 64 + d]) per head h (batch = heads), U [items][h 32 + q][K] behind an item view, gemm_cases row 9's
EPI_OP bound with eK = (K + 1) u32 (|U| |W_v|^T + |b_v|).  M = 96 (one ragged row tile of the present 64 x 128 tile, two of the new one) and
M = 1024 (the headline's rows); K = 384: three 128-deep steps, the smallest count at which both buffers are reused.

---- P . enc fed by the scores launch's tile statistics ("cross_fuse" bit 2; mra_gemm_desc.ps_stats) -------------------------------------------
U[b][m][n] = T(sum_k a'[m][k] enc[b][k][n]), a' = P~[m][k] x g[m][tile(k)] rounded as gemm_cases' pscale rows say, where the launch computes
g = exp2(stat_m[t] - m_row) / L_row itself from the statistics (stat_m, stat_l [b][m][ntiles]) and treats the P~ columns from ntiles x 176 on
as zero WITHOUT reading them (the test leaves NaN there).  Reference: float64 over the P~ and the statistics handed to the launch, factors
from qformer_kernel_cases.factor_ref, whose fp32 bound gb joins the pscale term:  |a' - a g64| <= [pscale term at g64] + |a| gb.
kv = 176 (one tile), 300 (two, ragged: columns 300 .. 351 of the last tile are zeros of the scores launch, 352 .. 383 padding), 1000 (six:
the four-slot ring wraps).  "diffuse": every tile matters; "peaked": one token carries a score ~30 log2 units above the rest, so the other
tiles' factors are below 2^-14 (f16 subnormals or zero).  Two batch entries, so the statistics' batch offset counts.
Mutants the bound must reject: "factor_from_wrong_tile" (tile t takes the maximum of tile t + 1) and "stale_ring_slot" (tile t >= 4 meets the
factors of tile t - 4, what a slot holds when it is not refilled)."""
import functools

import torch

from gemm_cases import ALPHA, DTYPES, F32, F64, U, U32, _gen, factor_ref, fold_kvp, round_bound, sub_abs

HEADS, Q, H, E = 12, 32, 768, 704
ITEMS = (1, 3, 5)
TEXT = (0, 9)
KINDS = ("generic", "grid")
MUTANTS = ("bias_dropped", "q_not_rounded")
REJECTED_BY = {"bias_dropped": "generic", "q_not_rounded": "grid"}   # the input kind whose bound must reject the mutant


@functools.lru_cache(maxsize=None)
def weights(kind: str, dt: str):
    """W_q [H][H], b_q [H] (fp32), W_k per head [HEADS][E][64] -- shared by every (items, L) of a kind."""
    dtype = DTYPES[dt]
    g = _gen(91, KINDS.index(kind))
    if kind == "grid":
        wq = (torch.randint(-32, 33, (H, H), generator=g).to(F32) / 32).to(dtype)
        bq = torch.randint(-128, 129, (H,), generator=g).to(F32) / 256
    else:
        wq = (torch.randn(H, H, generator=g) * 0.05).to(dtype)
        bq = torch.randn(H, generator=g) * 0.5
    wk = (torch.randn(HEADS, E, 64, generator=g) * 0.05).to(dtype)
    return wq, bq, wk


@functools.lru_cache(maxsize=None)
def inputs(kind: str, items: int, L: int, dt: str):
    """x [items][32 + L][H] in the operand type; rows 32 .. of every item are NaN."""
    dtype = DTYPES[dt]
    g = _gen(92, KINDS.index(kind), items, L)
    if kind == "grid":
        xq = torch.randint(-16, 17, (items, Q, H), generator=g).to(F32) / 8
    else:
        xq = torch.randn(items, Q, H, generator=g)
    x = torch.full((items, Q + L, H), float("nan"), dtype=dtype)
    x[:, :Q] = xq.to(dtype)
    return x


def x_view(L: int):
    """(item stride, rows per item, row stride) of the compact query rows inside x."""
    return ((Q + L) * H, Q, H)


def _layout(qh):
    """[HEADS][M][E] -> q_prime [items][HEADS * 32][E]"""
    M = qh.shape[1]
    return qh.view(HEADS, M // Q, Q, E).permute(1, 0, 2, 3).reshape(M // Q, HEADS * Q, E)


@functools.lru_cache(maxsize=None)
def reference(kind: str, items: int, L: int, dt: str):
    """(ref, bound) float64 [items][HEADS * 32][E]"""
    dtype = DTYPES[dt]
    wq, bq, wk = weights(kind, dt)
    x = inputs(kind, items, L, dt)[:, :Q].reshape(items * Q, H).to(F64)
    q = x @ wq.to(F64).T + bq.to(F64)
    absq = x.abs() @ wq.to(F64).abs().T + bq.to(F64).abs()
    if kind == "grid":
        q = q.to(dtype).to(F64)                        # exact accumulator: the rounded Q_h is known
        dq = torch.zeros_like(q)
    else:
        dq = round_bound(q, (H + 1) * U32 * absq, dtype)
    qh = q.view(-1, HEADS, 64).permute(1, 0, 2)         # [HEADS][M][64]
    dqh = dq.view(-1, HEADS, 64).permute(1, 0, 2)
    wk64 = wk.to(F64)
    ref = qh @ wk64.transpose(1, 2)                     # [HEADS][M][E]
    e32 = dqh @ wk64.abs().transpose(1, 2) + 65 * U32 * ((qh.abs() + dqh) @ wk64.abs().transpose(1, 2))
    return _layout(ref), _layout(round_bound(ref, e32, dtype))


def emulate(kind: str, items: int, L: int, dt: str, mutant=None):
    """The launch in fp32 on the CPU: phase 1 adds K step after K step (64 deep), + bias, rounds; phase 2 is one step."""
    dtype = DTYPES[dt]
    wq, bq, wk = weights(kind, dt)
    x = inputs(kind, items, L, dt)[:, :Q].reshape(items * Q, H).float()
    acc = torch.zeros(items * Q, H)
    for k0 in range(0, H, 64):
        acc = acc + x[:, k0:k0 + 64] @ wq.float()[:, k0:k0 + 64].T
    q = acc if mutant == "bias_dropped" else acc + bq
    if mutant != "q_not_rounded":
        q = q.to(dtype).float()
    qh = q.view(-1, HEADS, 64).permute(1, 0, 2)
    return _layout((qh @ wk.float().transpose(1, 2)).to(dtype))


def worst_ratio(out, kind: str, items: int, L: int, dt: str) -> float:
    """max |out - ref| / bound (inf for a NaN)"""
    ref, bound = reference(kind, items, L, dt)
    r = (out.to(F64) - ref).abs() / bound
    return float("inf") if torch.isnan(r).any() else float(r.max())


def buffer_bytes(items: int, L: int):
    """bytes of x, w_q, b_q, w_k, q_prime"""
    return (items * (Q + L) * H * 2, H * H * 2, H * 4, HEADS * E * 64 * 2, items * HEADS * Q * E * 2)


# ---- context GEMM -----------------------------------------------------------------------------------------------------------------------
CTX_K = 384
CTX_M = (96, 1024)


@functools.lru_cache(maxsize=None)
def ctx_inputs(M: int, dt: str):
    """U [items][HEADS * 32][K], W_v [HEADS * 64][K], b_v [HEADS * 64] (fp32)"""
    dtype = DTYPES[dt]
    g = _gen(93, M)
    u = torch.randn(M // Q, HEADS * Q, CTX_K, generator=g).to(dtype)
    wv = (torch.randn(HEADS * 64, CTX_K, generator=g) * 0.05).to(dtype)
    bv = torch.randn(HEADS * 64, generator=g) * 0.5
    return u, wv, bv


@functools.lru_cache(maxsize=None)
def ctx_reference(M: int, dt: str):
    """(ref, bound) float64 [M][HEADS * 64]"""
    dtype = DTYPES[dt]
    u, wv, bv = ctx_inputs(M, dt)
    uh = u.view(M // Q, HEADS, Q, CTX_K).permute(1, 0, 2, 3).reshape(HEADS, M, CTX_K).to(F64)
    wh = wv.view(HEADS, 64, CTX_K).to(F64)
    bh = bv.view(HEADS, 1, 64).to(F64)
    ref = uh @ wh.transpose(1, 2) + bh
    ek = (CTX_K + 1) * U32 * (uh.abs() @ wh.abs().transpose(1, 2) + bh.abs())
    lay = lambda t: t.permute(1, 0, 2).reshape(M, HEADS * 64)
    return lay(ref), lay(round_bound(ref, ek, dtype))


# ---- statistics-fed P . enc -------------------------------------------------------------------------------------------------------------
ST_KV = (176, 300, 1000)
ST_KINDS = ("diffuse", "peaked")
ST_B, ST_R = 2, HEADS * Q
ST_MUTANTS = ("factor_from_wrong_tile", "stale_ring_slot")


def st_ntiles(kv):
    return (kv + 175) // 176


@functools.lru_cache(maxsize=None)
def st_inputs(kv: int, kind: str, dt: str):
    """Q' [B][R][E] and enc [B][kv][E] in the operand type"""
    dtype = DTYPES[dt]
    g = _gen(94, kv, ST_KINDS.index(kind))
    qp = torch.randn(ST_B, ST_R, E, generator=g) * 0.3
    enc = torch.randn(ST_B, kv, E, generator=g) * 0.3
    if kind == "peaked":
        qp = qp + 0.5
        enc[:, kv - 10] = 0.5   # in the LAST tile: a stale slot or a neighbour's maximum there is visible
    return qp.to(dtype), enc.to(dtype)


def emulate_scores(qp, enc, kv, dtype):
    """EPI_SOFTPART in fp32: P~ [B][R][kvp] (NaN where the launch writes nothing), stat_m, stat_l [B][R][ntiles]"""
    nt, kvp = st_ntiles(kv), fold_kvp(kv)
    acc = qp.float() @ enc.float().transpose(1, 2)
    pt = torch.full((ST_B, ST_R, kvp), float("nan"), dtype=dtype)
    sm, sl = torch.zeros(ST_B, ST_R, nt), torch.zeros(ST_B, ST_R, nt)
    al = torch.tensor(ALPHA, dtype=F32)
    for t in range(nt):
        a = acc[:, :, t * 176:min((t + 1) * 176, kv)]
        sm[:, :, t] = a.amax(-1) * al
        e = torch.exp2(a * al - sm[:, :, t:t + 1]).to(dtype)
        pt[:, :, t * 176:(t + 1) * 176] = 0
        pt[:, :, t * 176:t * 176 + a.shape[-1]] = e
        sl[:, :, t] = e.float().sum(-1)
    return pt, sm, sl


def _tile_of(kvp, nt):
    return (torch.arange(kvp) // 176).clamp(max=nt - 1)


def _enc_rows(enc, kvp):
    """[B][kvp][E]: rows from kv on repeat the last token (the K-major operand of the launch)"""
    return enc[:, torch.arange(kvp).clamp(max=enc.shape[1] - 1)]


def emulate_penc(pt, sm, sl, enc, dtype, mutant=None):
    """The statistics-fed launch in fp32: factors, the scaled fragments, the product."""
    nt, kvp = sm.shape[-1], pt.shape[-1]
    mr = sm.amax(-1, keepdim=True)
    inv = 1.0 / (torch.exp2(sm - mr) * sl).sum(-1, keepdim=True)
    src = sm
    if mutant == "factor_from_wrong_tile":
        src = sm[:, :, (torch.arange(nt) + 1).clamp(max=nt - 1)]
    g = torch.exp2(src - mr) * inv
    if mutant == "stale_ring_slot":
        t = torch.arange(nt)
        g = g[:, :, torch.where(t >= 4, t - 4, t)]
    gk = g[:, :, _tile_of(kvp, nt)]
    a = torch.nan_to_num(pt.float(), nan=0.0)
    a[:, :, nt * 176:] = 0
    ap = (a.to(dtype) * gk.to(dtype)).float() if dtype == torch.float16 else (a * gk).to(dtype).float()
    return (ap @ _enc_rows(enc, kvp).float()).to(dtype)


def penc_reference(pt, sm, sl, enc, dtype):
    """(ref, bound) float64 [B][R][E] for the P~ and statistics handed to the launch"""
    nt, kvp = sm.shape[-1], pt.shape[-1]
    g, gb, _ = factor_ref(sm.reshape(-1, nt), sl.reshape(-1, nt))
    tk = _tile_of(kvp, nt)
    gd, gbd = g.view(ST_B, ST_R, nt)[:, :, tk], gb.view(ST_B, ST_R, nt)[:, :, tk]
    Ad = torch.nan_to_num(pt.double(), nan=0.0)
    Ad[:, :, nt * 176:] = 0
    Wd = _enc_rows(enc, kvp).double()
    ag, u = Ad * gd, U[dtype]
    term = Ad.abs() * (u * gd + sub_abs(dtype)) + u * ag.abs() + sub_abs(dtype) if dtype == torch.float16 else (u + U32) * ag.abs()
    term = term + Ad.abs() * gbd
    term = torch.where(Ad == 0, torch.zeros_like(term), term)
    ref = ag @ Wd
    e32 = term @ Wd.abs() + (kvp + 1) * U32 * ((ag.abs() + term) @ Wd.abs())
    return ref, round_bound(ref, e32, dtype)
