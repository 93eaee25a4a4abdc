"""Shared by tests/test_lm_head_cases_cpu.py and tests/test_gpu_lm_head.py (not a test module): the case table, seeded inputs rounded to the
operand type, float64 references, DERIVED per-element bounds and the fp32 emulation (with named mutants) of the kernels of csrc/lm_head.hip
behind ``mra_lm_head_ce_forward`` / ``mra_lm_head_ce_backward``.  Pure torch on the CPU.  Conventions as tests/lora_cases.py: u32 = 2^-24,
u = U[T] (2^-11 f16, 2^-8 bf16), every bound worst case and first order, nothing fitted to GPU output; a sum whose order is not fixed (the
MFMA's internal order) is bounded as a sum in ANY order at one u32 per link.  The references are float64 on the ROUNDED operands h, W.

    z = h W^T,  lse_r = log sum_v exp z_rv,  nll_r = lse_r - z_r,y_r,  p = softmax(z),  dh_r = g_r (p_r - e_y_r) W
    a label outside [0, V): nll NaN, dh_r = g_r p_r W

Geometry read off the kernels: vocabulary tiles of 64 columns (T = ceil(V / 64)), the backward's sum over V split into S ranges of
tps = ceil(T / S) whole tiles (``splits``: the formula of include/mra.h).

---- logits ------------------------------------------------------------------------------------------------------------------------------
Products of two 16-bit values are exact in fp32; K of them meet in K - 1 additions (MFMA steps of 32, ascending):
    e_z[r, v] = (K + 1) u32 sum_k |h_rk| |W_vk|

---- lse -----------------------------------------------------------------------------------------------------------------------------------
Per tile t: m_t = max of the tile's (computed) logits, exact; each term exp2((z - m_t) * log2e): the subtraction, the constant and the
product are three roundings of the argument, the hardware exp2 is good to 1 ulp (2 u32 taken):
    eta[r, v] = 3 u32 |z_rv - m_rt| + 2 u32          relative error of the term beyond e_z
The tile sum is a 64-lane butterfly (depth 6).  The merge scales s_t by exp2((m_t - M) * log2e) (3 u32 |m_t - M| + 2 u32 = zeta0, and one
product), adds ceil(T / 64) terms per lane in order and merges the lanes by a butterfly (6).  A relative error of a term of the sum moves
log S by at most its softmax share, so all of this weighs in with sum_v p_v (...):
    lse_b[r] = max_v e_z[r, v] + sum_v p_rv (eta_rv + zeta0_rt(v)) + (6 + 1 + ceil(T / 64) + 6) u32 + u32 (4 |lse - M| + |lse|)
(the last: logf to 2 ulp, twice for first order, and the rounding of M + log S).
    nll_b[r] = lse_b[r] + e_z[r, y_r] + u32 (|lse_r| + |z_r,y_r|)

---- dh ------------------------------------------------------------------------------------------------------------------------------------
dh = sum_t f_rt (sum_{v in t} P~_rv W_v) - g_r W_y with P~ = T(exp(z - m_t)) (relative u + e_z + eta; f16 adds the flush below 2^-24: an
absolute 2^-25 per element) and the fp32 factor f_rt = g_r exp2((m_t - lse) * log2e), relative lse_b + zeta_rt + u32,
zeta_rt = 3 u32 |m_rt - lse_r| + 2 u32.  No 16-bit factor is used.  A tile product is 64 exact products in any order (64 u32), one fma
per tile (tps of them), S partial sums in ascending order, one fma for the one-hot term:
    e[r, k]   = sum_v |g_r| p_rv (u + e_z[r, v] + eta_rv + lse_b[r] + zeta_rt(v) + u32) |W_vk|
              + [f16] sum_v |g_r| exp(m_rt(v) - lse_r) 2^-25 |W_vk|
              + (64 + tps + S + 3) u32 (sum_v |g_r| p_rv |W_vk| + |g_r W_y,k|)
    dh_b[r,k] = e + u (|ref| + e) + 2^-25 [f16]
Every element of every output is held to its bound.

Input families, by row (r + offset) % 8: mild; peaked at the label (one logit about 30 above the rest); shifted +80 (every logit near +80:
column 0 of W is 4 everywhere, h_r0 = +-20 or +-24); peaked at another column; shifted -80; all-equal (h_r = 0: nll = log V exactly);
shifted +96; shifted -96 (fp32 exp(+-96) overflows / flushes: a kernel without the tile maximum cannot pass, whatever the dtype).
Labels cycle through column 0, the last column of tile 0, the first of tile 1, V - 1, the first column of the ragged last tile, a random
column and a repeat of the previous row's label; with R >= 16 row 7 has label -1 and row 9 label V.  g has mixed signs and g[1] = 0.

Mutants (``emulate(..., mutant=)``):  ragged_counted (the tail columns past V enter maximum and sum as zero logits), first_tile_max (tile
maxima not merged: every tile sum is taken as relative to tile 0's maximum), lse_log2 (lse left in log2 units), label_shift (row r scored
against row r + 1's label), no_onehot, onehot_after_rounding (the one-hot, in the tile's units, is subtracted from the ROUNDED P~ and the
difference rounded again), last_split_dropped, g_row0 (g of row 0 for every row), exp_nomax (exp(z) without the maximum)."""
import functools
import math

import torch

from train_kernel_cases import F16_SUB, U, U32, _gen, ratio  # noqa: F401  (re-exported for the tests)

F32, F64 = torch.float32, torch.float64
DTYPES = (torch.float16, torch.bfloat16)
ROWS = (1, 3, 16, 17, 130)                 # one row; a short tile; exactly one MFMA row tile; one past it; past the 128-row group
VOCABS = (1, 8, 255, 256, 257, 260, 513, 1000, 2200)      # 2200: 35 tiles in 12 splits of 3, the last of 2 (more than one tile per split)
KS = (8, 64, 200, 512)                     # one vector; two MFMA steps; steps and a tail of 8, past one 128-column block; four blocks
TILE, GROUP, KBLOCK, MAX_SPLITS = 64, 128, 128, 16
L2E = 1.4426950408889634
MUTANTS = ("ragged_counted", "first_tile_max", "lse_log2", "label_shift", "no_onehot", "onehot_after_rounding", "last_split_dropped", "g_row0",
           "exp_nomax")


def cases():
    """(R, V, K): every V with every K, the row counts dealt so that every R meets every V and every K."""
    out = []
    for vi, V in enumerate(VOCABS):
        for ki, K in enumerate(KS):
            out.append((ROWS[(vi + ki) % 5], V, K))
            out.append((ROWS[(vi + 2 * ki + 2) % 5], V, K))
    return sorted(set(out))


def tiles(V: int) -> int:
    return (V + TILE - 1) // TILE


def splits(R: int, V: int, K: int) -> int:
    """include/mra.h: S = ceil(T / ceil(T / min(16, max(1, 512 / (ceil(K / 128) * ceil(R / 128))))))."""
    wgs = ((K + KBLOCK - 1) // KBLOCK) * ((R + GROUP - 1) // GROUP)
    smax = min(MAX_SPLITS, max(1, 512 // wgs)) if wgs else 1
    nt = tiles(V)
    tps = (nt + smax - 1) // smax
    return (nt + tps - 1) // tps


def up256(n: int) -> int:
    return (n + 255) // 256 * 256


def workspace_bytes(R: int, V: int, K: int, want_grad: bool) -> int:
    nt = tiles(V)
    n = 2 * up256(4 * R * nt) + up256(4 * R)
    if want_grad:
        n += up256(2 * R * TILE * nt) + up256(4 * splits(R, V, K) * R * K)
    return n


def pitches(R: int, V: int, K: int):
    """(ldh, ldw, lddh): most cases are pitched views."""
    return K + (8 if (R + V) % 2 else 0), K + (16 if (V + K // 8) % 3 else 0), K + (8 if (R + K // 8) % 2 == 0 else 24)


@functools.lru_cache(maxsize=None)
def make_case(R: int, V: int, K: int, dtype):
    """h [R, K], W [V, K] in ``dtype``; labels int32 [R]; g fp32 [R]."""
    gen = _gen(R, V, K, 31)
    W = torch.randn(V, K, generator=gen) * 0.5
    W[:, 0] = 4.0
    W = W.to(dtype)
    h = torch.randn(R, K, generator=gen) * (3.0 / math.sqrt(K))
    nt = tiles(V)
    special = [0, min(TILE - 1, V - 1), min(TILE, V - 1), V - 1, min((nt - 1) * TILE, V - 1)]
    labels = torch.zeros(R, dtype=torch.int64)
    other = torch.randint(0, V, (R,), generator=gen)
    rnd = torch.randint(0, V, (R,), generator=gen)
    off = (V + K // 8) % 8
    Wd = W.double()
    for r in range(R):
        c = (r + off // 2) % 7
        labels[r] = special[c] if c < 5 else (rnd[r] if c == 5 or r == 0 else labels[r - 1])
    for r in range(R):
        fam = (r + off) % 8
        if fam in (1, 3):
            col = int(labels[r]) if fam == 1 else int(other[r])
            d = Wd[col].clone()
            d[0] = 0.0                                   # the shared column would lift every logit alike
            h[r] += 30.0 * (d / (d * d).sum()).float()
        elif fam in (2, 4, 6, 7):
            h[r, 0] = {2: 20.0, 4: -20.0, 6: 24.0, 7: -24.0}[fam]
        elif fam == 5:
            h[r] = 0.0
    if R >= 16:
        labels[7], labels[9] = -1, V
    g = torch.randn(R, generator=gen)
    g[::3] = -g[::3].abs() - 0.1
    g[2::3] = g[2::3].abs() + 0.1
    if R > 1:
        g[1] = 0.0
    return dict(h=h.to(dtype), W=W, labels=labels.to(torch.int32), g=g.to(F32), family=[(r + off) % 8 for r in range(R)])


def _tile_of(V: int):
    return torch.arange(V) // TILE


@functools.lru_cache(maxsize=None)
def reference(R: int, V: int, K: int, dtype):
    """float64 values and the bounds of the module docstring: dict(z, lse, nll, dh, lse_b, nll_b, dh_b, valid)."""
    c = make_case(R, V, K, dtype)
    h, W, y, g = c["h"].double(), c["W"].double(), c["labels"].long(), c["g"].double()
    u = U[dtype]
    nt, S = tiles(V), splits(R, V, K)
    tps = (nt + S - 1) // S
    z = h @ W.t()
    e_z = (K + 1) * U32 * (h.abs() @ W.abs().t())
    lse = torch.logsumexp(z, dim=1)
    p = torch.exp(z - lse[:, None])
    tile = _tile_of(V)
    m_t = torch.stack([z[:, tile == t].max(1).values for t in range(nt)], 1)            # [R, nt]
    m_v = m_t[:, tile]                                                                    # [R, V]
    M = m_t.max(1).values
    eta = 3 * U32 * (z - m_v).abs() + 2 * U32
    zeta0 = 3 * U32 * (m_v - M[:, None]).abs() + 2 * U32
    lse_b = (e_z.max(1).values + (p * (eta + zeta0)).sum(1) + (13 + (nt + 63) // 64) * U32 + U32 * (4 * (lse - M).abs() + lse.abs()))
    valid = (y >= 0) & (y < V)
    yc = y.clamp(0, V - 1)
    zy = z.gather(1, yc[:, None]).squeeze(1)
    nll = torch.where(valid, lse - zy, torch.full_like(lse, float("nan")))
    nll_b = lse_b + e_z.gather(1, yc[:, None]).squeeze(1) + U32 * (lse.abs() + zy.abs())
    Wy = W[yc] * valid[:, None].double()
    dh = g[:, None] * (p @ W - Wy)
    zeta = 3 * U32 * (m_v - lse[:, None]).abs() + 2 * U32
    ga = g.abs()[:, None]
    rel = u + e_z + eta + lse_b[:, None] + zeta + U32
    e = (ga * p * rel) @ W.abs() + (64 + tps + S + 3) * U32 * ((ga * p) @ W.abs() + ga * Wy.abs())
    if dtype == torch.float16:
        e = e + (ga * torch.exp(m_v - lse[:, None]) * F16_SUB) @ W.abs()
    dh_b = e + u * (dh.abs() + e) + (F16_SUB if dtype == torch.float16 else 0.0)
    return dict(z=z, lse=lse, nll=nll, dh=dh, lse_b=lse_b, nll_b=nll_b, dh_b=dh_b, valid=valid)


def _exp2(x):
    return torch.exp2(x.to(F32))


def emulate(R: int, V: int, K: int, dtype, mutant=None):
    """The kernels in fp32 torch ops, tile by tile and split by split: (nll, lse, dh [R, K] in ``dtype``)."""
    c = make_case(R, V, K, dtype)
    hf, Wf, y, g = c["h"].float(), c["W"].float(), c["labels"].long(), c["g"].clone()
    if mutant == "label_shift":
        y = torch.roll(y, -1)
    if mutant == "g_row0":
        g = g[0].expand(R).clone()
    nt, S = tiles(V), splits(R, V, K)
    tps = (nt + S - 1) // S
    z = hf @ Wf.t()
    l2e = torch.tensor(L2E, dtype=F32)
    tmax, tsum = torch.empty(R, nt, dtype=F32), torch.empty(R, nt, dtype=F32)
    P = torch.zeros(R, nt * TILE, dtype=dtype)
    for t in range(nt):
        v0, v1 = t * TILE, min(V, t * TILE + TILE)
        zt = z[:, v0:v1]
        if mutant == "ragged_counted" and v1 - v0 < TILE:
            zt = torch.cat([zt, torch.zeros(R, TILE - (v1 - v0), dtype=F32)], 1)
        m = torch.zeros(R, dtype=F32) if mutant == "exp_nomax" else zt.max(1).values
        e = _exp2((zt - m[:, None]) * l2e)
        tmax[:, t], tsum[:, t] = m, e.sum(1)
        P[:, v0:v1] = e[:, :v1 - v0].to(dtype)
    if mutant == "first_tile_max":
        M, Ssum = tmax[:, 0], tsum.sum(1)
    else:
        M = tmax.max(1).values
        Ssum = (tsum * _exp2((tmax - M[:, None]) * l2e)).sum(1)
    lse = M + (torch.log2(Ssum) if mutant == "lse_log2" else torch.log(Ssum))
    valid = (y >= 0) & (y < V)
    yc = y.clamp(0, V - 1)
    nll = torch.where(valid, lse - z.gather(1, yc[:, None]).squeeze(1), torch.full_like(lse, float("nan")))
    f = g[:, None] * _exp2((tmax - lse[:, None]) * l2e)                                    # [R, nt]
    if mutant == "onehot_after_rounding":
        for r in range(R):
            if valid[r]:
                t = int(yc[r]) // TILE
                one = _exp2((lse[r] - tmax[r, t]) * l2e).to(dtype)
                P[r, yc[r]] = (P[r, yc[r]].float() - one.float()).to(dtype)
    acc = torch.zeros(R, K, dtype=F32)
    for s in range(S - 1 if mutant == "last_split_dropped" else S):
        part = torch.zeros(R, K, dtype=F32)
        for t in range(s * tps, min(nt, s * tps + tps)):
            v0, v1 = t * TILE, min(V, t * TILE + TILE)
            part = part + f[:, t:t + 1] * (P[:, v0:v1].float() @ Wf[v0:v1])
        acc = acc + part
    if mutant not in ("no_onehot", "onehot_after_rounding"):
        acc = acc - g[:, None] * Wf[yc] * valid[:, None].float()
    return nll, lse, acc.to(dtype)


def ratios(R: int, V: int, K: int, dtype, nll, lse, dh):
    """(nll, lse, dh) worst |d| / bound; inf where a NaN row's nll is not NaN, or a valid row's is."""
    ref = reference(R, V, K, dtype)
    v = ref["valid"]
    nll = nll.double().cpu()
    if not torch.isnan(nll[~v]).all():
        r_nll = float("inf")
    else:
        r_nll = ratio(nll[v], ref["nll"][v], ref["nll_b"][v])
    return r_nll, ratio(lse.cpu(), ref["lse"], ref["lse_b"]), ratio(dh.cpu(), ref["dh"], ref["dh_b"])
