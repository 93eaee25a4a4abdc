"""Shared by tests/test_gemm_cases_cpu.py and tests/test_gpu_gemm_forward.py (not a test module): the launch forms of csrc/gemm.hip that the
Q-Former forward, the K/V projection and mra_llm_proj issue (csrc/mra_abi.hip), as a CASE TABLE (CASES) with seeded inputs rounded to the
operand type, float64 references, DERIVED per-element bounds, and an fp32 emulation of every form with named mutants.  Pure torch on the CPU.

Both tests see a launch the same way: flat input buffers (NaN wherever no view addresses them), flat output buffers that start as all-ones
bits, and ``check`` -- which holds every output element to its bound, wants every owned element rewritten and every other one still all-ones.
The CPU test feeds ``check`` the emulation's buffers, the GPU test those of mra_debug_gemm.

Notation as tests/qformer_kernel_cases.py and tests/train_kernel_cases.py: u32 = 2^-24, u = U[T], every bound worst case and first order, no
constant fitted to GPU output.  Like those files this one ASSUMES an MFMA is no worse than a chain of fp32 additions of its exact products
(a product of two f16 / bf16 values is exact in fp32).

---- accumulator ------------------------------------------------------------------------------------------------------------------------------
acc + bias: K products and the bias meet in K links of any order -- the two-buffer loops add K tile after K tile, the ring kernel adds its even
and its odd K tiles in two wave groups and then the halves:
    eK = (K + 1) u32 (|A| |W|^T + |bias|)
EPI_F32       C = acc + bias in fp32:                  |C - ref| <= eK
EPI_RES_F32   one more link and one more term:         |C - ref| <= (K + 2) u32 (|A| |W|^T + |bias| + |R|)
EPI_OP        C = T(acc + bias):                       round_bound(ref, eK, T) = eK + u (|ref| + eK) + 2^-25 [f16]
EPI_KV        the same value at the head-major index ((((n / hidden) items + item) heads + head) tokens + tok) 64 + d
EPI_GELU_OP   gelu_erf (csrc/mra_common.h) IS 0.5 x (1 + erf_fast(x fl(2^-1/2))), the function train_kernel_cases derives E_ERF and eg for.  The
              pre-activation's error passes through |gelu'| <= 1.13:
              e32 = 1.13 eK + eg(pre),  eg(u) = |u| E_ERF / 2 + 3 u32 |gelu(u)|;   |C - gelu(pre)| <= round_bound(gelu(pre), e32, T)
n_ragged      columns N .. ceil(N / tile) tile - 1 of an EPI_F32 launch are written with unspecified values: owned, not compared.

---- EPI_RES_LN -------------------------------------------------------------------------------------------------------------------------------
C is EPI_RES_F32's.  The workgroup that finishes a 64-row block last reads the block's C rows back (sc1 loads) and normalises them: two passes,
the mean and the variance by a division by H.  ln_y32 is held to the LayerNorm-family bound of qformer_kernel_cases.ln_ref against the float64
LayerNorm OF THE C ROWS THE LAUNCH RETURNED (a row read before its last column tile was visible still holds sentinel NaN there: the output is
NaN); ln_y16 is ln_y32 rounded once, bit for bit; every counter is zero afterwards, and a second launch on the same counters gives the same.

---- EPI_SOFTPART (scores of the folded cross-attention) --------------------------------------------------------------------------------------
s = A W^T without a bias, eK = (K + 1) u32 |A| |W|^T.  Per row and 176-column tile, each stage against the kernel's own previous stage:
    stat_m = fl(alpha max_n acc)            |stat_m - alpha max_n s| <= alpha max_n eK + u32 |stat_m|        (max is monotone; one product)
    P~ = T(exp2(fma(acc, alpha, -stat_m)))  y = alpha s - stat_m (the stat_m RETURNED); the exponent errs by d = alpha eK + u32 |y| (the fma
                                            rounds once), the instruction by 2 u32:
                                            |P~ - 2^y| <= round_bound(2^y, 2^y (ln2 d + 2 u32) + 2^-126, T)    (v_exp_f32 returns no subnormals)
    stat_l = sum of the tile's P~ AS STORED |stat_l - sum| <= 176 u32 sum          (176 values in any order)
    columns N .. end of the last tile of P~ are exact zeros (and not in stat_l); columns from ntiles 176 on are not written.
w_kwrap: K = 2 E, the weights [N][E] walked twice: s = A[:, :E] W^T + A[:, E:] W^T, the same bound with |A| (|W| |W|)^T.

---- pscale (P . enc with the split softmax's row factors applied in registers) ----------------------------------------------------------------
ref = sum_k A[m][k] g[m][tile(k)] W[k][n], tile(k) = min(k / 176, ps_ntiles - 1), W K-major; rows k >= k_rows repeat row k_rows - 1 against A = 0.
The kernel (gemm_ws_kernel, PSC) multiplies each A fragment on its way into the MFMA:
    f16:   a' = f16(a f16(g))     packed multiplies: the factor is rounded to f16 first (relative u, or 2^-25 absolute once g < 2^-14 -- factors
                                   reach 1e-6), then the product once: |a' - a g| <= |a| (u g + 2^-25) + u |a g| + 2^-25
    bf16:  a' = bf16(float(a) g)  in fp32, rounded once:  |a' - a g| <= (u + u32) |a g|                (bf16 has the range of fp32)
    e32 = sum_k |a' - a g| |W| + (K + 1) u32 sum_k (|a g| + |a' - a g|) |W|;    |C - ref| <= round_bound(ref, e32, T)
Without pscale the same launch is EPI_OP over the K-major weights."""
import ctypes as C
import functools
import math

import torch

from qformer_kernel_cases import LOG2E, U, U32, depth, factor_ref, ln_emulate, ln_ref, round_bound, sub_abs  # noqa: F401  (re-exported)
from train_kernel_cases import E_ERF, gelu64, gelu_emulate, ratio  # noqa: F401

F32 = torch.float32
F64 = torch.float64
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}

# csrc/kernels.h (the numbers mraudio_amd/_lib.py repeats; kept here so that this file imports without the built library)
EPI_OP, EPI_GELU_OP, EPI_RES_F32, EPI_F32, EPI_KV, EPI_SOFTPART, EPI_RES_LN = 0, 1, 2, 3, 4, 5, 9
EPI_NAME = {0: "OP", 1: "GELU_OP", 2: "RES_F32", 3: "F32", 4: "KV", 5: "SOFTPART", 9: "RES_LN"}
GT_AUTO, GT_64, GT_128, GT_256, GT_WS_128x384, GT_WS_176x384, GT_K128_64x128 = 0, 1, 2, 3, 4, 5, 6
GT_RING_144x128, GT_RING_192x128, GT_RING_96x64 = 9, 10, 11
GF_V1_64, GF_V1_128, GF_WS_256, GF_P8_256, GF_WS_128x384, GF_WS_176x384, GF_K128_64x128, GF_K128_64x64 = 0, 1, 3, 4, 5, 6, 7, 10
GF_RING_144x128, GF_RING_192x128, GF_RING_96x64 = 11, 12, 13
TILE_N = {GF_V1_64: 64, GF_V1_128: 128, GF_WS_256: 256, GF_P8_256: 256, GF_WS_128x384: 128, GF_WS_176x384: 176, GF_K128_64x128: 64,
          GF_K128_64x64: 64, GF_RING_144x128: 144, GF_RING_192x128: 192, GF_RING_96x64: 96}
K_STEP = {GF_K128_64x128: 128, GF_K128_64x64: 128, GF_P8_256: 128}       # K elements one main-loop step consumes (64 elsewhere)
RING = (GF_RING_144x128, GF_RING_192x128, GF_RING_96x64)
ALPHA = float(torch.tensor(0.125, dtype=F32) * torch.tensor(1.4426950408889634, dtype=F32))   # the forward's scale, log2 units
LN_EPS = 1e-12
CUS = 256           # compute units of the device the persistent case is planned for
C_PAD, C_TAIL = 8, 3    # columns between the row length and the row stride of an output, whole rows behind it: all keep the sentinel

# Every (family, epilogue) pair the forwards reach, with its call site in csrc/mra_abi.hip.  The CPU test holds CASES against this list.
PAIRS = {
    (GF_V1_64, EPI_OP): "layer chain at few rows: qkv gemm, cross q gemm; fold q' gemm / fold context gemm (GT_64); mra_llm_proj; kv_project at few tiles",
    (GF_V1_64, EPI_GELU_OP): "ffn up gemm at few rows",
    (GF_V1_64, EPI_RES_F32): "attn out / cross out / ffn down gemm at few rows (K < 2048)",
    (GF_V1_64, EPI_F32): "cross q gemm and fold q' gemm in split precision; mra_llm_proj with fp32 output",
    (GF_K128_64x64, EPI_RES_F32): "ffn down gemm at few rows (K = inter >= 2048)",
    (GF_V1_128, EPI_OP): "qkv gemm at >= 1024 rows with the ring off; fold q' gemm (GT_128); fold p.enc gemm against encT",
    (GF_V1_128, EPI_F32): "fold q' gemm in split precision (GT_128); fold scores gemm when heads * queries != 384 (n_ragged, batched)",
    (GF_K128_64x128, EPI_RES_F32): "ffn down gemm at >= 512 rows with the ring off",
    (GF_K128_64x128, EPI_OP): "fold context gemm at >= 512 rows",
    (GF_RING_144x128, EPI_OP): "qkv gemm, ring",
    (GF_RING_192x128, EPI_GELU_OP): "ffn up gemm, ring",
    (GF_RING_192x128, EPI_OP): "the same tile without the activation (EpiRing16)",
    (GF_RING_96x64, EPI_RES_F32): "attn out / cross out / ffn down gemm, ring, LayerNorm in a launch of its own",
    (GF_RING_96x64, EPI_F32): "EpiRing96",
    (GF_RING_96x64, EPI_OP): "EpiRing96",
    (GF_RING_96x64, EPI_GELU_OP): "EpiRing96",
    (GF_RING_96x64, EPI_RES_LN): "attn out gemm + ln, cross out gemm + ln, ffn down gemm + ln",
    (GF_WS_176x384, EPI_SOFTPART): "fold scores gemm (softmax partials)",
    (GF_WS_176x384, EPI_OP): "fold p.enc gemm, K-major encoder tokens, with and without pscale",
    (GF_WS_128x384, EPI_OP): "fold p.enc gemm against encT (audio width)",
    (GF_V1_64, EPI_KV): "kv_project at few tiles",
    (GF_V1_128, EPI_KV): "kv_project, GT_128",
    (GF_P8_256, EPI_KV): "kv_project: one workgroup per tile, and persistent",
    (GF_WS_256, EPI_KV): "kv_project with an odd number of K steps",
}

ROW_MUTANTS = {
    1: ("last_k_step_dropped", "bias_of_problem_0", "rows_past_M_stored", "residual_through_c_view"),
    2: ("last_k_step_dropped",),
    3: ("bias_of_problem_0",),
    4: ("rows_past_M_stored", "last_k_step_dropped"),
    5: ("odd_k_tiles_dropped",),
    6: ("odd_k_tiles_dropped", "bias_of_problem_0"),
    7: ("odd_k_tiles_dropped", "residual_through_c_view"),
    8: ("ln_before_last_tile", "counter_left_set"),
    9: ("a_batch_stride_ignored",),
    10: ("kwrap_single_pass", "ragged_tail_in_sum", "tile_sum_unrounded"),
    11: ("w_batch_stride_ignored",),
    12: ("pscale_tile_unclamped", "w_batch_stride_ignored"),
    13: ("w_batch_stride_ignored",),
    14: ("bias_stride_ignored",),
    15: ("kv_head_swapped",),
}


def fold_kvp(kv: int) -> int:
    """csrc/mra_handle.h fold_kvp: the row stride of the folded cross-attention's score / P rows."""
    return (max((kv + 127) // 128 * 128, (kv + 175) // 176 * 176) + 127) // 128 * 128


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


# =========================================================================================================================================
# layouts: where a logical [batch, rows, cols] operand lives in a flat buffer
# =========================================================================================================================================
def lay(view, numel, off=0, bs=0):
    """view = (item_stride, rows per item, row stride) in elements from element ``off`` on; batch entry b starts ``bs`` elements later."""
    return dict(view=tuple(int(v) for v in view), numel=int(numel), off=int(off), bs=int(bs))


def plain_lay(rows, cols, pad=0, tail=0, batch=1):
    """Dense rows of stride cols + pad, ``tail`` rows behind them, batch entries one after the other (mra_handle.h plain())."""
    ld = cols + pad
    per = (rows + tail) * ld
    return lay((0, max(rows, 1), ld), per * batch, 0, per)


def item_lay(rows, cols, pad=C_PAD):
    """Rows [3, 8) of 9-row items with row stride cols + pad (tests/native/kernel_check's views)."""
    ld = cols + pad
    return lay((9 * ld, 5, ld), (rows + 4) // 5 * 9 * ld, 3 * ld)


def cls_lay(rows, cols, pad=C_PAD, S=6):
    """One row per item of S rows (the forward's cls_view): row 1 of every item."""
    ld = cols + pad
    return lay((S * ld, 1, ld), rows * S * ld, ld)


def index(l, rows, cols, batch=1):
    """Flat element indices [batch, rows, cols] of a layout."""
    m = torch.arange(rows)
    s, rpi, ld = l["view"]
    row = (m // rpi) * s + (m % rpi) * ld
    return l["off"] + (torch.arange(batch) * l["bs"])[:, None, None] + row[None, :, None] + torch.arange(cols)[None, None, :]


def _bits_dtype(dtype):
    return {2: torch.int16, 4: torch.int32}[torch.empty(0, dtype=dtype).element_size()]


def sentinel(numel, dtype):
    """All-ones bits: NaN in f32, f16 and bf16, 0xFFFFFFFF as a counter."""
    return torch.full((numel,), -1, dtype=_bits_dtype(dtype)).view(dtype)


def is_sentinel(t):
    return t.view(_bits_dtype(t.dtype)) == -1


def place(mat, l, dtype, fill=None):
    """``mat`` [batch, rows, cols] laid out in a flat NaN tensor (or into ``fill``)."""
    flat = torch.full((l["numel"],), float("nan"), dtype=dtype) if fill is None else fill
    flat[index(l, mat.shape[1], mat.shape[2], mat.shape[0]).reshape(-1)] = mat.reshape(-1).to(dtype)
    return flat


# =========================================================================================================================================
# the case table
# =========================================================================================================================================
def prob(M, N, K, a=None, c=None, r=None, batch=1, **kw):
    """One problem.  a / c / r: layouts (default: dense A, C with C_PAD columns and C_TAIL rows to spare, dense R).  Further keys: bias
    (default True), n_ragged, w_kwrap, kmajor (k_rows), pscale (ps_ntiles), kv = (tokens, items, heads), ln = "both" / "y32" / "y16",
    bias_bs, w_bs (0 = shared)."""
    p = dict(M=M, N=N, K=K, batch=batch, bias=True, n_ragged=0, w_kwrap=0, k_rows=0, ps_ntiles=0, kv=None, ln=None, scores=None)
    p.update(kw)
    p["a"] = a or plain_lay(M, K, batch=batch)
    p["c"] = c
    p["r"] = r
    return p


CASES = []


def case(row, name, epi, tile, family, probs, persist=0, heavy=False):
    assert all(c["name"] != name for c in CASES), name
    CASES.append(dict(row=row, name=name, epi=epi, tile=tile, family=family, probs=probs, persist=persist, heavy=heavy))


def _out_cols(c, p):
    tn = TILE_N[c["family"]]
    return (p["N"] + tn - 1) // tn * tn if (p["n_ragged"] or c["epi"] == EPI_SOFTPART) else p["N"]


def _finish(c):
    """Default output / residual layouts, once the family (the tile that n_ragged rounds up to) is known."""
    for p in c["probs"]:
        if c["epi"] == EPI_KV:
            tok, items, heads = p["kv"]
            p["c"] = lay((0, 1, 1), p["N"] // (heads * 64) * items * heads * tok * 64)
            continue
        if p["c"] is None:
            p["c"] = plain_lay(p["M"], _out_cols(c, p), C_PAD, C_TAIL, p["batch"])
        if c["epi"] in (EPI_RES_F32, EPI_RES_LN) and p["r"] is None:
            p["r"] = plain_lay(p["M"], p["N"])
        if c["epi"] == EPI_RES_LN:
            p["y32"] = item_lay(p["M"], p["N"]) if p["ln"] in ("both", "y32") else None
            p["y16"] = cls_lay(p["M"], p["N"]) if p["ln"] == "y16" else (plain_lay(p["M"], p["N"], C_PAD, C_TAIL) if p["ln"] == "both" else None)


def _group(Ms, N, K, last_cls=True):
    """The grouped launches of the layer chain: problem i has Ms[i] rows; odd problems read A through item views (the text rows of the
    forward), a last problem of at most 3 rows through a one-row-per-item view (cls_view); outputs likewise."""
    ps = []
    for i, M in enumerate(Ms):
        if last_cls and i == len(Ms) - 1 and M <= 3 and len(Ms) > 1:
            ps.append(prob(M, N, K, a=cls_lay(M, K), c=cls_lay(M, N)))
        elif i % 2:
            ps.append(prob(M, N, K, a=item_lay(M, K), c=item_lay(M, N)))
        else:
            ps.append(prob(M, N, K))
    return ps


def _build_table():
    E = EPI_NAME
    # 1. layer chain at few rows, mra_llm_proj: GT_AUTO -> GF_V1_64
    for epi in (EPI_OP, EPI_GELU_OP, EPI_RES_F32, EPI_F32):
        for M, K, views in ((1, 64, False), (70, 192, True), (133, 768, False), (70, 768, True), (133, 64, True), (1, 192, False)):
            p = prob(M, 128, K, a=item_lay(M, K), c=item_lay(M, 128)) if views else prob(M, 128, K)
            case(1, f"v1_64 {E[epi]} M{M} K{K}" + (" views" if views else ""), epi, GT_AUTO, GF_V1_64, [p])
        case(1, f"v1_64 {E[epi]} groups 64/27 K192", epi, GT_AUTO, GF_V1_64, _group((64, 27), 128, 192))
        case(1, f"v1_64 {E[epi]} groups 64/27/70/3 K768", epi, GT_AUTO, GF_V1_64, _group((64, 27, 70, 3), 128, 768))
    # 2. FFN down at few rows: GT_AUTO -> GF_K128_64x64 (every K >= 2048, K % 128 == 0)
    case(2, "k128_64x64 RES_F32 M70 K2048", EPI_RES_F32, GT_AUTO, GF_K128_64x64, [prob(70, 128, 2048, c=item_lay(70, 128))])
    case(2, "k128_64x64 RES_F32 groups 70/27 K3072", EPI_RES_F32, GT_AUTO, GF_K128_64x64, _group((70, 27), 128, 3072))
    case(2, "k128_64x64 RES_F32 groups 70/3 K2048", EPI_RES_F32, GT_AUTO, GF_K128_64x64, _group((70, 3), 128, 2048))
    # 3. QKV at >= 1024 rows, ring off: GT_128 -> GF_V1_128
    case(3, "v1_128 OP M133 K64", EPI_OP, GT_128, GF_V1_128, [prob(133, 256, 64)])
    case(3, "v1_128 OP M293 K192 views", EPI_OP, GT_128, GF_V1_128, [prob(293, 256, 192, a=item_lay(293, 192), c=item_lay(293, 256))])
    case(3, "v1_128 OP groups 293/133 K192", EPI_OP, GT_128, GF_V1_128, _group((293, 133), 256, 192))
    case(3, "v1_128 OP groups 133/293 K64", EPI_OP, GT_128, GF_V1_128, _group((133, 293), 256, 64))
    # 4. FFN down at >= 512 rows, ring off: GT_K128_64x128
    for epi in (EPI_RES_F32, EPI_OP):
        for M, K in ((5, 128), (133, 384), (256, 3072), (133, 128), (256, 384)):
            case(4, f"k128_64x128 {E[epi]} M{M} K{K}", epi, GT_K128_64x128, GF_K128_64x128, [prob(M, 128, K, c=item_lay(M, 128) if M == 133 else None)])
        case(4, f"k128_64x128 {E[epi]} groups 133/5 K384", epi, GT_K128_64x128, GF_K128_64x128, _group((133, 5), 128, 384))
        case(4, f"k128_64x128 {E[epi]} groups 133/5/256/70 K128", epi, GT_K128_64x128, GF_K128_64x128, _group((133, 5, 256, 70), 128, 128))
    # 5. QKV, ring 144 x 128 (4 stages): fewer than, exactly and more than 4 K steps, odd and even step counts
    ring_k = (64, 192, 256, 320, 768)
    for i, K in enumerate(ring_k):
        case(5, f"ring144 OP M37 N144 K{K}", EPI_OP, GT_RING_144x128, GF_RING_144x128, [prob(37, 144, K, c=item_lay(37, 144) if i % 2 else None)])
        case(5, f"ring144 OP M293 N288 K{K}", EPI_OP, GT_RING_144x128, GF_RING_144x128, [prob(293, 288, K, a=item_lay(293, K) if i % 2 else None)])
    for K in (64, 320, 768):
        case(5, f"ring144 OP groups 293/37 N288 K{K}", EPI_OP, GT_RING_144x128, GF_RING_144x128, _group((293, 37), 288, K))
    # 6. FFN up, ring 192 x 128: groups of 2 and 4 with unequal M
    for epi in (EPI_GELU_OP, EPI_OP):
        for K in ring_k:
            case(6, f"ring192 {E[epi]} groups 293/100 N192 K{K}", epi, GT_RING_192x128, GF_RING_192x128, _group((293, 100), 192, K))
            case(6, f"ring192 {E[epi]} groups 293/100/33/4 N384 K{K}", epi, GT_RING_192x128, GF_RING_192x128, _group((293, 100, 33, 4), 384, K, last_cls=False))
    # 7. residual projections, ring 96 x 64 (7 stages)
    for epi in (EPI_RES_F32, EPI_F32, EPI_OP, EPI_GELU_OP):
        for i, K in enumerate((64, 448, 512, 3072)):
            case(7, f"ring96 {E[epi]} M11 N96 K{K}", epi, GT_RING_96x64, GF_RING_96x64, [prob(11, 96, K, c=item_lay(11, 96) if i % 2 else None)])
            case(7, f"ring96 {E[epi]} M203 N192 K{K}", epi, GT_RING_96x64, GF_RING_96x64, [prob(203, 192, K, a=item_lay(203, K) if i % 2 == 0 else None)])
        case(7, f"ring96 {E[epi]} groups 203/11 N192 K448", epi, GT_RING_96x64, GF_RING_96x64, _group((203, 11), 192, 448))
        case(7, f"ring96 {E[epi]} groups 203/11/70/3 N96 K512", epi, GT_RING_96x64, GF_RING_96x64, _group((203, 11, 70, 3), 96, 512))
    # 8. the same with the LayerNorm inside: N = 768; outputs through views with gaps; each launch runs twice on its counters
    for M, K, ln in ((70, 64, "both"), (203, 448, "y32"), (203, 3072, "y16"), (2048, 768, "both"), (70, 768, "y16"), (203, 64, "both"), (70, 448, "y32")):
        case(8, f"ring96 RES_LN M{M} K{K} {ln}", EPI_RES_LN, GT_RING_96x64, GF_RING_96x64, [prob(M, 768, K, c=item_lay(M, 768) if M != 2048 else None, ln=ln)])
    case(8, "ring96 RES_LN groups 203/70 K448 both", EPI_RES_LN, GT_RING_96x64, GF_RING_96x64,
         [prob(203, 768, 448, ln="both"), prob(70, 768, 448, a=item_lay(70, 448), c=item_lay(70, 768), ln="both")])
    case(8, "ring96 RES_LN groups 70/203 K64 y32/y16", EPI_RES_LN, GT_RING_96x64, GF_RING_96x64,
         [prob(70, 768, 64, c=item_lay(70, 768), ln="y32"), prob(203, 768, 64, ln="y16")])
    case(8, "ring96 RES_LN groups 203/3 K768 both", EPI_RES_LN, GT_RING_96x64, GF_RING_96x64,
         [prob(203, 768, 768, ln="both"), prob(3, 768, 768, a=cls_lay(3, 768), c=cls_lay(3, 768), ln="both")])

    # 9. Q' per head: batch = heads, A the head's 64 (x 3) columns inside rows of all heads, C = items_view(R E, 32, E)
    def qprime(items, heads, Ew, K):
        M, R = items * 32, heads * 32
        return prob(M, Ew, K, a=lay((0, M, heads * K), M * heads * K, 0, K), c=lay((R * Ew, 32, Ew), items * R * Ew + C_TAIL * Ew, 0, 32 * Ew),
                    batch=heads, bias=False)
    case(9, "q' GT_64 OP M96 E192 K64", EPI_OP, GT_64, GF_V1_64, [qprime(3, 3, 192, 64)])
    case(9, "q' GT_64 F32 M96 E192 K192", EPI_F32, GT_64, GF_V1_64, [qprime(3, 3, 192, 192)])
    case(9, "q' GT_128 OP M256 E256 K64", EPI_OP, GT_128, GF_V1_128, [qprime(8, 3, 256, 64)])
    case(9, "q' GT_128 F32 M256 E256 K192", EPI_F32, GT_128, GF_V1_128, [qprime(8, 3, 256, 192)])

    # 10. scores with the split softmax: 176 x 384 tile, row stride fold_kvp(kv), columns from ntiles * 176 on untouched
    def scores(M, kv, K, batch, kind, kwrap=0):
        kvp = fold_kvp(kv)
        return prob(M, kv, K, a=plain_lay(M, K, batch=batch), c=plain_lay(M, kvp, 0, C_TAIL, batch), batch=batch, bias=False, n_ragged=1,
                    scores=kind, w_kwrap=kwrap)
    for M, kv, K, batch, kind in ((384, 176, 64, 1, "mild"), (200, 177, 192, 2, "peaked"), (384, 530, 192, 3, "mild"), (200, 1000, 64, 2, "peaked"),
                                  (384, 1000, 192, 1, "peaked"), (200, 530, 64, 1, "mild")):
        case(10, f"scores SOFTPART M{M} kv{kv} K{K} batch{batch} {kind}", EPI_SOFTPART, GT_WS_176x384, GF_WS_176x384, [scores(M, kv, K, batch, kind)])
    case(10, "scores SOFTPART M384 kv530 K384 batch2 mild kwrap", EPI_SOFTPART, GT_WS_176x384, GF_WS_176x384, [scores(384, 530, 384, 2, "mild", kwrap=3)])
    case(10, "scores SOFTPART M200 kv177 K384 batch1 peaked kwrap", EPI_SOFTPART, GT_WS_176x384, GF_WS_176x384, [scores(200, 177, 384, 1, "peaked", kwrap=3)])
    # 11. scores when heads * queries != 384: fp32, n_ragged, batched
    case(11, "scores F32 ragged M96 N300 K192 batch3", EPI_F32, GT_128, GF_V1_128,
         [prob(96, 300, 192, c=plain_lay(96, 384, C_PAD, C_TAIL, 3), batch=3, bias=False, n_ragged=1)])

    # 12. P . enc over the K-major encoder tokens, with and without the row factors
    def penc(M, Ew, kv, batch, ps):
        kvp = fold_kvp(kv)
        return prob(M, Ew, kvp, a=plain_lay(M, kvp, batch=batch), batch=batch, bias=False, k_rows=kv, ps_ntiles=(kv + 175) // 176 if ps else 0)
    for M, Ew, kv, batch in ((384, 176, 150, 1), (200, 352, 300, 2), (384, 352, 1000, 3), (200, 176, 1000, 1), (384, 176, 300, 2)):
        for ps in (0, 1):
            case(12, f"p.enc OP M{M} E{Ew} kv{kv} batch{batch}" + (" pscale" if ps else ""), EPI_OP, GT_WS_176x384, GF_WS_176x384, [penc(M, Ew, kv, batch, ps)])
    # 13. P . enc against encT (audio width)
    case(13, "p.encT GT_128 OP M384 E256 kv300 batch2", EPI_OP, GT_128, GF_V1_128, [prob(384, 256, 384, batch=2, bias=False)])
    case(13, "p.encT GT_WS_128x384 OP M384 E256 kv300 batch3", EPI_OP, GT_WS_128x384, GF_WS_128x384, [prob(384, 256, 384, batch=3, bias=False)])

    # 14. context per head: batch = heads, N = 64, A = items_view(R E, 32, E), C the head's 64 columns of [M][heads * 64]
    def context(items, heads, Ew):
        M, R = items * 32, heads * 32
        return prob(M, 64, Ew, a=lay((R * Ew, 32, Ew), items * R * Ew, 0, 32 * Ew), c=lay((0, M, heads * 64), (M + C_TAIL) * heads * 64, 0, 64),
                    batch=heads, bias_bs=64)
    case(14, "context GT_64 OP M96 E192", EPI_OP, GT_64, GF_V1_64, [context(3, 3, 192)])
    case(14, "context GT_K128_64x128 OP M544 E256", EPI_OP, GT_K128_64x128, GF_K128_64x128, [context(17, 3, 256)])
    # 15. K/V projection (persist = 1): N = 2 cross layers x (K, V) x 2 heads x 64; tiles straddle items
    case(15, "kv GT_AUTO M70 tok7 K64", EPI_KV, GT_AUTO, GF_V1_64, [prob(70, 512, 64, kv=(7, 10, 2))], persist=1)
    case(15, "kv GT_128 M514 tok257 K192", EPI_KV, GT_128, GF_V1_128, [prob(514, 512, 192, kv=(257, 2, 2))], persist=1)
    case(15, "kv GT_256 M530 tok257 K128", EPI_KV, GT_256, GF_P8_256, [prob(530, 512, 128, kv=(257, 3, 2))], persist=1)
    case(15, "kv GT_256 M530 tok7 K192", EPI_KV, GT_256, GF_WS_256, [prob(530, 512, 192, kv=(7, 76, 2))], persist=1)
    case(15, "kv GT_AUTO persistent M4112 N9216 K128", EPI_KV, GT_AUTO, GF_P8_256, [prob(16 * 257, 9216, 128, kv=(257, 16, 12))], persist=1, heavy=True)
    for c in CASES:
        _finish(c)


_build_table()
BY_NAME = {c["name"]: c for c in CASES}


def cases_of(row):
    return [c for c in CASES if c["row"] == row]


# =========================================================================================================================================
# inputs
# =========================================================================================================================================
@functools.lru_cache(maxsize=4)
def inputs(name: str, dt: str):
    """Per problem: logical A [B, M, K], W [Bw, N, Kw] (K-major: [Bw, k_rows, N]), bias [Bb, N] / None, R [M, N] / None, g (pscale) [B, ps_ntiles,
    512] / None, ln gain / bias [N]; and ``flat``: the input buffers as the launch sees them."""
    c = BY_NAME[name]
    dtype = DTYPES[dt]
    out = []
    for i, p in enumerate(c["probs"]):
        M, N, K, B = p["M"], p["N"], p["K"], p["batch"]
        g = _gen(c["row"], i, M, N, K, B, len(name))
        d = dict()
        Kw = K // 2 if p["w_kwrap"] else K
        if p["scores"]:       # alpha s of order 1.4 (mild) or 14 (peaked: part of a row's P~ underflows in f16)
            sigma = (8.0 if p["scores"] == "mild" else 80.0) / math.sqrt(K)
            A = torch.randn(B, M, K, generator=g)
            W = torch.randn(B, N, Kw, generator=g) * sigma
        elif p["k_rows"]:     # A = P~ in [0, 1] with zeros from kv on, W = the encoder tokens, K-major
            A = torch.rand(B, M, K, generator=g) ** 4
            A[:, :, p["k_rows"]:] = 0.0
            W = torch.randn(B, p["k_rows"], N, generator=g)
        else:
            A = torch.randn(B, M, K, generator=g)
            W = torch.randn(B, N, Kw, generator=g) / math.sqrt(K)
        d["A"], d["W"] = A.to(dtype), W.to(dtype)
        d["bias"] = None
        if p["bias"]:
            bias = torch.randn(B if p.get("bias_bs") else 1, N, generator=g) * 0.5
            if c["epi"] == EPI_GELU_OP:
                bias[:, :8] = torch.linspace(-8.0, 8.0, 8)      # pre-activations reach |u| = 8 (train_kernel_cases.make_gelu)
            d["bias"] = bias
        d["R"] = torch.randn(M, N, generator=g) * 2.0 if c["epi"] in (EPI_RES_F32, EPI_RES_LN) else None
        d["g"] = None
        if p["ps_ntiles"]:    # row factors exp2(m_tile - m_row) / L of a split softmax: from 1 down to 1e-6, NaN in the rows a tile does not have
            e = torch.rand(B, p["ps_ntiles"], 512, generator=g) * 20.0
            gf = torch.exp2(-e)
            gf[:, :, M:] = float("nan")
            d["g"] = gf
        if c["epi"] == EPI_RES_LN:
            d["gain"] = 1.0 + 0.1 * torch.randn(N, generator=g)
            d["beta"] = torch.randn(N, generator=g)
        flat = dict(A=place(d["A"], p["a"], dtype))
        flat["W"] = d["W"].reshape(-1).clone()      # dense [N][K] ([N][K / 2] under w_kwrap, [k_rows][N] K-major), batch entries one after the other
        if d["bias"] is not None:
            flat["bias"] = d["bias"].reshape(-1).clone()
        if d["R"] is not None:
            flat["R"] = place(d["R"][None], p["r"], F32)
        if d["g"] is not None:
            flat["pscale"] = d["g"].reshape(-1).clone()
        if c["epi"] == EPI_RES_LN:
            flat["ln_gain"], flat["ln_bias"] = d["gain"].clone(), d["beta"].clone()
        d["flat"] = flat
        out.append(d)
    return out


def out_dtype(c, dtype):
    return F32 if c["epi"] in (EPI_RES_F32, EPI_F32, EPI_RES_LN) else dtype


def ntiles_of(c, p):
    tn = TILE_N[c["family"]]
    return (p["N"] + tn - 1) // tn


def counter_offsets(c):
    """First counter of every EPI_RES_LN problem, laid out as the forward does: one per 64-row block, problem after problem."""
    offs, n = [], 0
    for p in c["probs"]:
        offs.append(n)
        n += (p["M"] + 63) // 64
    return offs, n


def fresh_outputs(c, dt):
    """Per problem the flat output buffers, all-ones bits (counters: zero -- the one state the caller provides)."""
    dtype = DTYPES[dt]
    outs = []
    for p in c["probs"]:
        o = dict(C=sentinel(p["c"]["numel"], out_dtype(c, dtype)))
        if c["epi"] == EPI_SOFTPART:
            n = p["batch"] * p["M"] * ntiles_of(c, p) + C_PAD
            o["stat_m"], o["stat_l"] = sentinel(n, F32), sentinel(n, F32)
        if c["epi"] == EPI_RES_LN:
            if p["y32"]:
                o["ln_y32"] = sentinel(p["y32"]["numel"], F32)
            if p["y16"]:
                o["ln_y16"] = sentinel(p["y16"]["numel"], dtype)
        outs.append(o)
    return outs


# =========================================================================================================================================
# references and bounds
# =========================================================================================================================================
def kv_index(p, rows=None):
    """Flat cache index [M, N] of the head-major scatter."""
    tok, items, heads = p["kv"]
    M, N = p["M"] if rows is None else rows, p["N"]
    m, n = torch.arange(M)[:, None], torch.arange(N)[None, :]
    hidden = heads * 64
    sel, within = n // hidden, n % hidden
    return ((((sel * items + m // tok) * heads + within // 64) * tok + m % tok) * 64 + within % 64)


def _w_rows(p, W):
    """[Bw, N, K] float64 view of the weights as the product sees them (w_kwrap: walked twice; K-major: transposed, rows >= k_rows repeat the last)."""
    Wd = W.double()
    if p["k_rows"]:
        k = torch.arange(p["K"]).clamp(max=p["k_rows"] - 1)
        return Wd[:, k, :].transpose(1, 2)
    if p["w_kwrap"]:
        return torch.cat([Wd, Wd], dim=2)
    return Wd


def _factor_cols(p, g):
    """[B, M, K] the factor that multiplies A[m][k] (float32 values as float64)."""
    t = (torch.arange(p["K"]) // 176).clamp(max=p["ps_ntiles"] - 1)
    return g.double()[:, t, :p["M"]].transpose(1, 2)


@functools.lru_cache(maxsize=4)
def reference(name: str, dt: str):
    """Per problem a dict: ref / bound [B, M, N] float64 of C (SOFTPART: s, eK for the staged checks)."""
    c = BY_NAME[name]
    dtype = DTYPES[dt]
    epi = c["epi"]
    refs = []
    for p, d in zip(c["probs"], inputs(name, dt)):
        K = p["K"]
        Ad, Wd = d["A"].double(), _w_rows(p, d["W"])
        if d["g"] is not None:
            gd = _factor_cols(p, d["g"])
            ag = Ad * gd
            u = U[dtype]
            term = Ad.abs() * (u * gd + sub_abs(dtype)) + u * ag.abs() + sub_abs(dtype) if dtype == torch.float16 else (u + U32) * ag.abs()
            term = torch.where(Ad == 0, torch.zeros_like(term), term)            # 0 x anything finite is an exact 0
            acc = ag @ Wd.transpose(1, 2)
            e32 = term @ Wd.abs().transpose(1, 2) + (K + 1) * U32 * ((ag.abs() + term) @ Wd.abs().transpose(1, 2))
            refs.append(dict(ref=acc, bound=round_bound(acc, e32, dtype)))
            continue
        acc = Ad @ Wd.transpose(1, 2)
        mag = Ad.abs() @ Wd.abs().transpose(1, 2)
        if d["bias"] is not None:
            acc = acc + d["bias"].double()[:, None, :]
            mag = mag + d["bias"].double().abs()[:, None, :]
        eK = (K + 1) * U32 * mag
        if epi == EPI_SOFTPART:
            refs.append(dict(s=acc, eK=eK))
        elif epi == EPI_F32:
            refs.append(dict(ref=acc, bound=eK))
        elif epi in (EPI_RES_F32, EPI_RES_LN):
            Rd = d["R"].double()[None]
            refs.append(dict(ref=acc + Rd, bound=(K + 2) * U32 * (mag + Rd.abs())))
        elif epi == EPI_GELU_OP:
            ref = gelu64(acc)
            e32 = 1.13 * eK + 0.5 * acc.abs() * E_ERF + 3 * U32 * ref.abs()
            refs.append(dict(ref=ref, bound=round_bound(ref, e32, dtype)))
        else:
            refs.append(dict(ref=acc, bound=round_bound(acc, eK, dtype)))
    return refs


def ln_check(p, d, C_rows, y32, y16, dtype):
    """The LayerNorm outputs against the float64 LayerNorm of the C rows returned.  C_rows / y32 [M, N] fp32, y16 [M, N] T (either may be
    None).  Returns {"ln_y32": ratio, "ln_y16": 0 / inf}."""
    M, N = C_rows.shape
    ref, bound = ln_ref(C_rows, d["gain"][None].expand(M, N), d["beta"][None].expand(M, N), LN_EPS)
    r = {}
    if y32 is not None:
        r["ln_y32"] = ratio(y32, ref, bound)
    if y16 is not None:
        if y32 is not None:
            r["ln_y16"] = 0.0 if torch.equal(y16.view(torch.int16), y32.to(dtype).view(torch.int16)) else float("inf")
        else:
            r["ln_y16"] = ratio(y16, ref, round_bound(ref, bound, dtype))
    return r


def softpart_check(p, c, ref, Pt, sm, sl, dtype):
    """The three stages of EPI_SOFTPART.  Pt [B, M, ntiles * 176] T, sm / sl [B, M, ntiles] fp32.  Returns ratios."""
    B, M, N = ref["s"].shape
    nt = ntiles_of(c, p)
    pad = nt * 176 - N
    a = float(torch.tensor(ALPHA, dtype=F32).double())
    s = torch.nn.functional.pad(ref["s"], (0, pad), value=-float("inf")).view(B, M, nt, 176)
    eK = torch.nn.functional.pad(ref["eK"], (0, pad), value=0.0).view(B, M, nt, 176)
    smd = sm.double()
    m_ref = a * s.amax(-1)
    r = {"stat_m": ratio(sm, m_ref, a * eK.amax(-1) + U32 * smd.abs())}
    y = a * s - smd[..., None]
    p_ref = torch.exp2(y)                                                  # exp2(-inf) = 0 on the ragged tail
    dlt = a * eK + U32 * y.abs().nan_to_num(posinf=0.0)
    e32 = p_ref * (math.log(2.0) * dlt + 2 * U32) + 2.0 ** -126
    pb = round_bound(p_ref, e32, dtype)
    valid = (torch.arange(nt * 176) < N).view(nt, 176)
    pb = torch.where(valid, pb, torch.zeros_like(pb))                       # the tail: exact zeros
    Ptd = Pt.view(B, M, nt, 176)
    r["P~"] = ratio(Ptd, p_ref, pb)
    tot = Ptd.double().sum(-1)
    r["stat_l"] = ratio(sl, tot, 176 * U32 * tot)
    return r


# =========================================================================================================================================
# ownership: which elements of an output buffer a launch must rewrite (True), may rewrite (None mask) and must leave alone
# =========================================================================================================================================
def owned(c, p, what):
    """(must [numel] bool, may [numel] bool) of output buffer ``what``."""
    B, M, N = p["batch"], p["M"], p["N"]
    if what == "C":
        n = p["c"]["numel"]
        must, may = torch.zeros(n, dtype=torch.bool), torch.zeros(n, dtype=torch.bool)
        if c["epi"] == EPI_KV:
            must[kv_index(p).reshape(-1)] = True
            return must, may
        cols = _out_cols(c, p)
        must[index(p["c"], M, N if c["epi"] != EPI_SOFTPART else cols, B).reshape(-1)] = True
        if cols > N and c["epi"] != EPI_SOFTPART:
            may[index(p["c"], M, cols, B).reshape(-1)] = True
            may &= ~must
        return must, may
    if what in ("stat_m", "stat_l"):
        n = B * M * ntiles_of(c, p)
        must = torch.zeros(n + C_PAD, dtype=torch.bool)
        must[:n] = True
        return must, torch.zeros_like(must)
    l = p["y32"] if what == "ln_y32" else p["y16"]
    must = torch.zeros(l["numel"], dtype=torch.bool)
    must[index(l, M, N).reshape(-1)] = True
    return must, torch.zeros_like(must)


# =========================================================================================================================================
# check: one launch's output buffers against the references
# =========================================================================================================================================
def check(name: str, dt: str, outs, counters=None):
    """outs: per problem the flat output buffers after the launch (dict as fresh_outputs); counters: the flat counter buffer after it
    (EPI_RES_LN).  Returns (ratios {key: worst |d| / bound}, failures [str])."""
    c = BY_NAME[name]
    dtype = DTYPES[dt]
    epi = c["epi"]
    ratios, fails = {}, []

    def note(key, v, i):
        ratios[key] = max(ratios.get(key, 0.0), v)
        if not v <= 1.0:
            fails.append(f"problem {i} {key}: |d| / bound = {v:.4g}")

    for i, (p, d, ref, o) in enumerate(zip(c["probs"], inputs(name, dt), reference(name, dt), outs)):
        B, M, N = p["batch"], p["M"], p["N"]
        for what, buf in o.items():
            must, may = owned(c, p, what)
            s = is_sentinel(buf)
            if (s & must).any():
                fails.append(f"problem {i} {what}: {int((s & must).sum())} owned elements left unwritten")
            if (~s & ~must & ~may).any():
                fails.append(f"problem {i} {what}: {int((~s & ~must & ~may).sum())} elements written outside the owned region")
        if epi == EPI_KV:
            note("C", ratio(o["C"][kv_index(p)][None], ref["ref"], ref["bound"]), i)
            continue
        if epi == EPI_SOFTPART:
            nt = ntiles_of(c, p)
            Pt = o["C"][index(p["c"], M, nt * 176, B)]
            sm, sl = (o[k][:B * M * nt].view(B, M, nt) for k in ("stat_m", "stat_l"))
            for k, v in softpart_check(p, c, ref, Pt, sm, sl, dtype).items():
                note(k, v, i)
            continue
        Cm = o["C"][index(p["c"], M, N, B)]
        note("C", ratio(Cm, ref["ref"], ref["bound"]), i)
        if epi == EPI_RES_LN:
            y32 = o["ln_y32"][index(p["y32"], M, N)][0] if p["y32"] else None
            y16 = o["ln_y16"][index(p["y16"], M, N)][0] if p["y16"] else None
            for k, v in ln_check(p, d, Cm[0], y32, y16, dtype).items():
                note(k, v, i)
    if epi == EPI_RES_LN:
        if not bool((counters == 0).all()):
            fails.append(f"{int((counters != 0).sum())} counters are not zero after the launch")
        ratios["counters"] = 0.0 if bool((counters == 0).all()) else float("inf")
    return ratios, fails


# =========================================================================================================================================
# fp32 emulation of every form (mutant = None: faithful)
# =========================================================================================================================================
def _fma32(a, b, cc):
    """fl32(a b + c) for fp32 tensors (the product is exact in float64; the double rounding is below anything measured here)."""
    return (a.double() * b.double() + cc.double()).float()


def _acc32(c, p, A, W, start=None, mutant=None):
    """fp32 accumulation step by step: A [M, K] T, W [N, K] T (as the product sees them) -> [M, N] fp32.  The ring kernel adds its even and
    its odd K tiles separately (``start``, the residual + bias, rides the even ones); the other loops add step after step."""
    K = A.shape[1]
    step = K_STEP.get(c["family"], 64)
    Af, Wf = A.float(), W.float()
    tiles = [(k0, k0 + step) for k0 in range(0, K, step)]
    if mutant == "last_k_step_dropped":
        tiles = tiles[:-1]
    if mutant == "odd_k_tiles_dropped" and len(tiles) % 2:
        tiles = tiles[:-1]
    if mutant == "kwrap_single_pass":
        tiles = tiles[:len(tiles) // 2]
    zero = torch.zeros(A.shape[0], W.shape[0])
    parts = [zero if start is None else start.clone(), zero.clone()]
    for t, (k0, k1) in enumerate(tiles):
        g = t & 1 if c["family"] in RING else 0
        parts[g] = parts[g] + Af[:, k0:k1] @ Wf[:, k0:k1].T
    return parts[0] + parts[1]


def emulate(name: str, dt: str, mutant=None, counters=None):
    """The launch in fp32 on the CPU: returns (outs as fresh_outputs after the launch, counters after it).  ``counters``: the counter buffer
    before the launch (default zeros)."""
    c = BY_NAME[name]
    dtype = DTYPES[dt]
    epi = c["epi"]
    ins = inputs(name, dt)
    outs = fresh_outputs(c, dt)
    offs, ncnt = counter_offsets(c)
    cnt = torch.zeros(ncnt, dtype=torch.int32) if counters is None else counters.clone()
    for i, (p, d, o) in enumerate(zip(c["probs"], ins, outs)):
        B, M, N, K = p["batch"], p["M"], p["N"], p["K"]
        od = out_dtype(c, dtype)
        extra = 1 if mutant == "rows_past_M_stored" else 0           # the row behind the last, computed on the clamped row M - 1
        cols = _out_cols(c, p)
        Cl = torch.zeros(B, M + extra, cols, dtype=od)
        nt = ntiles_of(c, p)
        sm, sl = torch.zeros(B, M, nt), torch.zeros(B, M, nt)
        for b in range(B):
            ba = 0 if mutant == "a_batch_stride_ignored" else b
            bw = 0 if mutant == "w_batch_stride_ignored" else b
            A = d["A"][ba]
            W = _w_rows(p, d["W"])[bw].to(dtype)
            bias = None
            if d["bias"] is not None:
                src = ins[0]["bias"] if mutant == "bias_of_problem_0" else d["bias"]
                bias = src[0 if (src.shape[0] == 1 or mutant == "bias_stride_ignored") else b]
            if d["g"] is not None:      # the row factors on A's way into the MFMA
                t = torch.arange(K) // 176
                gsrc = d["g"][b]
                if mutant == "pscale_tile_unclamped":
                    gsrc = torch.cat([gsrc, torch.full((K // 176 + 1, 512), float("nan"))])      # the slices behind the last: not the caller's
                else:
                    t = t.clamp(max=p["ps_ntiles"] - 1)
                gf = gsrc[t, :M].T
                A = (A * gf.to(dtype)) if dtype == torch.float16 else (A.float() * gf).to(dtype)
            if extra:
                A = torch.cat([A, A[-1:]])
            start = None
            if epi in (EPI_RES_F32, EPI_RES_LN):       # bias + residual inside the accumulators
                R = d["R"]
                if mutant == "residual_through_c_view":   # the residual buffer addressed with C's view: other elements of it (NaN where nothing lives)
                    ridx = (index(p["c"], M, N)[0] - p["c"]["off"] + p["r"]["off"]).clamp(max=p["r"]["numel"] - 1)
                    R = d["flat"]["R"][ridx]
                if extra:
                    R = torch.cat([R, R[-1:]])
                start = R + (bias if bias is not None else 0.0)
            acc = _acc32(c, p, A, W, start, mutant)
            if start is None and bias is not None:
                acc = acc + bias
            if epi == EPI_SOFTPART:
                a32 = torch.tensor(ALPHA, dtype=F32)
                x = torch.nn.functional.pad(acc, (0, nt * 176 - N), value=-float("inf")).view(M, nt, 176)
                if mutant == "ragged_tail_in_sum":     # the tail columns repeat weight row N - 1 and are counted
                    x = torch.where(torch.isinf(x), acc[:, -1:, None].expand_as(x), x)
                mx = x.amax(-1) * a32
                pf = torch.exp2(_fma32(x, a32, -mx[..., None]))
                po = pf.to(dtype)
                sm[b], sl[b] = mx, (pf if mutant == "tile_sum_unrounded" else po.float()).sum(-1)
                Cl[b] = po.view(M, nt * 176)
                continue
            if epi == EPI_GELU_OP:
                acc = gelu_emulate(acc)
            if cols > N:
                acc = torch.nn.functional.pad(acc, (0, cols - N), value=0.0)
            Cl[b] = acc.to(od)
        if epi == EPI_KV:
            idx = kv_index(p)
            if mutant == "kv_head_swapped":
                tok, items, heads = p["kv"]
                q = dict(p, kv=(tok, items, heads))
                n = torch.arange(N)
                idx = kv_index(q)[:, (n // 64 // heads) * heads * 64 + (heads - 1 - (n // 64) % heads) * 64 + n % 64]
            o["C"][idx.reshape(-1)] = Cl.reshape(-1)
        else:
            idx = index(p["c"], M + extra, cols, B)
            ok = idx < p["c"]["numel"]
            o["C"][idx[ok]] = Cl[ok]
        if epi == EPI_SOFTPART:
            o["stat_m"][:B * M * nt] = sm.reshape(-1)
            o["stat_l"][:B * M * nt] = sl.reshape(-1)
        if epi == EPI_RES_LN:
            # a row block's LayerNorm runs when its counter reaches ntiles - 1 + 1; a counter that did not start at zero never gets there
            blocks = (M + 63) // 64
            mine = cnt[offs[i]:offs[i] + blocks]
            ran = (mine == 0)[torch.arange(M) // 64]
            x = Cl[0, :M].clone()
            if mutant == "ln_before_last_tile":
                x[:, -96:] = float("nan")
            y = ln_emulate(x, d["gain"], d["beta"], LN_EPS, by_division=True)
            for key, l in (("ln_y32", p["y32"]), ("ln_y16", p["y16"])):
                if l:
                    idx = index(l, M, N)[0][ran]
                    o[key][idx.reshape(-1)] = y[ran].reshape(-1).to(o[key].dtype)
            cnt[offs[i]:offs[i] + blocks] = torch.where(mine == 0, torch.tensor(nt if mutant == "counter_left_set" else 0, dtype=torch.int32), mine + nt)
    return outs, cnt


# =========================================================================================================================================
# descriptors of mra_debug_gemm / mra_debug_gemm_plan (ctypes; shared by the plan and refusal checks on the CPU and the launches on the GPU)
# =========================================================================================================================================
BUFFERS = ("A", "W", "bias", "C", "R", "ln_gain", "ln_bias", "ln_y32", "ln_y16", "ln_counter", "stat_m", "stat_l", "pscale")


def buffer_sizes(c, dt):
    """Per problem {buffer: (numel, torch dtype)} of every buffer the launch takes (counters: one buffer per launch, listed under problem 0)."""
    dtype = DTYPES[dt]
    sizes = []
    _, ncnt = counter_offsets(c)
    for p, d, o in zip(c["probs"], inputs(c["name"], dt), fresh_outputs(c, dt)):
        s = {k: (v.numel(), v.dtype) for k, v in d["flat"].items()}
        s.update({k: (v.numel(), v.dtype) for k, v in o.items()})
        if c["epi"] == EPI_RES_LN:
            s["ln_counter"] = (ncnt, torch.int32)
        sizes.append(s)
    return sizes


def descriptors(c, dt, addr):
    """The mra_gemm_desc array of a case.  ``addr(i, buffer)`` -> (address of the buffer's first element, its bytes) or None."""
    from mraudio_amd import _lib as L
    dtype = DTYPES[dt]
    esz = {"A": 2, "W": 2, "C": torch.empty(0, dtype=out_dtype(c, dtype)).element_size(), "ln_y16": 2}
    offs, _ = counter_offsets(c)
    arr = (L.mra_gemm_desc * len(c["probs"]))()
    for i, p in enumerate(c["probs"]):
        d = arr[i]
        d.struct_bytes = C.sizeof(L.mra_gemm_desc)
        first = {"A": p["a"]["off"], "C": p["c"]["off"], "R": p["r"]["off"] if p["r"] else 0, "ln_counter": offs[i],
                 "ln_y32": p["y32"]["off"] if p.get("y32") else 0, "ln_y16": p["y16"]["off"] if p.get("y16") else 0}
        for b in BUFFERS:
            got = addr(0 if b == "ln_counter" else i, b)
            if got is None:
                continue
            base, nbytes = got
            skip = first.get(b, 0) * esz.get(b, 4)
            setattr(d, b, base + skip)
            setattr(d, {"A": "a_bytes", "W": "w_bytes", "C": "c_bytes", "R": "r_bytes"}.get(b, b + "_bytes"), nbytes - skip)
        d.a_view[:] = p["a"]["view"]
        d.c_view[:] = p["c"]["view"]
        if p["r"]:
            d.r_view[:] = p["r"]["view"]
        if p.get("y32"):
            d.ln_y32_view[:] = p["y32"]["view"]
        if p.get("y16"):
            d.ln_y16_view[:] = p["y16"]["view"]
        d.M, d.N, d.K = p["M"], p["N"], p["K"]
        if p["kv"]:
            d.kv_tokens, d.kv_items, d.kv_heads = p["kv"]
        if p["batch"] > 1:
            d.batch = p["batch"]
            d.a_bs = p["a"]["bs"]
            d.w_bs = p.get("w_bs", (p["k_rows"] * p["N"]) if p["k_rows"] else p["N"] * (p["K"] // 2 if p["w_kwrap"] else p["K"]))
            d.c_bs_bytes = p["c"]["bs"] * esz["C"]
            d.bias_bs = p.get("bias_bs", 0)
        d.n_ragged, d.w_kwrap = p["n_ragged"], p["w_kwrap"]
        if p["k_rows"]:
            d.w_ld, d.k_rows = p["N"], p["k_rows"]
        d.ps_ntiles = p["ps_ntiles"]
        d.ln_eps, d.alpha = LN_EPS, ALPHA
        d.tile_cfg = c["tile"] if i == 0 else GT_AUTO
        d.persist = c["persist"]
    return arr


def fake_addr(c, dt):
    """Addresses for the host-only checks: every buffer at a 4 KiB boundary of its own, never dereferenced."""
    sizes = buffer_sizes(c, dt)
    table, nxt = {}, 1 << 20
    for i, s in enumerate(sizes):
        for b, (numel, tdt) in s.items():
            nbytes = numel * torch.empty(0, dtype=tdt).element_size()
            table[(i, b)] = (nxt, nbytes)
            nxt += (nbytes + 8191) // 4096 * 4096
    return lambda i, b: table.get((i, b))
