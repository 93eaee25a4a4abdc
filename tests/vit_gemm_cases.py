"""Shared by tests/test_vit_gemm_cases_cpu.py and tests/test_gpu_gemm_vit.py (not a test module): the launch forms of csrc/gemm.hip that only
the ViT-g encoder issues (csrc/vit.hip, mra_vit_forward) and the three small kernels its folded LayerNorm rests on, as a CASE TABLE with seeded
inputs rounded to the operand type, float64 references, DERIVED bounds and an fp32 emulation of every form with named mutants.  Method,
notation and helpers are those of tests/gemm_cases.py (``G``): u32 = 2^-24, u = U[T], sub = 2^-25 [f16], every bound worst case and first order,
nothing fitted to GPU output; an MFMA is assumed no worse than a chain of fp32 additions of its exact products.  G.check is bound to G's own
table, so this file has a ``check`` of the same form: flat NaN-padded inputs, all-ones outputs, owned elements rewritten, all others untouched.

acc = A W^T in fp32, mag = |A| |W|^T, eK = (K + 1) u32 (mag + |bias|) as in G (K products and the bias in K links of any order).

EPI_RES_F32       C = acc + bias + R (the accumulators start at bias + R):      |C - ref| <= (K + 2) u32 (mag + |bias| + |R|)
EPI_RES_OP        C = T(float(T(acc + bias)) + float(aux)), ref = acc + bias + aux with the aux values AS GIVEN (in place: the stream before
                  the launch).  o = T(acc + bias) errs by e1 = round_bound(acc + bias, eK, T); the fp32 add rounds once, u32 (|ref| + e1); then T:
                      |C - ref| <= round_bound(ref, e1 + u32 (|ref| + e1), T)
EPI_RES_OP_STAT   C as EPI_RES_OP.  Per (row, 64-column block) the kernel sums the n = 64 values AS STORED (exact in fp32) in any order,
                  mean' = fl(sum) / 64 (exact scaling), then the squared deviations from mean' by fma.  Against the float64 mean and ssd of
                  the C values the launch RETURNED:
                      dm   = |mean' - mean| <= n u32 sum|x| / n = u32 sum|x|
                      d_i' = fl(x_i - mean'):  |d_i' - d_i| <= dm + u32 |d_i|, so |d_i'^2 - d_i^2| <= 2 |d_i| dm + dm^2 + 2 u32 d_i^2
                      |ssd' - ssd| <= sum_i (2 |d_i| dm + dm^2) + (n + 2) u32 ssd          (n links of the sum, one rounding per fma)
EPI_RES_F32_STAT  C is EPI_RES_F32's.  gemm_p8_tile stores C through epilogue<.., EPI_RES_F32, PRE = true>, which adds a zero bias vector to a COPY
                  (v = acc + 0) and leaves the accumulators as they were; the staged copy-out then rounds the same accumulators (bias = nullptr:
                  acc + 0 again).  So ln_y16 == T(C returned) BIT FOR BIT.  The statistics of each 128-column group (a wave's half tile) are taken
                  from those accumulators too: the bound above with n = 128, against float64 statistics of the returned C.
EPI_LNF_OP        v = fma(rstd, fma(-mu, cs, acc), b'), C = T(v); ref = rstd (A W'^T - mu cs) + b' in float64 from the mu, rstd, cs, b' GIVEN.
                  acc errs by eK (no bias inside: mag alone); the inner fma rounds once a value of at most |acc| + |mu cs| -- THAT term carries the
                  cancellation when the row mean is far from zero -- the scaling multiplies by |rstd|, the outer fma rounds once:
                      ei  = eK + u32 (|acc| + |mu cs|)
                      e32 = |rstd| ei + u32 (|ref| + |rstd| ei);        |C - ref| <= round_bound(ref, e32, T)
EPI_LNF_GELU_OP   the same pre-activation, then G's GELU treatment: |C - gelu(pre)| <= round_bound(gelu(pre), 1.13 e32 + eg(pre), T),
                  eg(x) = |x| E_ERF / 2 + 3 u32 |gelu(x)|.
EPI_OP / EPI_GELU_OP  as G.  A persistent launch must also equal the one-workgroup-per-tile launch bit for bit (same tiles, same order of K).

---- the chain (case 10) ----------------------------------------------------------------------------------------------------------------
EPI_RES_F32_STAT -> vit_group_stats -> EPI_LNF_OP on the first launch's ln_y16 = x16, weights from vit_fold_weight.  Against
ref = LayerNorm_float64(C returned; gain, beta) W^T + b with the UNFOLDED w (operand dtype), i.e. r sum_k (x_k - m) g_k w_k + sum_k beta_k w_k + b.
With x16 = T(x), W' = T(w g), (mu', rstd') the merged statistics (their bounds dmu, drs from the vit_group_stats section), cs and b' as returned
by vit_fold_weight (their bounds dcs, dbf):
    operands   sum_k |x16 - x| |w g| <= u sum |x| |w g| (+ sub K max|w g| [f16]);   sum_k |x16| |W' - w g| <= (u + u32) sum |x16| |w g| (+ sub sum |x16|)
    statistics dmu = mean_g dm_g + merge dmu;  dM2 = sum_g (eq_g + 2 n |d_g| dm_g) + merge dM2  (dm_g, eq_g: the group bounds of the first launch)
    mean term  |mu' cs - m sum w g| <= dmu |cs| + |m| (dcs + sum_k |W' - w g|)
    inner      E = operands + mean term + launch ei (above, from the values the launch was GIVEN)
    total      e32 = r E + drs |inner_ref| + dbf + u32 (|ref| + r E),  inner_ref = sum_k (x_k - m) g_k w_k;     round_bound(ref, e32, T)

---- vit_fold_weight -----------------------------------------------------------------------------------------------------------------------
Wf = T(fl(w g)): one fp32 product rounded once more,  |Wf - w g| <= round_bound(w g, u32 |w g|, T)
cs = the sum of the K values Wf RETURNED, a lane's K / 64 by serial adds and then the wave tree: K links of any order at most,
     |cs - sum Wf| <= K u32 sum |Wf|
bf = bias + sum_k beta_k w_k by an fma chain per lane, the wave sum and the bias add:  |bf - ref| <= (K + 1) u32 (sum |beta w| + |bias|)

---- vit_group_stats ------------------------------------------------------------------------------------------------------------------------
G groups of n columns, (a_i, y_i) = (mean, ssd) of group i.  The kernel: mean' = fl(sum a_i) / G serially, d_i' = fl(a_i - mean'),
M2' = sum_i fl(y_i + fl(fl(n d_i') d_i')), var' = M2' / (n G) + eps, rstd' = 1 / sqrt(var').  Against the float64 Chan merge of the groups GIVEN:
    dmu  = (G + 1) u32 mean_i |a_i|                                  (G - 1 adds and the division)
    dM2  = n sum_i (2 |d_i| (dmu + u32 |d_i|) + dmu^2) + (G + 4) u32 M2      (two products and one add per term, G links)
    rstd through 1 / sqrt as the LayerNorm family of qformer_kernel_cases (ln_ref: (10 + D / 2) u32 + (dm r)^2 / 2 relative, D the depth of
    the sum): here the sum's depth is G and the mean's effect on M2 is dM2 itself,
    drs  = r (dM2 / (2 (M2 + n G eps)) + (10 + G / 2) u32)
Against the float64 mean and variance of a ROW whose groups were computed exactly and rounded to fp32 once (|a_i| u32, y_i u32 of input error):
    dmu += u32 mean |a_i|;   dM2 += u32 M2 + n sum_i 2 |d_i| u32 |a_i|

---- vit_row_stats / vit_row_stats16 ----------------------------------------------------------------------------------------------------------
One wave per row, D / 64 values per lane: mean by D links and a division, deviations in registers, their squares by D links.  The LayerNorm
family's bound once more (qformer_kernel_cases.ln_ref with depth(D) = D / 64 + 6 for the lane-serial-then-tree sums):
    dmu = (depth + 2) u32 mean|x|;    drs = r ((10 + depth / 2) u32 + (dmu r)^2 / 2)
The operand-dtype copy is T(x) bit for bit."""
import ctypes as C
import functools
import math

import torch

import gemm_cases as G
from gemm_cases import C_PAD, C_TAIL, DTYPES, F32, F64, U, U32, depth, gelu64, index, is_sentinel, lay, place, plain_lay, ratio, round_bound, sentinel, sub_abs  # noqa: F401
from train_kernel_cases import E_ERF, gelu_emulate

EPI_OP, EPI_GELU_OP, EPI_RES_F32, EPI_RES_OP, EPI_RES_F32_STAT, EPI_LNF_OP, EPI_LNF_GELU_OP, EPI_RES_OP_STAT = 0, 1, 2, 8, 10, 11, 12, 13
EPI_NAME = {0: "OP", 1: "GELU_OP", 2: "RES_F32", 8: "RES_OP", 10: "RES_F32_STAT", 11: "LNF_OP", 12: "LNF_GELU_OP", 13: "RES_OP_STAT"}
GT_AUTO, GT_128, GT_256, GT_P8_TAIL, GT_P8_MIXED = 0, 2, 3, 7, 8
GF_V1_64, GF_V1_128, GF_P8_256, GF_P8_MIXED = 0, 1, 4, 9
CUS = 256
VIT_EPS = 1e-6
STAT_GUARD = 8      # floats behind the statistics a launch writes: keep the sentinel

# Every (family, epilogue) pair mra_vit_forward reaches and G's table does not hold, with its call site in csrc/vit.hip.  nqkv = 3 heads 96 and
# mlp are multiples of 256 (mra_vit_create refuses anything else), so QKV / fc1 never take the mixed tile: (GF_P8_MIXED, EPI_OP) and
# (GF_P8_MIXED, EPI_F32) are instantiated but not reached and are not listed.  GT_P8_TAIL has no call site outside tests/native.
PAIRS = {
    (GF_P8_256, EPI_LNF_OP): "vit qkv gemm, ln_fold 1 (tile_cfg GT_256), per tile and persistent (gemm_persist)",
    (GF_P8_256, EPI_LNF_GELU_OP): "vit fc1 gemm, ln_fold 1",
    (GF_P8_MIXED, EPI_RES_F32_STAT): "residual_gemm(stat) of the projection and fc2, fp32 stream",
    (GF_P8_MIXED, EPI_RES_OP): "residual_gemm of the projection and fc2, residual_dtype = op, ln_fold 0 and the last block's fc2",
    (GF_P8_MIXED, EPI_RES_OP_STAT): "residual_gemm(stat), residual_dtype = op",
    (GF_P8_MIXED, EPI_RES_F32): "residual_gemm with ln_fold 0, and the last block's fc2",
    (GF_P8_256, EPI_OP): "vit qkv gemm with ln_fold 0 at >= 512 tiles, persistent",
    (GF_P8_256, EPI_GELU_OP): "vit fc1 gemm with ln_fold 0 at >= 512 tiles, persistent",
    (GF_V1_64, EPI_RES_F32): "patch embedding gemm below 23 frames: R = pos[1:] broadcast (item stride 0), C skips each frame's cls row",
    (GF_V1_128, EPI_RES_F32): "patch embedding gemm from 23 frames on (GT_AUTO reaches the 128 tile at >= 384 tiles)",
}

ROW_MUTANTS = {
    1: ("last_k_step_dropped", "odd_pair_row_tile_computed", "tail_second_half_dropped"),
    2: ("last_k_step_dropped", "tail_rows_past_M_stored"),
    3: ("last_k_step_dropped", "stat_group_other_width", "y16_rounded_before_residual"),
    4: ("residual_after_neighbour_store", "last_k_step_dropped"),
    5: ("stat_group_other_width", "stat_of_unrounded"),
    6: ("mu_not_applied", "cs_from_unrounded_w", "last_k_step_dropped"),
    7: ("mu_not_applied", "dead_row_wraps"),
    8: ("persistent_second_round_skipped",),
    9: ("residual_through_c_view", "cls_row_written"),
}


def _gen(*key):
    return torch.Generator().manual_seed((977 + sum((i + 1) * 7919 * int(k) for i, k in enumerate(key))) % (2 ** 31))


# =========================================================================================================================================
# the case table
# =========================================================================================================================================
CASES = []
BY_NAME = {}


def case(row, name, epi, tile, family, M, N, K, **kw):
    assert name not in BY_NAME, name
    c = dict(row=row, name=name, epi=epi, tile=tile, family=family, M=M, N=N, K=K, persist=0, aux=None, rows="plain", c=None, r=None, y16=None,
             table=True)
    c.update(kw)
    cols16 = epi not in (EPI_RES_F32, EPI_RES_F32_STAT)
    if c["c"] is None:
        c["c"] = plain_lay(M, N, C_PAD, C_TAIL)
    if epi in (EPI_RES_F32, EPI_RES_F32_STAT) and c["r"] is None:
        c["r"] = plain_lay(M, N)
    if epi == EPI_RES_F32_STAT:
        c["y16"] = plain_lay(M, N, C_PAD, C_TAIL)      # a padded row stride (a multiple of 8)
    c["out_f32"] = not cols16
    if c["table"]:
        CASES.append(c)
    BY_NAME[name] = c
    return c


def persist_shape(cus):
    """Rows of the persistent case: 17 column tiles of 256, row tiles so that cus < tiles < 2 cus, the last one ragged (40 rows)."""
    mtiles = cus // 17 + 2
    assert cus < 17 * mtiles < 2 * cus, cus
    return (mtiles - 1) * 256 + 40


def persist_cases(cus):
    """The three persistent cases for a device of ``cus`` compute units (registered on first use; 256 CUs are in the table)."""
    out = []
    M = persist_shape(cus)
    for epi in (EPI_LNF_OP, EPI_OP, EPI_GELU_OP):
        name = f"p8_256 persistent {EPI_NAME[epi]} M{M} N4352 K128"
        # tile_cfg GT_256: below 512 tiles GT_AUTO (pick_tile) takes the 128 tile, and the case must lie between one and two rounds of the chip
        out.append(BY_NAME.get(name) or case(8, name, epi, GT_256, GF_P8_256, M, 17 * 256, 128, persist=1, table=cus == CUS))
    return out


def _build_table():
    case(1, "mixed RES_F32 M600 N384 K128", EPI_RES_F32, GT_P8_MIXED, GF_P8_MIXED, 600, 384, 128)
    case(2, "mixed RES_F32 M200 N1408 K384", EPI_RES_F32, GT_P8_MIXED, GF_P8_MIXED, 200, 1408, 384)
    case(3, "mixed RES_F32_STAT M776 N1408 K1408", EPI_RES_F32_STAT, GT_P8_MIXED, GF_P8_MIXED, 776, 1408, 1408)
    case(4, "mixed RES_OP M600 N640 K256 in place", EPI_RES_OP, GT_P8_MIXED, GF_P8_MIXED, 600, 640, 256, aux="inplace")
    case(4, "mixed RES_OP M600 N640 K256 separate", EPI_RES_OP, GT_P8_MIXED, GF_P8_MIXED, 600, 640, 256, aux="separate")
    case(5, "mixed RES_OP_STAT M520 N1408 K128 in place", EPI_RES_OP_STAT, GT_P8_MIXED, GF_P8_MIXED, 520, 1408, 128, aux="inplace")
    case(6, "p8_256 LNF_OP M300 N512 K1408 rows", EPI_LNF_OP, GT_256, GF_P8_256, 300, 512, 1408, rows="exact")
    case(6, "p8_256 LNF_OP M300 N512 K1408 offset rows", EPI_LNF_OP, GT_256, GF_P8_256, 300, 512, 1408, rows="offset")
    case(7, "p8_256 LNF_GELU_OP M257 N256 K128", EPI_LNF_GELU_OP, GT_256, GF_P8_256, 257, 256, 128, rows="exact")
    persist_cases(CUS)
    # 9. patch embedding: 2 frames of 16 patches, S = 17 tokens of D = 128: R = the 16 position rows shared by both frames, C = rows 1 .. 16 of each frame
    S, D, P2 = 17, 128, 16
    case(9, "patch RES_F32 2x16 N128 K640", EPI_RES_F32, GT_AUTO, GF_V1_64, 2 * P2, D, 640, r=lay((0, P2, D), P2 * D),
         c=lay((S * D, P2, D), 2 * S * D + C_TAIL * D, D), frames=(2, S))
    P2 = 196
    S = P2 + 1
    case(9, "patch RES_F32 2x196 N128 K640 GT_128", EPI_RES_F32, GT_128, GF_V1_128, 2 * P2, D, 640, r=lay((0, P2, D), P2 * D),
         c=lay((S * D, P2, D), 2 * S * D + C_TAIL * D, D), frames=(2, S))


_build_table()


def cases_of(row):
    return [c for c in CASES if c["row"] == row]


def groups_of(c):
    """(group width, groups per row) of the statistics a case writes, or None."""
    if c["epi"] == EPI_RES_F32_STAT:
        return 128, c["N"] // 128
    if c["epi"] == EPI_RES_OP_STAT:
        return 64, c["N"] // 64
    return None


# =========================================================================================================================================
# inputs
# =========================================================================================================================================
def fold_inputs(N, K, dtype, g, with_bias=True, one_sided=False):
    """w [N, K] T, gain / beta [K], bias [N] or None, and what vit_fold_weight makes of them in float64-then-rounded form: W' = T(fl(w gain)),
    cs = fp32(sum W'), bf = fp32(bias + sum beta w); cs_unrounded = fp32(sum w gain).
    one_sided: positive weights and gain = 1 + 0.45 u, so that every product rounds DOWN to w and the K rounding errors of W' add up instead of
    cancelling: sum W' and sum w gain then differ by 0.45 u sum |w|, K / sqrt(K) times what random signs leave -- the one input family on which a
    worst-case bound at K = 1408 can tell column sums of the rounded W' from those of the unrounded one in f16."""
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dtype)
    gain = 1.0 + 0.25 * torch.randn(K, generator=g)
    if one_sided:
        w, gain = w.abs(), torch.full((K,), 1.0 + 0.45 * U[dtype])
    beta = 0.5 * torch.randn(K, generator=g)
    bias = 0.5 * torch.randn(N, generator=g) if with_bias else None
    Wf = (w.float() * gain).to(dtype)
    cs = Wf.double().sum(-1).float()
    bf = ((bias.double() if with_bias else 0.0) + (w.double() * beta.double()).sum(-1)).float()
    return dict(w=w, gain=gain, beta=beta, bias=bias, Wf=Wf, cs=cs, bf=bf, cs_unrounded=(w.double() * gain.double()).sum(-1).float())


@functools.lru_cache(maxsize=3)
def inputs(name: str, dt: str):
    """Logical A [M, K], W [N, K], bias [N], R / aux [M, N], stat [M, 2] = (mu, rstd), cs [N]; and ``flat``: the input buffers of the launch."""
    c = BY_NAME[name]
    dtype = DTYPES[dt]
    M, N, K, epi = c["M"], c["N"], c["K"], c["epi"]
    g = _gen(c["row"], M, N, K, epi, len(name))
    d = dict(R=None, aux=None, stat=None, cs=None)
    lnf = epi in (EPI_LNF_OP, EPI_LNF_GELU_OP)
    if lnf:
        x = torch.randn(M, K, generator=g) * (0.5 + torch.rand(M, 1, generator=g)) + 0.3 * torch.randn(M, 1, generator=g)
        if c["rows"] == "offset":      # the mean about 50 times the row's standard deviation: acc and mu cs cancel
            x = torch.randn(M, K, generator=g) + 50.0 * torch.where(torch.rand(M, 1, generator=g) < 0.5, -1.0, 1.0)
        d["A"] = x.to(dtype)
        xd = d["A"].double()
        mu = xd.mean(-1)
        var = ((xd - mu[:, None]) ** 2).mean(-1)
        d["stat"] = torch.stack([mu, 1.0 / torch.sqrt(var + VIT_EPS)], -1).float()
        f = fold_inputs(N, K, dtype, g, one_sided=c["rows"] == "offset")
        d["W"], d["cs"], d["bias"], d["cs_unrounded"] = f["Wf"], f["cs"], f["bf"], f["cs_unrounded"]
        if epi == EPI_LNF_GELU_OP:
            d["bias"][:8] = torch.linspace(-8.0, 8.0, 8)
    else:
        d["A"] = torch.randn(M, K, generator=g).to(dtype)
        d["W"] = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dtype)
        d["bias"] = torch.randn(N, generator=g) * 0.5
        if epi == EPI_GELU_OP:
            d["bias"][:8] = torch.linspace(-8.0, 8.0, 8)
    if c["r"] is not None:
        d["R"] = torch.randn(c["r"]["view"][1] if c.get("frames") else M, N, generator=g) * 2.0       # patch form: one set of position rows
    if c["aux"]:
        d["aux"] = (torch.randn(M, N, generator=g) * 2.0).to(dtype)
    flat = dict(A=place(d["A"][None], plain_lay(M, K), dtype), W=d["W"].reshape(-1).clone(), bias=d["bias"].clone())
    if d["R"] is not None:
        flat["R"] = place(d["R"][None], dict(c["r"], view=(0, d["R"].shape[0], c["r"]["view"][2])), F32)
    if c["aux"] == "separate":
        flat["aux"] = place(d["aux"][None], c["c"], dtype)
    if lnf:
        flat["ln_y32"] = d["stat"].reshape(-1).clone()
        flat["ln_gain"] = d["cs"].clone()
    d["flat"] = flat
    return d


def residual_rows(c, d):
    """R as row m of the problem sees it [M, N] (the patch form repeats its rows per frame)."""
    if d["R"] is None:
        return None
    return d["R"][torch.arange(c["M"]) % d["R"].shape[0]]


def fresh_outputs(c, dt):
    """The flat output buffers, all-ones bits; an in-place launch finds its stream inside C."""
    dtype = DTYPES[dt]
    od = F32 if c["out_f32"] else dtype
    o = dict(C=sentinel(c["c"]["numel"], od))
    if c["aux"] == "inplace":
        place(inputs(c["name"], dt)["aux"][None], c["c"], dtype, fill=o["C"])
    gs = groups_of(c)
    if gs:
        o["ln_y32"] = sentinel(c["M"] * gs[1] * 2 + STAT_GUARD, F32)
    if c["y16"]:
        o["ln_y16"] = sentinel(c["y16"]["numel"], dtype)
    return o


# =========================================================================================================================================
# references and bounds, by row chunks
# =========================================================================================================================================
def c_reference(c, d, dtype, r0, r1):
    """(ref, bound) float64 [r1 - r0, N] of C."""
    K, epi = c["K"], c["epi"]
    Ad, Wd = d["A"][r0:r1].double(), d["W"].double()
    acc = Ad @ Wd.T
    mag = Ad.abs() @ Wd.abs().T
    b = d["bias"].double()[None]
    if epi in (EPI_LNF_OP, EPI_LNF_GELU_OP):
        mu, rstd = d["stat"][r0:r1, 0].double()[:, None], d["stat"][r0:r1, 1].double()[:, None]
        mcs = mu * d["cs"].double()[None]
        ref = rstd * (acc - mcs) + b
        ei = (K + 1) * U32 * mag + U32 * (acc.abs() + mcs.abs())
        e32 = rstd.abs() * ei + U32 * (ref.abs() + rstd.abs() * ei)
        if epi == EPI_LNF_OP:
            return ref, round_bound(ref, e32, dtype)
        out = gelu64(ref)
        return out, round_bound(out, 1.13 * e32 + 0.5 * ref.abs() * E_ERF + 3 * U32 * out.abs(), dtype)
    eK = (K + 1) * U32 * (mag + b.abs())
    if epi in (EPI_RES_F32, EPI_RES_F32_STAT):
        Rd = residual_rows(c, d)[r0:r1].double()
        return acc + b + Rd, (K + 2) * U32 * (mag + b.abs() + Rd.abs())
    if epi in (EPI_RES_OP, EPI_RES_OP_STAT):
        t = acc + b
        e1 = round_bound(t, eK, dtype)
        ref = t + d["aux"][r0:r1].double()
        return ref, round_bound(ref, e1 + U32 * (ref.abs() + e1), dtype)
    if epi == EPI_GELU_OP:
        out = gelu64(acc + b)
        return out, round_bound(out, 1.13 * eK + 0.5 * (acc + b).abs() * E_ERF + 3 * U32 * out.abs(), dtype)
    return acc + b, round_bound(acc + b, eK, dtype)


def group_stat_check(x, stats, n):
    """x [M, N] the values as returned (any float dtype), stats [M, N / n, 2] fp32 -> (mean ratio, ssd ratio)."""
    M, N = x.shape
    xg = x.double().view(M, N // n, n)
    mean = xg.mean(-1)
    dv = xg - mean[..., None]
    ssd = (dv * dv).sum(-1)
    dm = U32 * xg.abs().sum(-1)
    eq = (2 * dv.abs() * dm[..., None] + (dm * dm)[..., None]).sum(-1) + (n + 2) * U32 * ssd
    return ratio(stats[..., 0], mean, dm), ratio(stats[..., 1], ssd, eq)


CHUNK = 1024


def check(name: str, dt: str, outs):
    """outs: the flat output buffers after the launch (dict as fresh_outputs).  Returns (ratios {key: worst |d| / bound}, failures [str])."""
    c = BY_NAME[name]
    dtype = DTYPES[dt]
    d = inputs(name, dt)
    M, N = c["M"], c["N"]
    ratios, fails = {}, []

    def note(key, v):
        ratios[key] = max(ratios.get(key, 0.0), v)
        if not v <= 1.0:
            fails.append(f"{key}: |d| / bound = {v:.4g}")

    def canary(what, buf, must):
        s = is_sentinel(buf)
        if (s & must).any():
            fails.append(f"{what}: {int((s & must).sum())} owned elements left unwritten")
        if (~s & ~must).any():
            fails.append(f"{what}: {int((~s & ~must).sum())} elements written outside the owned region")

    cidx = index(c["c"], M, N)[0]
    must = torch.zeros(c["c"]["numel"], dtype=torch.bool)
    must[cidx.reshape(-1)] = True
    canary("C", outs["C"], must)
    Cm = outs["C"][cidx]
    for r0 in range(0, M, CHUNK):
        r1 = min(M, r0 + CHUNK)
        ref, bound = c_reference(c, d, dtype, r0, r1)
        note("C", ratio(Cm[r0:r1], ref, bound))
    gs = groups_of(c)
    if gs:
        n, ng = gs
        must = torch.zeros(outs["ln_y32"].numel(), dtype=torch.bool)
        must[:M * ng * 2] = True
        canary("ln_y32", outs["ln_y32"], must)
        rm, rq = group_stat_check(Cm, outs["ln_y32"][:M * ng * 2].view(M, ng, 2), n)
        note("group mean", rm)
        note("group ssd", rq)
    if c["y16"]:
        yidx = index(c["y16"], M, N)[0]
        must = torch.zeros(c["y16"]["numel"], dtype=torch.bool)
        must[yidx.reshape(-1)] = True
        canary("ln_y16", outs["ln_y16"], must)
        same = torch.equal(outs["ln_y16"][yidx].view(torch.int16), Cm.to(dtype).view(torch.int16))
        note("ln_y16 == T(C)", 0.0 if same else float("inf"))
    return ratios, fails


# =========================================================================================================================================
# fp32 emulation (mutant = None: faithful)
# =========================================================================================================================================
def acc32(A, W, start=None, drop_last=False, step=128):
    """fp32 accumulation in K steps of 128 (the eight-phase loop's pair of 64-deep tiles), from ``start`` (bias + residual) or zero."""
    K = A.shape[1]
    Af, Wf = A.float(), W.float()
    tiles = [(k0, min(K, k0 + step)) for k0 in range(0, K, step)]
    if drop_last:
        tiles = tiles[:-1]
    acc = torch.zeros(A.shape[0], W.shape[0]) if start is None else start.clone()
    for k0, k1 in tiles:
        acc = acc + Af[:, k0:k1] @ Wf[:, k0:k1].T
    return acc


def stats32(x, n):
    """Group (mean, ssd) in fp32 as the kernels take them: [M, N] -> [M, N / n, 2]."""
    M, N = x.shape
    xg = x.float().view(M, N // n, n)
    mean = xg.sum(-1) * torch.tensor(1.0 / n, dtype=F32)
    dv = xg - mean[..., None]
    return torch.stack([mean, (dv * dv).sum(-1)], -1)


def persistent_tiles(M, N, grid):
    """(m0, n0) of the tiles a persistent grid reaches only in its second round: virtual blocks grid .. tiles - 1 through the XCD remap and the
    8-row-tile panels of tile_of (csrc/gemm.hip)."""
    mt, nt = (M + 255) // 256, N // 256
    tiles = mt * nt
    q, r = tiles >> 3, tiles & 7
    out = []
    for vb in range(grid, tiles):
        xcd = vb & 7
        tid = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + (vb >> 3)
        panel = tid // (8 * nt)
        first = panel * 8
        gsz = min(8, mt - first)
        inp = tid - panel * 8 * nt
        out.append(((first + inp % gsz) * 256, (inp // gsz) * 256))
    return out


def emulate(name: str, dt: str, mutant=None):
    """The launch in fp32 on the CPU: the output buffers as fresh_outputs after the launch."""
    c = BY_NAME[name]
    dtype = DTYPES[dt]
    d = inputs(name, dt)
    o = fresh_outputs(c, dt)
    M, N, K, epi = c["M"], c["N"], c["K"], c["epi"]
    drop = mutant == "last_k_step_dropped"
    b = d["bias"][None]
    if epi in (EPI_RES_F32, EPI_RES_F32_STAT):
        R = residual_rows(c, d)
        if mutant == "residual_through_c_view":     # the position rows addressed with C's item stride: the second frame reads behind them
            ridx = index(dict(c["c"], off=0), M, N)[0]
            R = torch.where(ridx < d["flat"]["R"].numel(), d["flat"]["R"][ridx.clamp(max=d["flat"]["R"].numel() - 1)], torch.tensor(float("nan")))
        val = acc32(d["A"], d["W"], R + b, drop)
        out = val
    elif epi in (EPI_RES_OP, EPI_RES_OP_STAT):
        ob = (acc32(d["A"], d["W"], None, drop) + b).to(dtype)
        val = ob.float() + d["aux"].float()
        out = val.to(dtype)
        if mutant == "residual_after_neighbour_store":   # the tail tile reads the stream after a neighbour has updated it: its columns add twice
            t0 = N - 128
            out[:, t0:] = (ob.float()[:, t0:] + out.float()[:, t0:]).to(dtype)
    elif epi in (EPI_LNF_OP, EPI_LNF_GELU_OP):
        acc = acc32(d["A"], d["W"], None, drop)
        mu, rstd = d["stat"][:, 0:1], d["stat"][:, 1:2]
        if mutant == "dead_row_wraps":                   # the ragged row tile's statistics read from row m % 256 instead of the clamped row
            rows = torch.arange(M)
            rows = torch.where(rows >= 256, rows - 256, rows)
            mu, rstd = mu[rows], rstd[rows]
        cs = (d["cs_unrounded"] if mutant == "cs_from_unrounded_w" else d["cs"])[None]
        inner = acc if mutant == "mu_not_applied" else G._fma32(-mu.expand(M, N), cs.expand(M, N), acc)
        val = G._fma32(rstd.expand(M, N), inner, b.expand(M, N))
        out = (gelu_emulate(val) if epi == EPI_LNF_GELU_OP else val).to(dtype)
    else:
        val = acc32(d["A"], d["W"], None, drop) + b
        out = (gelu_emulate(val) if epi == EPI_GELU_OP else val).to(dtype)
    rows = M
    if mutant in ("odd_pair_row_tile_computed", "tail_rows_past_M_stored"):   # a tile without live rows (the missing tile of an odd count, the dead half of a tail tile) runs on clamped rows and stores past M
        out = torch.cat([out, out[-1:]])
        rows = M + 1
    idx = index(c["c"], rows, N)[0]
    if mutant == "cls_row_written":                      # the C view without its one-row offset: every frame's cls row takes a patch row
        idx = idx - c["c"]["off"]
    live = torch.ones(rows, N, dtype=torch.bool)
    if mutant == "tail_second_half_dropped":             # rows 256 .. 511 of every pair in the last 128 columns
        live[(torch.arange(rows) % 512) >= 256, N - 128:] = False
    if mutant == "persistent_second_round_skipped":
        for m0, n0 in persistent_tiles(M, N, CUS & ~7):
            live[m0:m0 + 256, n0:n0 + 256] = False
    ok = (idx < c["c"]["numel"]) & live
    o["C"][idx[ok]] = out[ok]
    gs = groups_of(c)
    if gs:
        n, ng = gs
        src = val if mutant == "stat_of_unrounded" else out[:M]
        if mutant == "stat_group_other_width":           # the statistics written at the other epilogue's index (m groups' + g), groups' = N / n'
            n2 = 192 - n
            st = stats32(src, n)
            m_i, g_i = torch.meshgrid(torch.arange(M), torch.arange(ng), indexing="ij")
            pos = (m_i * (N // n2) + g_i) * 2
            okp = pos + 1 < o["ln_y32"].numel()
            o["ln_y32"][pos[okp]] = st[..., 0][okp]
            o["ln_y32"][pos[okp] + 1] = st[..., 1][okp]
        else:
            o["ln_y32"][:M * ng * 2] = stats32(src, n).reshape(-1)
    if c["y16"]:
        y = out[:M].to(dtype)
        if mutant == "y16_rounded_before_residual":
            y = (acc32(d["A"], d["W"], b.expand(M, N).clone(), drop).to(dtype).float() + residual_rows(c, d)).to(dtype)
        o["ln_y16"][index(c["y16"], M, N)[0].reshape(-1)] = y.reshape(-1)
    return o


# =========================================================================================================================================
# descriptors (ctypes)
# =========================================================================================================================================
def descriptor(c, dt, addr, persist=None):
    """The mra_gemm_desc of a case.  ``addr(buffer)`` -> (address of the buffer's first element, its bytes) or None; buffers A, W, bias, C, R,
    aux, ln_y32, ln_gain, ln_y16."""
    from mraudio_amd import _lib as L
    arr = (L.mra_gemm_desc * 1)()
    d = arr[0]
    d.struct_bytes = C.sizeof(L.mra_gemm_desc)
    csz = 4 if c["out_f32"] else 2
    first = {"C": c["c"]["off"] * csz, "aux": c["c"]["off"] * 2, "R": 0, "ln_y16": (c["y16"]["off"] if c["y16"] else 0) * 2}
    for b in ("A", "W", "bias", "C", "R", "aux", "ln_y32", "ln_gain", "ln_y16"):
        got = addr("C" if (b == "aux" and c["aux"] == "inplace") else b)
        if got is None or (b == "aux" and not c["aux"]):
            continue
        base, nbytes = got
        setattr(d, b, base + first.get(b, 0))
        setattr(d, {"A": "a_bytes", "W": "w_bytes", "C": "c_bytes", "R": "r_bytes"}.get(b, b + "_bytes"), nbytes - first.get(b, 0))
    d.a_view[:] = plain_lay(c["M"], c["K"])["view"]
    d.c_view[:] = c["c"]["view"]
    if c["r"]:
        d.r_view[:] = c["r"]["view"]
    if c["y16"]:
        d.ln_y16_view[:] = c["y16"]["view"]
    d.M, d.N, d.K = c["M"], c["N"], c["K"]
    d.tile_cfg = c["tile"]
    d.persist = c["persist"] if persist is None else persist
    return arr


def buffer_sizes(c, dt):
    d, o = inputs(c["name"], dt), fresh_outputs(c, dt)
    s = {k: (v.numel(), v.dtype) for k, v in d["flat"].items()}
    s.update({k: (v.numel(), v.dtype) for k, v in o.items()})
    return s


def fake_addr(c, dt):
    """Addresses for the host-only checks: every buffer at a 4 KiB boundary of its own, never dereferenced."""
    table, nxt = {}, 1 << 20
    for b, (numel, tdt) in buffer_sizes(c, dt).items():
        nbytes = numel * torch.empty(0, dtype=tdt).element_size()
        table[b] = (nxt, nbytes)
        nxt += (nbytes + 8191) // 4096 * 4096
    return lambda b: table.get(b)


# =========================================================================================================================================
# the companion kernels of the folded LayerNorm
# =========================================================================================================================================
FOLD_MUTANTS = ("cs_last_pass_dropped", "beta_times_folded_w")
GROUP_MUTANTS = ("between_group_term_dropped", "variance_over_groups_only")
ROWSTAT_MUTANTS = ("one_pass_variance", "copy_of_centred_rows")
FOLD_CASES = ((6, 384, True), (6, 384, False))            # N = 6: a full workgroup of 4 rows and a partial one
GROUP_CASES = ((300, 3, 128), (300, 22, 64))              # (M, G, columns per group)
ROWSTAT_CASES = ((5, 128), (5, 1408))                     # (M, D): a partial workgroup of 4 rows


@functools.lru_cache(maxsize=8)
def fold_case(N, K, with_bias, dt):
    return fold_inputs(N, K, DTYPES[dt], _gen(11, N, K, with_bias), with_bias)


def fold_weight_check(f, Wf, cs, bf, dtype):
    """The kernel's three outputs against float64: {key: ratio}."""
    K = f["w"].shape[1]
    wg = f["w"].double() * f["gain"].double()[None]
    r = {"Wf": ratio(Wf, wg, round_bound(wg, U32 * wg.abs(), dtype))}
    Wd = Wf.double()
    r["cs"] = ratio(cs, Wd.sum(-1), K * U32 * Wd.abs().sum(-1))
    bw = f["w"].double() * f["beta"].double()[None]
    b0 = f["bias"].double() if f["bias"] is not None else torch.zeros(f["w"].shape[0], dtype=F64)
    r["bf"] = ratio(bf, b0 + bw.sum(-1), (K + 1) * U32 * (bw.abs().sum(-1) + b0.abs()))
    return r


def fold_weight_emulate(f, dtype, mutant=None):
    wf32 = f["w"].float() * f["gain"][None]
    Wf = wf32.to(dtype)
    cs = (wf32 if mutant == "cs_from_unrounded_w" else Wf.float()[:, :-64] if mutant == "cs_last_pass_dropped" else Wf.float()).sum(-1)
    src = Wf.float() if mutant == "beta_times_folded_w" else f["w"].float()
    bf = (src * f["beta"][None]).sum(-1) + (f["bias"] if f["bias"] is not None else 0.0)
    return Wf, cs, bf


@functools.lru_cache(maxsize=4)
def group_case(M, Gn, n):
    """Rows x [M, Gn n] fp32 (means up to 30 standard deviations off, group means spread), and their groups (mean, ssd) computed in float64 and
    rounded to fp32 once."""
    g = _gen(12, M, Gn, n)
    x = torch.randn(M, Gn * n, generator=g) * (0.2 + torch.rand(M, 1, generator=g)) + 30.0 * torch.randn(M, 1, generator=g) * (torch.arange(M)[:, None] % 3 == 0)
    x = x + 0.5 * torch.randn(M, Gn, generator=g).repeat_interleave(n, 1)
    xg = x.double().view(M, Gn, n)
    a = xg.mean(-1)
    y = ((xg - a[..., None]) ** 2).sum(-1)
    return x, torch.stack([a, y], -1).float()


def group_stats_check(groups, n, eps, stats, row=None):
    """stats [M, 2] against the float64 Chan merge of ``groups`` [M, G, 2] (row = None) or against the statistics of the rows themselves."""
    Gn = groups.shape[1]
    a, y = groups[..., 0].double(), groups[..., 1].double()
    if row is None:
        mean = a.mean(-1)
        dv = a - mean[:, None]
        M2 = (y + n * dv * dv).sum(-1)
    else:
        rd = row.double()
        mean = rd.mean(-1)
        M2 = ((rd - mean[:, None]) ** 2).sum(-1)
        dv = a - mean[:, None]
    dmu = (Gn + 1) * U32 * a.abs().mean(-1)
    dM2 = n * (2 * dv.abs() * (dmu[:, None] + U32 * dv.abs()) + (dmu * dmu)[:, None]).sum(-1) + (Gn + 4) * U32 * M2
    if row is not None:
        dmu = dmu + U32 * a.abs().mean(-1)
        dM2 = dM2 + U32 * M2 + n * (2 * dv.abs() * U32 * a.abs()).sum(-1)
    r = 1.0 / torch.sqrt(M2 / (n * Gn) + eps)
    drs = r * (dM2 / (2 * (M2 + n * Gn * eps)) + (10 + Gn / 2) * U32)
    return {"mean": ratio(stats[:, 0], mean, dmu), "rstd": ratio(stats[:, 1], r, drs)}, (mean, r, dmu, drs)


def group_stats_emulate(groups, n, eps, mutant=None):
    Gn = groups.shape[1]
    a, y = groups[..., 0], groups[..., 1]
    mean = torch.zeros(a.shape[0])
    for i in range(Gn):
        mean = mean + a[:, i]
    mean = mean / Gn
    m2 = torch.zeros(a.shape[0])
    for i in range(Gn):
        dv = a[:, i] - mean
        m2 = m2 + (y[:, i] if mutant == "between_group_term_dropped" else y[:, i] + torch.tensor(float(n)) * dv * dv)
    cnt = float(Gn) if mutant == "variance_over_groups_only" else float(n) * Gn
    return torch.stack([mean, 1.0 / torch.sqrt(m2 / cnt + torch.tensor(eps, dtype=F32))], -1)


@functools.lru_cache(maxsize=8)
def rowstat_case(M, D, dt, f32):
    g = _gen(13, M, D, f32)
    x = torch.randn(M, D, generator=g) * torch.tensor([1.0, 0.05, 3.0, 1.0, 0.5])[:M, None] + torch.tensor([0.0, 20.0, -2.0, 100.0, 0.1])[:M, None]
    return x if f32 else x.to(DTYPES[dt])


def row_stats_check(x, eps, stats, x16=None, dtype=None):
    D = x.shape[1]
    dep = depth(D)
    xd = x.double()
    mean = xd.mean(-1)
    var = ((xd - mean[:, None]) ** 2).mean(-1)
    r = 1.0 / torch.sqrt(var + eps)
    dmu = (dep + 2) * U32 * xd.abs().mean(-1)
    drs = r * ((10 + dep / 2) * U32 + 0.5 * (dmu * r) ** 2)
    out = {"mean": ratio(stats[:, 0], mean, dmu), "rstd": ratio(stats[:, 1], r, drs)}
    if x16 is not None:
        out["x16 == T(x)"] = 0.0 if torch.equal(x16.view(torch.int16), x.to(dtype).view(torch.int16)) else float("inf")
    return out


def row_stats_emulate(x, eps, dtype, mutant=None):
    xf = x.float()
    D = xf.shape[1]
    mean = xf.sum(-1) / D
    dv = xf - mean[:, None]
    var = (xf * xf).sum(-1) / D - mean * mean if mutant == "one_pass_variance" else (dv * dv).sum(-1) / D
    stats = torch.stack([mean, 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=F32))], -1)
    return stats, (dv if mutant == "copy_of_centred_rows" else xf).to(dtype)


# =========================================================================================================================================
# the chain: EPI_RES_F32_STAT -> vit_group_stats -> EPI_LNF_OP (case 10)
# =========================================================================================================================================
CHAIN = dict(M=300, Kp=256, D=384, Nq=256)       # projection [M, Kp] x [D, Kp]^T + residual -> LayerNorm over D -> QKV [M, D] x [Nq, D]^T
CHAIN_MUTANTS = ("mu_not_applied", "stat_group_other_width", "beta_times_folded_w")   # (cs from the unrounded W' lies inside a bound against the UNFOLDED w: row 6 catches it)
case(10, "chain proj RES_F32_STAT M300 N384 K256", EPI_RES_F32_STAT, GT_P8_MIXED, GF_P8_MIXED, CHAIN["M"], CHAIN["D"], CHAIN["Kp"], table=False)
case(10, "chain qkv LNF_OP M300 N256 K384", EPI_LNF_OP, GT_256, GF_P8_256, CHAIN["M"], CHAIN["Nq"], CHAIN["D"], rows="chain", table=False)


@functools.lru_cache(maxsize=2)
def chain_fold(dt):
    return fold_inputs(CHAIN["Nq"], CHAIN["D"], DTYPES[dt], _gen(10, CHAIN["Nq"], CHAIN["D"]))


def chain_check(dt, Cret, x16, stat, Wf, cs, bf, out):
    """The second launch's output ``out`` [M, Nq] T against float64 LayerNorm(C returned) w^T + b.  Cret [M, D] fp32 and x16 [M, D] T from the
    first launch, stat [M, 2] from vit_group_stats, Wf / cs / bf from vit_fold_weight.  Returns the ratio."""
    dtype = DTYPES[dt]
    f = chain_fold(dt)
    D = CHAIN["D"]
    u = U[dtype]
    xd, x16d = Cret.double(), x16.double()
    m = xd.mean(-1, keepdim=True)
    var = ((xd - m) ** 2).mean(-1, keepdim=True)
    r = 1.0 / torch.sqrt(var + VIT_EPS)
    wg = f["w"].double() * f["gain"].double()[None]                       # [Nq, D]
    inner_ref = (xd - m) @ wg.T
    ref = r * inner_ref + (f["w"].double() * f["beta"].double()[None]).sum(-1)[None] + f["bias"].double()[None]
    # the statistics: the first launch's group (mean, ssd) within the group bounds (dm_g, eq_g), then the merge's own bound on top
    n, Gn = 128, D // 128
    xg = xd.view(-1, Gn, n)
    a = xg.mean(-1)
    dg = xg - a[..., None]
    y = (dg * dg).sum(-1)
    dm_g = U32 * xg.abs().sum(-1)
    eq_g = (2 * dg.abs() * dm_g[..., None] + (dm_g * dm_g)[..., None]).sum(-1) + (n + 2) * U32 * y
    di = (a - m).abs()
    M2 = (var * D)
    dmu_merge = (Gn + 1) * U32 * a.abs().mean(-1, keepdim=True)
    dmu = dm_g.mean(-1, keepdim=True) + dmu_merge
    dM2 = (eq_g + n * 2 * di * dm_g).sum(-1, keepdim=True) + n * (2 * di * (dmu_merge + U32 * di) + dmu_merge ** 2).sum(-1, keepdim=True) + (Gn + 4) * U32 * M2
    drs = r * (dM2 / (2 * (M2 + D * VIT_EPS)) + (10 + Gn / 2) * U32)
    Wd = Wf.double()
    dW = (Wd - wg).abs()
    ops = (u * xd.abs() + sub_abs(dtype)) @ wg.abs().T + x16d.abs() @ ((u + U32) * wg.abs() + sub_abs(dtype)).T
    dcs = D * U32 * Wd.abs().sum(-1)[None]
    mean_term = dmu * cs.double().abs()[None] + m.abs() * (dcs + dW.sum(-1)[None])
    acc = x16d @ Wd.T
    mcs = stat[:, 0:1].double() * cs.double()[None]
    ei = (D + 1) * U32 * (x16d.abs() @ Wd.abs().T) + U32 * (acc.abs() + mcs.abs())
    E = ops + mean_term + ei
    bw = f["w"].double() * f["beta"].double()[None]
    dbf = ((D + 1) * U32 * (bw.abs().sum(-1) + f["bias"].double().abs()))[None]
    e32 = r * E + drs * inner_ref.abs() + dbf + U32 * (ref.abs() + r * E)
    return ratio(out, ref, round_bound(ref, e32, dtype))


def chain_emulate(dt, mutant=None):
    """The three launches and vit_fold_weight in fp32: (Cret, x16, stat, Wf, cs, bf, out)."""
    dtype = DTYPES[dt]
    name = "chain proj RES_F32_STAT M300 N384 K256"
    c = BY_NAME[name]
    o = emulate(name, dt)
    M, D = CHAIN["M"], CHAIN["D"]
    Cret = o["C"][index(c["c"], M, D)[0]]
    x16 = o["ln_y16"][index(c["y16"], M, D)[0]]
    groups = o["ln_y32"][:M * (D // 128) * 2].view(M, D // 128, 2)
    if mutant == "stat_group_other_width":
        groups = stats32(Cret, 64)[:, :D // 128]
    stat = group_stats_emulate(groups, 128, VIT_EPS)
    f = chain_fold(dt)
    Wf, cs, bf = fold_weight_emulate(f, dtype, mutant if mutant == "beta_times_folded_w" else None)
    acc = acc32(x16, Wf)
    Nq = CHAIN["Nq"]
    inner = acc if mutant == "mu_not_applied" else G._fma32(-stat[:, 0:1].expand(M, Nq), cs[None].expand(M, Nq), acc)
    out = G._fma32(stat[:, 1:2].expand(M, Nq), inner, bf[None].expand(M, Nq)).to(dtype)
    return Cret, x16, stat, Wf, cs, bf, out
