"""Shared by tests/test_raw_scores_cases_cpu.py and tests/test_gpu_raw_features.py (not a test module): the scores launch of the folded
cross-attention over RAW encoder tokens (csrc/gemm.hip, gemm_ws_kernel with CS = 2: GemmProb::col_scale + col_stats) as a case table with
seeded inputs rounded to the operand type, float64 references and derived bounds, in the style of tests/gemm_cases.py (whose helpers and
notation -- u32 = 2^-24, u = U[T], ratio = worst |d| / bound -- it reuses).  Pure torch / numpy on the CPU.

The launch:  acc = A W^T (A = Q'' [M][K], W = the raw token rows [N][K], batch entries one after the other);  r_n = 1 / sqrt(var_n + eps),
the biased variance of token row n over K;  stat_m = fl(alpha max_n fl(r_n acc));  p = exp2(fma(fl(r_n acc), alpha, -stat_m));
C = T(p r_n);  stat_l = the fp32 sum of p over the tile's valid columns;  col_scale[b][n] = r_n for n < N.

---- r_n ------------------------------------------------------------------------------------------------------------------------------------
The kernel never forms E[x^2] - mean^2.  The loader lane that staged 16-byte chunk c of a token row accumulates, per K step, the chunk's
mean and centred sum of squares and merges it into its running pair (Chan et al.); the eight lanes of a row then merge pairwise by lane swaps
(1, 2, 4).  ``r_emulate`` replays exactly that order in numpy fp32 (lane j of row n holds logical chunk j ^ ((n >> 1) & 7) of every K step --
the staging swizzle).
A chunk mean carries an error of a few u32 |mean|, so the between-chunk part of M2 errs by about u32 |mean| / sigma relative: the result is
exact to a few u32 at |mean| << sigma and to ~10 u32 at |mean| / sigma ~ 100 -- the first-order WORST case (every rounding of a chunk sum and
of the running mean pushing one way: 16 u32 (|mean| + 4 sigma) / sigma on r, by Cauchy-Schwarz over the merge weights) is two orders above
what any order of additions shows on real rows, and useless as a bar.  The compiler may contract a multiply-add that the emulation rounds
twice and the device's division and square root are good to ~1 ulp rather than correctly rounded, so the device need not match the
emulation bit for bit.  The bar is therefore the emulation's own worst error with a STATED MARGIN:
    r_bar() = R_MARGIN x (worst relative error of r_emulate against float64 over every case and batch entry),  R_MARGIN = 4
(about 33 u32 = 2e-6 here).  tests/test_raw_scores_cases_cpu.py holds it between 4 u32 and the worst-case figure above, and shows that the
E[x^2] - mean^2 form in fp32 misses it on the same rows by three orders of magnitude.  Token rows have means from -6 to 6 and standard
deviations from 0.05 to 8 (|mean| / sigma up to 120), rounded to T before anything is computed from them.

---- the three stages, each against the kernel's own previous stage (gemm_cases.softpart_check with r) ----------------------------------------
    s' = r s with the r RETURNED: the accumulator errs by eK = (K + 1) u32 |A| |W|^T, the product rounds once: eK' = r eK + u32 |s'|
    stat_m   |stat_m - alpha max_n s'| <= alpha max_n eK' + u32 |stat_m|
    C        y = alpha s' - stat_m (the stat_m RETURNED), d = alpha eK' + u32 |y|, e32 = 2^y (ln2 d + 2 u32) + 2^-126;
             |C - 2^y r| <= round_bound(2^y r, r e32 + u32 2^y r, T)                                   (one more fp32 product, then T)
    stat_l   |stat_l - sum_n 2^y| <= sum_n e32 + 176 u32 sum_n 2^y                                      (the exponentials themselves, unrounded)
    columns N .. end of the last tile of C are exact zeros and not in stat_l."""
import functools
import itertools
import math

import numpy as np
import torch

from gemm_cases import ALPHA, C_PAD, DTYPES, F32, F64, U32, fold_kvp, ratio, round_bound, sentinel  # noqa: F401  (re-exported)

EPS = 1e-5            # enc_ln_eps of the forward
R_MARGIN = 4.0        # r_bar() = R_MARGIN x the emulation's worst relative error (see above)
TILE = 176
BATCH = 2

# every combination the launch can differ in: full / short row tile, one exact tile / a ragged second tile, an even / odd number of K steps
# (both LDS buffers as the last one), mild / peaked scores (part of a peaked row underflows in f16)
CASES = [dict(name=f"m{M}_kv{kv}_k{K}_{kind}", M=M, N=kv, K=K, kind=kind, batch=BATCH)
         for M, kv, K, kind in itertools.product((384, 200), (176, 216), (128, 192), ("mild", "peaked"))]
BY_NAME = {c["name"]: c for c in CASES}


def ntiles(c):
    return (c["N"] + TILE - 1) // TILE


def _gen(c):
    return torch.Generator().manual_seed(7919 * c["M"] + 104729 * c["N"] + 1299709 * c["K"] + (17 if c["kind"] == "mild" else 23))


@functools.lru_cache(maxsize=4)
def inputs(name: str, dt: str):
    """A [B, M, K] (centred rows: what Q'' = Q_h W_k' is), W [B, N, K] raw token rows, both rounded to T."""
    c = BY_NAME[name]
    dtype = DTYPES[dt]
    g = _gen(c)
    B, M, N, K = c["batch"], c["M"], c["N"], c["K"]
    mean = torch.linspace(-6.0, 6.0, N)[torch.randperm(N, generator=g)]
    std = torch.logspace(math.log10(0.05), math.log10(8.0), N)[torch.randperm(N, generator=g)]
    W = (mean[None, :, None] + std[None, :, None] * torch.randn(B, N, K, generator=g)).to(dtype)
    A = torch.randn(B, M, K, generator=g)
    A = (A - A.mean(-1, keepdim=True)) * ((8.0 if c["kind"] == "mild" else 80.0) / math.sqrt(K))   # alpha r s of order 1.4 / 14
    return dict(A=A.to(dtype), W=W, mean=mean, std=std)


@functools.lru_cache(maxsize=4)
def reference(name: str, dt: str):
    """float64 of the rounded operands: s [B, M, N], eK, r [B, N]."""
    c = BY_NAME[name]
    d = inputs(name, dt)
    Ad, Wd = d["A"].double(), d["W"].double()
    s = Ad @ Wd.transpose(1, 2)
    eK = (c["K"] + 1) * U32 * (Ad.abs() @ Wd.abs().transpose(1, 2))
    var = Wd.var(-1, unbiased=False)
    return dict(s=s, eK=eK, r=1.0 / torch.sqrt(var + EPS), var=var, mean=Wd.mean(-1))


def fresh_outputs(c, dt):
    """Flat output buffers, all-ones bits: C [B][M][ld] with ld = fold_kvp(N) (the forward's row stride), stat_m / stat_l [B M ntiles] + pad,
    col_scale [B][ld] + pad."""
    B, M, ld = c["batch"], c["M"], fold_kvp(c["N"])
    n = B * M * ntiles(c) + C_PAD
    return dict(C=sentinel(B * M * ld, DTYPES[dt]), stat_m=sentinel(n, F32), stat_l=sentinel(n, F32), col_scale=sentinel(B * ld + C_PAD, F32))


def r_error(ref, r_out):
    """worst relative error of r_out [B, N] against the float64 reference."""
    return float(((r_out.double() - ref["r"]).abs() / ref["r"]).max())


@functools.lru_cache(maxsize=2)
def r_bar(dt: str = "f16"):
    """The relative bound on r_n: R_MARGIN x the worst error of the fp32 emulation of the kernel's merge order over every case."""
    worst = 0.0
    for c in CASES:
        W = inputs(c["name"], dt)["W"]
        worst = max(worst, r_error(reference(c["name"], dt), torch.stack([r_emulate(W[b]) for b in range(c["batch"])])))
    return R_MARGIN * worst


def r_ratio(c, ref, r_out, dt="f16"):
    """worst |r - r_ref| / (r_bar r_ref); r_out [B, N]."""
    return r_error(ref, r_out) / r_bar(dt)


def check(name: str, dt: str, outs):
    """outs as fresh_outputs after the launch.  Returns (ratios, failures)."""
    c = BY_NAME[name]
    dtype = DTYPES[dt]
    ref = reference(name, dt)
    B, M, N, ld, nt = c["batch"], c["M"], c["N"], fold_kvp(c["N"]), ntiles(c)
    ratios, fails = {}, []

    def note(key, v):
        ratios[key] = v
        if not v <= 1.0:
            fails.append(f"{key}: |d| / bound = {v:.4g}")

    # ownership: C columns [0, nt * 176) of every row, the statistics, col_scale[b][:N]; everything else still all-ones bits
    def untouched(t):
        return t.view({2: torch.int16, 4: torch.int32}[t.element_size()]) == -1
    Cm = outs["C"].view(B, M, ld)
    cs = outs["col_scale"][:B * ld].view(B, ld)
    for what, written, rest in (("C", Cm[:, :, :nt * TILE], Cm[:, :, nt * TILE:]), ("col_scale", cs[:, :N], cs[:, N:]),
                                ("stat_m", outs["stat_m"][:B * M * nt], outs["stat_m"][B * M * nt:]),
                                ("stat_l", outs["stat_l"][:B * M * nt], outs["stat_l"][B * M * nt:]),
                                ("col_scale pad", cs[:, :0], outs["col_scale"][B * ld:])):
        if untouched(written).any():
            fails.append(f"{what}: {int(untouched(written).sum())} owned elements left unwritten")
        if not untouched(rest).all():
            fails.append(f"{what}: {int((~untouched(rest)).sum())} elements written outside the owned region")
    r_out = cs[:, :N]
    note("r", r_ratio(c, ref, r_out, dt))
    # the stages, with the r returned
    a = float(torch.tensor(ALPHA, dtype=F32).double())
    pad = nt * TILE - N
    rd = r_out.double()[:, None, :]
    s1 = ref["s"] * rd
    e1 = ref["eK"] * rd + U32 * s1.abs()
    s1 = torch.nn.functional.pad(s1, (0, pad), value=-float("inf")).view(B, M, nt, TILE)
    e1 = torch.nn.functional.pad(e1, (0, pad), value=0.0).view(B, M, nt, TILE)
    rt = torch.nn.functional.pad(rd.expand(B, M, N), (0, pad), value=0.0).view(B, M, nt, TILE)
    sm = outs["stat_m"][:B * M * nt].view(B, M, nt)
    sl = outs["stat_l"][:B * M * nt].view(B, M, nt)
    smd = sm.double()
    note("stat_m", ratio(sm, a * s1.amax(-1), a * e1.amax(-1) + U32 * smd.abs()))
    y = a * s1 - smd[..., None]
    p_ref = torch.exp2(y)
    dlt = a * e1 + U32 * y.abs().nan_to_num(posinf=0.0)
    e32 = p_ref * (math.log(2.0) * dlt + 2 * U32) + 2.0 ** -126
    valid = (torch.arange(nt * TILE) < N).view(nt, TILE)
    e32 = torch.where(valid, e32, torch.zeros_like(e32))
    c_ref = p_ref * rt
    cb = torch.where(valid, round_bound(c_ref, rt * e32 + U32 * c_ref, dtype), torch.zeros_like(c_ref))
    note("C", ratio(Cm[:, :, :nt * TILE].reshape(B, M, nt, TILE), c_ref, cb))
    tot = p_ref.sum(-1)
    note("stat_l", ratio(sl, tot, e32.sum(-1) + TILE * U32 * tot))
    return ratios, fails


# =========================================================================================================================================
# fp32 emulations
# =========================================================================================================================================
def _f(x):
    return np.asarray(x, dtype=np.float32)


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def r_emulate(W, eps=EPS):
    """W [rows, K] (T) -> r [rows] fp32 in the kernel's merge order (module docstring)."""
    x = W.float().numpy()
    rows, K = x.shape
    nk = K // 64
    lane_chunk = (np.arange(8)[None, :] ^ ((np.arange(rows)[:, None] >> 1) & 7))          # [rows, 8 lanes] -> logical chunk
    mean = np.zeros((rows, 8), np.float32)
    m2 = np.zeros((rows, 8), np.float32)
    for kt in range(nk):
        idx = kt * 64 + lane_chunk[:, :, None] * 8 + np.arange(8)[None, None, :]
        v = np.take_along_axis(x[:, None, :].repeat(8, 1), idx, axis=2)                    # [rows, 8, 8]
        s = np.zeros((rows, 8), np.float32)
        for e in range(8):
            s = s + v[:, :, e]
        m8 = s * _f(0.125)
        q8 = np.zeros((rows, 8), np.float32)
        for e in range(8):
            dd = v[:, :, e] - m8
            q8 = _fma(dd, dd, q8)
        fk = _f(1.0) / _f(kt + 1)
        fq = _f(8.0) * _f(kt) * fk
        dl = m8 - mean
        mean = _fma(dl, np.broadcast_to(fk, dl.shape), mean)
        m2 = (m2 + q8) + (dl * dl) * fq
    cnt = _f(8.0 * nk)
    for sw in (1, 2, 4):
        om, oq = mean[:, np.arange(8) ^ sw], m2[:, np.arange(8) ^ sw]
        dl = om - mean
        mean = _fma(dl, np.broadcast_to(_f(0.5), dl.shape), mean)
        m2 = (m2 + oq) + (dl * dl) * (_f(0.5) * cnt)
        cnt = cnt * _f(2.0)
    var = m2[:, 0] / cnt + _f(eps)
    return torch.from_numpy(_f(1.0) / np.sqrt(var, dtype=np.float32))


def r_naive(W, eps=EPS):
    """The formulation the kernel avoids: fp32 sums of x and x^2 (sequential), var = E[x^2] - mean^2."""
    x = W.float().numpy()
    rows, K = x.shape
    s = np.zeros(rows, np.float32)
    q = np.zeros(rows, np.float32)
    for k in range(K):
        s = s + x[:, k]
        q = _fma(x[:, k], x[:, k], q)
    mean = s / _f(K)
    var = q / _f(K) - mean * mean
    with np.errstate(invalid="ignore", divide="ignore"):
        return torch.from_numpy(_f(1.0) / np.sqrt(var + _f(eps), dtype=np.float32))


def emulate(name: str, dt: str, r=None):
    """The launch in fp32 on the CPU (float64 accumulator rounded once: inside the accumulator bound): buffers as fresh_outputs."""
    c = BY_NAME[name]
    dtype = DTYPES[dt]
    d = inputs(name, dt)
    B, M, N, ld, nt = c["batch"], c["M"], c["N"], fold_kvp(c["N"]), ntiles(c)
    o = fresh_outputs(c, dt)
    if r is None:
        r = torch.stack([r_emulate(d["W"][b]) for b in range(B)])
    acc = (d["A"].double() @ d["W"].double().transpose(1, 2)).float()
    v = acc * r[:, None, :]
    pad = nt * TILE - N
    vt = torch.nn.functional.pad(v, (0, pad), value=-float("inf")).view(B, M, nt, TILE)
    sm = vt.amax(-1) * torch.tensor(ALPHA, dtype=F32)
    y = (vt.double() * float(torch.tensor(ALPHA, dtype=F32).double()) - sm.double()[..., None]).float()
    p = torch.exp2(y)
    rt = torch.nn.functional.pad(r[:, None, :].expand(B, M, N), (0, pad), value=0.0).view(B, M, nt, TILE)
    Cm = o["C"].view(B, M, ld)
    Cm[:, :, :nt * TILE] = (p * rt).to(dtype).view(B, M, nt * TILE)
    o["stat_m"][:B * M * nt] = sm.reshape(-1)
    o["stat_l"][:B * M * nt] = p.sum(-1).reshape(-1)
    o["col_scale"][:B * ld].view(B, ld)[:, :N] = r
    return o
