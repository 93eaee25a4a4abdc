"""Shared by tests/test_train_kernel_cases_cpu.py and tests/test_gpu_train_kernels.py (not a test module): seeded inputs rounded to the
operand type, float64 references, DERIVED per-element bounds and fp32 emulations (with named mutants) for the kernels the Q-Former training
step launches besides the attention cores -- the weight-gradient GEMM (csrc/gemm_tn.hip), the LayerNorm backward, the embedding backward
and the batched weight transpose (csrc/backward.hip) and the two training epilogues of csrc/gemm.hip.  Pure torch on the CPU.

Notation as tests/qformer_kernel_cases.py: u32 = 2^-24, u = U[T] (2^-11 f16, 2^-8 bf16), ``depth(n) = ceil(n / 64) + 6`` links for a wave
reduction over n values, every bound worst case and first order, no constant fitted to GPU output (the CPU test prints how far below 1.0
the faithful emulations sit).  A sum whose order is not fixed -- the MFMA's internal order, fp32 atomics from several workgroups -- is bounded
as a sum in ANY order at one u32 per link: n terms carry (n - 1) u32 on the sum of their magnitudes.  The hardware documents read for this
suite do not state how v_mfma_f32_32x32x16 rounds inside one instruction; like the attention bounds of the forward, these bounds ASSUME it
is no worse than a chain of fp32 additions of its exact products.

---- gemm_tn: dW[n][k] (+)= sum_m dY[m][n] X[m][k], db[n] += sum_m dY[m][n] -------------------------------------------------------------
A product of two f16 values has 22 significant bits and of two bf16 values 16: exact in fp32 (no product of the inputs used here leaves the
fp32 normal range).  The contraction is cut into ``splits`` pieces (blockIdx.z), each summed in fp32 in some order and then added to the
prefilled value W0 -- in place (one piece) or by atomics (several).  M products, ``splits`` partial sums and W0 meet in M + splits links:
    |dW - ref| <= (M + splits + 1) u32 (sum_m |y x| + |W0|)           (+ 1: first order)
db is the same sum against a ones operand: (M + splits + 1) u32 (sum_m |y| + |db0|).  Without accumulate W0 = 0.

---- ln_bwd ---------------------------------------------------------------------------------------------------------------------------
dx = r (g - mean(g) - xhat mean(g xhat)) (+ add), g = dy gamma, xhat = (x - mean) r, r = (var + eps)^-1/2, D = depth(H).  The statistics are
those of the "LayerNorm family" derivation of tests/qformer_kernel_cases.py (two-pass, fl(1 / H) products):
    dm    = (D + 2) u32 mean|x|                                        error of the mean
    e_r   = (D / 2 + 7) u32 + dm^2 r^2 / 2                             relative error of r (variance (D + 4) u32 + dm^2 r^2, halved; sqrtf and
                                                                       the division 4; eps given in fp32 against the reference's 1e-12: 1)
    ex_i  = r dm + |xhat_i| (e_r + 2 u32)                              error of xhat_i (x - mean and the product with r: one rounding each)
    esg   = (D + 3) u32 mean|g|                                        mean(g): g rounded once, the wave sum, the product with fl(1 / H)
    esgx  = (D + 4) u32 mean|g xhat| + mean(|g| ex)                    mean(g xhat): one more rounding per term, and the error of xhat
    e_in  = 3 u32 |g| + 2 u32 |mean g| + 3 u32 |xhat mean(g xhat)| + esg + |xhat| esgx + ex |mean(g xhat)| + ex esgx
                                                                       g - mean(g) - xhat mean(g xhat): g's rounding, the product, two subtractions
    |dx - ref| <= r e_in + |r (g - mean g - xhat mean(g xhat))| (e_r + 2 u32) + u32 |ref|      (the product with r; the optional add)
dx16 is dx rounded once to T: bit for bit.  A one-pass variance has a relative error of order u32 mean^2 / var: 6 % at mean 1000, var 1.
Constant rows (CONSTANT_ROW values: the fp32 mean is exact in any summation order, exact_mean_rows) have dm = 0, so the computed xhat is
exactly 0 and r = 1e6 at eps = 1e-12: dx = 1e6 (g - mean g), held to r (3 u32 |g| + 2 u32 |mean g| + esg) + |dx| (e_r + 3 u32) -- with the
general dm the term r dm = 1e6 (D + 2) u32 |c| would admit anything there.
dgamma += sum_rows dy xhat, dbeta += sum_rows dy, summed over the rows in any order (registers, LDS, atomics) onto the prefilled value:
    |dgamma - ref| <= (rows + 2) u32 (sum_r |dy xhat| + |dgamma0|) + sum_r |dy| ex          (rows + 1 links, each term rounded once)
    |dbeta - ref|  <= (rows + 1) u32 (sum_r |dy| + |dbeta0|)

---- embed_bwd ------------------------------------------------------------------------------------------------------------------------
dquery[s] += sum_items demb[n][s], dpos[l] += sum_items demb[n][Q + l]: items links, items u32 (sum |g| + |prefill|).  dword[id] receives
one atomic per hit: hits u32 (sum_hits |g| + |prefill|); a row never hit keeps its bits.  ids are clamped to [0, vocab) as the forward does.

---- GELU epilogues -------------------------------------------------------------------------------------------------------------------
pre = A W^T + bias.  K exact products, the bias: eK = (K + 1) u32 (|A| |W|^T + |bias|).
erf_fast (csrc/mra_common.h) is Abramowitz & Stegun 7.1.26, |error| <= 1.5e-7 in exact arithmetic.  In fp32, with z = fl(u fl(2^-1/2)):
    the argument      2 u32 relative, |z erf'(z)| <= 0.49:                                              1 u32
    t = rcp(fma)      3 u32 relative (one fma, the hardware reciprocal 2 u32); through t poly'(t) <= sum i |a_i| = 16.2:   49 u32
    Horner            five fmas and a product on coefficients of both signs: 10 u32 sum |a_i| = 10 u32 x 4.46:           45 u32
    exp2              the argument's two roundings, ln2 z^2 e^(-z^2) 2 u32 <= 0.6 u32, the instruction 2 u32:             3 u32
    product, 1 - .                                                                                                         2 u32
E_ERF = 1.5e-7 + 100 u32 = 6.1e-6 absolute (the polynomial terms are worst at z = 0 and shrink with e^(-z^2): a constant is safe).
    gelu(u)  = u (1 + erf) / 2:    eg(u)  = |u| E_ERF / 2 + 3 u32 |gelu(u)|
    gelu'(u) = Phi(u) + u phi(u):  egp(u) = E_ERF / 2 + 8 u32         (u phi(u): five roundings and exp2 on <= 0.25, its argument's rounding
                                                                       u^3 phi(u) u32 <= 1.2 u32; Phi 2 u32; the sum 1 u32 x 1.13)
EPI_GELU_BOTH   aux = T(pre):  |aux - pre| <= eK + u (|pre| + eK) + 2^-25 [f16]
                C = T(gelu(float(aux))) of the aux RETURNED (the backward reads that tensor, so the pair must agree):
                |C - gelu(aux)| <= eg(aux) + u (|gelu(aux)| + eg(aux)) + 2^-25 [f16]
EPI_GELU_BWD    C = T(acc gelu'(aux)), acc = A W^T (K u32 |A| |W|^T = eK without a bias):
                |C - ref| <= |gelu'(aux)| eK + |acc| egp + u32 |ref|, then the rounding to T: + u (|ref| + that) + 2^-25 [f16]

---- transpose16_batch ----------------------------------------------------------------------------------------------------------------
dst = src^T, bit for bit; element values are the linear index so a misplaced tile names itself."""
import math

import torch

from qformer_kernel_cases import CONSTANT_ROW, F16_SUB, U, U32, depth, make_ln_rows, sub_abs  # noqa: F401  (re-exported for the tests)

F32 = torch.float32


def ratio(out, ref, bound) -> float:
    """max |out - ref| / bound; an element with bound 0 must be exact (0 / 0 counts 0); inf for a non-finite output."""
    d = (out.double() - ref).abs()
    if not torch.isfinite(d).all():
        return float("inf")
    r = torch.where(d == 0, torch.zeros_like(d), d / bound)
    return r.max().item() if r.numel() else 0.0


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


# =========================================================================================================================================
# gemm_tn
# =========================================================================================================================================
TN_SINGLE_M = tuple(range(33, 65)) + (1, 31, 257, 531, 645, 770)
TN_MUTANTS = ("tail_rows", "last_split_dropped", "db_every_block", "prefill_overwritten")
GROUP_N, GROUP_K, GROUP_M = (64, 128, 192, 64), (64, 192, 128, 256), (160, 45, 160, 370)


def tn_splits(M: int, N: int, K: int) -> int:
    """Pieces launch_gemm_tn cuts the contraction into (one job)."""
    tiles, nsteps = (N // 64) * (K // 64), (M + 31) // 32
    return max(1, min((512 + tiles - 1) // tiles, nsteps // 4))


def tn_group_splits(Ms, Ns, Ks) -> int:
    """The one factor launch_gemm_tn_group uses for every job of a group of two or more."""
    tiles = sum((n // 64) * (k // 64) for n, k in zip(Ns, Ks))
    return max(1, min((1024 + tiles - 1) // tiles, min((m + 31) // 32 for m in Ms) // 4))


def make_tn(M: int, N: int, K: int, dtype, seed: int = 0):
    """y [M, N], x [M, K] rounded to ``dtype``; W0 [N, K], db0 [N] fp32 prefills of clearly non-zero size."""
    g = _gen(M, N, K, seed, 1)
    y = (torch.randn(M, N, generator=g) * 0.5).to(dtype)
    x = torch.randn(M, K, generator=g).to(dtype)
    W0 = torch.randn(N, K, generator=g) * 3.0
    db0 = torch.randn(N, generator=g) * 3.0
    return y, x, W0, db0


def tn_ref(y, x, W0, db0, splits: int):
    """(dW float64, bound, db float64, bound); W0 / db0 None = zero."""
    M = y.shape[0]
    yd, xd = y.double(), x.double()
    w0 = torch.zeros(y.shape[1], x.shape[1], dtype=torch.float64) if W0 is None else W0.double()
    b0 = torch.zeros(y.shape[1], dtype=torch.float64) if db0 is None else db0.double()
    c = (M + splits + 1) * U32
    return w0 + yd.T @ xd, c * (yd.abs().T @ xd.abs() + w0.abs()), b0 + yd.sum(0), c * (yd.abs().sum(0) + b0.abs())


def tn_emulate(y, x, W0, db0, splits: int, mutant=None):
    """fp32: per piece of ceil(steps / splits) 32-row steps a partial product, added to the prefill one after the other.  Returns (dW, db)."""
    M, N = y.shape
    K = x.shape[1]
    yf, xf = y.float(), x.float()
    if mutant == "tail_rows":          # the rows past M re-read row M - 1 and are not zeroed
        pad = (-M) % 32
        yf, xf = torch.cat([yf, yf[-1:].expand(pad, -1)]), torch.cat([xf, xf[-1:].expand(pad, -1)])
    W = torch.zeros(N, K) if (W0 is None or mutant == "prefill_overwritten") else W0.clone()
    db = torch.zeros(N) if db0 is None else db0.clone()
    nsteps = (M + 31) // 32
    per = (nsteps + splits - 1) // splits
    pieces = [(s * per * 32, min(nsteps, (s + 1) * per) * 32) for s in range(splits) if s * per < nsteps]
    if mutant == "last_split_dropped" and len(pieces) > 1:
        pieces = pieces[:-1]
    for m0, m1 in pieces:
        W = W + yf[m0:m1].T @ xf[m0:m1]
        db = db + yf[m0:m1].sum(0) * (K // 64 if mutant == "db_every_block" else 1)
    return W, db


# =========================================================================================================================================
# ln_bwd
# =========================================================================================================================================
LNB_H = (256, 512, 768, 1024)
LNB_ROWS = (1, 3, 4, 5, 15, 16, 17, 33, 70)
LNB_FAMILIES = ("normal", "offset1000", "outlier", "constant")
LNB_MUTANTS = ("one_pass", "no_mean_g", "dgamma_raw_x", "tail_in_dgamma", "b_uses_a_gamma")
LNB_EPS = 1e-12


def make_lnb(kind: str, rows: int, H: int, seed: int = 0):
    """dict of fp32 tensors: x (the family), dy, add [rows, H]; gamma [H] with zeros (every 7th) and negative entries; dgamma0, dbeta0 [H]."""
    g = _gen(rows, H, seed, sum(map(ord, kind)))
    gamma = torch.randn(H, generator=g)
    gamma[::7] = 0.0
    gamma[1::11] = -gamma[1::11].abs() - 0.5
    return dict(x=make_ln_rows(kind, rows, H, seed=seed) if rows else torch.zeros(0, H), dy=torch.randn(rows, H, generator=g),
                add=torch.randn(rows, H, generator=g) * 2.0, gamma=gamma, dgamma0=torch.randn(H, generator=g) * 5.0,
                dbeta0=torch.randn(H, generator=g) * 5.0)


def exact_mean_rows(x):
    """[rows, 1] bool: rows that hold one CONSTANT_ROW value throughout.  Every partial sum k c (k <= 1024, c of at most three significant
    bits) is exact in fp32 in any order and fl(fl(H c) fl(1 / H)) = c (asserted on the CPU for every width): the computed mean is c, so
    dm = 0, the computed xhat is exactly 0 and the bound keeps no r dm term on these rows."""
    c = x[:, :1]
    return (x == c).all(-1, keepdim=True) & torch.isin(c, torch.tensor(CONSTANT_ROW))


def lnb_ref(x, dy, gamma, eps: float, add=None, dgamma0=None, dbeta0=None):
    """float64: (dx, dx_bound, dgamma, dgamma_bound, dbeta, dbeta_bound); the prefills default to zero."""
    rows, H = x.shape
    D = depth(H)
    xd, dyd, gd = x.double(), dy.double(), gamma.double()
    mean = xd.mean(-1, keepdim=True)
    d = xd - mean
    r = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)
    xh = d * r
    g = dyd * gd
    mg, mgx = g.mean(-1, keepdim=True), (g * xh).mean(-1, keepdim=True)
    inner = g - mg - xh * mgx
    dx = r * inner + (add.double() if add is not None else 0.0)
    dm = (D + 2) * U32 * xd.abs().mean(-1, keepdim=True)
    dm = torch.where(exact_mean_rows(x), torch.zeros_like(dm), dm)
    e_r = (D / 2 + 7) * U32 + 0.5 * (dm * r) ** 2
    ex = r * dm + xh.abs() * (e_r + 2 * U32)
    esg = (D + 3) * U32 * g.abs().mean(-1, keepdim=True)
    esgx = (D + 4) * U32 * (g * xh).abs().mean(-1, keepdim=True) + (g.abs() * ex).mean(-1, keepdim=True)
    e_in = U32 * (3 * g.abs() + 2 * mg.abs() + 3 * (xh * mgx).abs()) + esg + xh.abs() * esgx + ex * mgx.abs() + ex * esgx
    dx_bound = r * e_in + (r * inner).abs() * (e_r + 2 * U32) + U32 * dx.abs()
    g0 = dgamma0.double() if dgamma0 is not None else torch.zeros(H, dtype=torch.float64)
    b0 = dbeta0.double() if dbeta0 is not None else torch.zeros(H, dtype=torch.float64)
    dgamma = g0 + (dyd * xh).sum(0)
    dg_bound = (rows + 2) * U32 * ((dyd * xh).abs().sum(0) + g0.abs()) + (dyd.abs() * ex).sum(0)
    dbeta = b0 + dyd.sum(0)
    db_bound = (rows + 1) * U32 * (dyd.abs().sum(0) + b0.abs())
    return dx, dx_bound, dgamma, dg_bound, dbeta, db_bound


def lnb_emulate(x, dy, gamma, eps: float, add=None, dgamma0=None, dbeta0=None, mutant=None):
    """ln_bwd_kernel's fp32 arithmetic (torch's fp32 sums stand in for the wave sums and the atomics).  Returns (dx, dgamma, dbeta)."""
    rows, H = x.shape
    inv_h = torch.tensor(1.0 / H, dtype=F32)
    mean = x.sum(-1, keepdim=True) * inv_h
    d = x - mean
    if mutant == "one_pass":
        var = (x * x).sum(-1, keepdim=True) * inv_h - mean * mean
    else:
        var = (d * d).sum(-1, keepdim=True) * inv_h
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=F32))
    xh = d * rstd
    g = dy * gamma
    sg = g.sum(-1, keepdim=True) * inv_h
    sgx = (g * xh).sum(-1, keepdim=True) * inv_h
    if mutant == "no_mean_g":
        sg = torch.zeros_like(sg)
    dx = rstd * (g - sg - xh * sgx)
    if add is not None:
        dx = dx + add
    tg = dy * (x if mutant == "dgamma_raw_x" else xh)
    tb = dy
    if mutant == "tail_in_dgamma" and rows % 4:     # the wave holding the last row counts its clamped re-reads of that row
        pad = 4 - rows % 4
        tg, tb = torch.cat([tg, tg[-1:].expand(pad, -1)]), torch.cat([tb, tb[-1:].expand(pad, -1)])
    dgamma = tg.sum(0) + (dgamma0 if dgamma0 is not None else 0.0)
    dbeta = tb.sum(0) + (dbeta0 if dbeta0 is not None else 0.0)
    return dx, dgamma, dbeta


# =========================================================================================================================================
# embed_bwd
# =========================================================================================================================================
EMB_CASES = ((3, 4, 32, 256, 10), (1, 1, 32, 768, 5), (5, 7, 32, 1024, 3), (2, 0, 32, 768, 10))   # items, L, Q, H, vocab
EMB_MUTANTS = ("no_clamp", "pos_off_by_q", "word_overwrite")


def make_emb(items: int, L: int, Q: int, H: int, vocab: int, seed: int = 0):
    """demb [items, Q + L, H]; ids [items, L] with -1 and ``vocab`` among them and repeats within and across items (the first column of
    every item is id 1 % vocab, the last two of an item are equal); dquery0 [Q, H], dpos0 [L, H], dword0 [vocab, H] prefills."""
    g = _gen(items, L, Q, H, vocab, seed)
    demb = torch.randn(items, Q + L, H, generator=g)
    ids = torch.randint(0, vocab, (items, L), generator=g)
    if L:
        ids[:, 0] = 1 % vocab
        flat = ids.view(-1)
        if flat.numel() >= 4:
            flat[1] = -1
            flat[2] = vocab
        else:
            flat[0] = vocab          # the single id of the (1, 1, ...) case: clamped to vocab - 1
        if L >= 3:
            ids[:, -1] = ids[:, -2]
    return dict(demb=demb, ids=ids, dquery0=torch.randn(Q, H, generator=g) * 3.0, dpos0=torch.randn(L, H, generator=g) * 3.0,
                dword0=torch.randn(vocab, H, generator=g) * 3.0)


def emb_ref(demb, ids, Q: int, vocab: int, dquery0=None, dpos0=None, dword0=None):
    """float64 (dquery, bound, dpos, bound, dword, bound, hit [vocab] bool); a NULL prefill counts as zero."""
    items, S, H = demb.shape
    L = S - Q
    dd = demb.double()
    z = lambda t, n: t.double() if t is not None else torch.zeros(n, H, dtype=torch.float64)   # noqa: E731
    q0, p0, w0 = z(dquery0, Q), z(dpos0, L), z(dword0, vocab)
    dq, dq_b = q0 + dd[:, :Q].sum(0), items * U32 * (dd[:, :Q].abs().sum(0) + q0.abs())
    dp, dp_b = p0 + dd[:, Q:].sum(0), items * U32 * (dd[:, Q:].abs().sum(0) + p0.abs())
    idx = ids.clamp(0, vocab - 1).reshape(-1)
    hits = torch.bincount(idx, minlength=vocab).double()
    rowsum = torch.zeros(vocab, H, dtype=torch.float64).index_add_(0, idx, dd[:, Q:].reshape(-1, H))
    rowabs = torch.zeros(vocab, H, dtype=torch.float64).index_add_(0, idx, dd[:, Q:].abs().reshape(-1, H))
    dw, dw_b = w0 + rowsum, hits[:, None] * U32 * (rowabs + w0.abs())
    return dq, dq_b, dp, dp_b, dw, dw_b, hits > 0


def emb_emulate(demb, ids, Q: int, vocab: int, dquery0, dpos0, dword0, mutant=None):
    items, S, H = demb.shape
    L = S - Q
    dq = dquery0 + demb[:, :Q].sum(0)
    dp = dpos0 + (demb[:, :L] if mutant == "pos_off_by_q" else demb[:, Q:]).sum(0)
    dw = dword0.clone()
    for n in range(items):
        for l in range(L):
            i = int(ids[n, l])
            if mutant == "no_clamp":
                if not 0 <= i < vocab:
                    continue                 # an unclamped id lands outside the table
            else:
                i = min(max(i, 0), vocab - 1)
            dw[i] = (dword0[i] if mutant == "word_overwrite" else dw[i]) + demb[n, Q + l]
    return dq, dp, dw


# =========================================================================================================================================
# GELU epilogues
# =========================================================================================================================================
E_ERF = 1.5e-7 + 100 * U32
GELU_MUTANTS = ("no_u_phi", "c_from_unrounded")
GELU_EDGE_COLS = 8      # the first columns of every problem carry biases (or pre-activations) spread over [-8, 8]


def make_gelu(M: int, N: int, K: int, dtype, seed: int = 0, with_bias: bool = True):
    """A [M, K], W [N, K] in ``dtype`` (W ~ N(0, 1 / K): sums of order 1), bias fp32 [N] or None; the first GELU_EDGE_COLS biases are -8 .. 8
    in equal steps, so the pre-activations there reach |u| = 8 while the GEMM sums stay small.  aux [M, N] in ``dtype`` for the backward:
    N(0, 2) with the same columns offset by -8 .. 8."""
    g = _gen(M, N, K, seed, 3)
    A = torch.randn(M, K, generator=g).to(dtype)
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dtype)
    edge = torch.linspace(-8.0, 8.0, GELU_EDGE_COLS)
    bias = None
    if with_bias:
        bias = torch.randn(N, generator=g) * 0.5
        bias[:GELU_EDGE_COLS] = edge
    aux = torch.randn(M, N, generator=g) * 2.0
    aux[:, :GELU_EDGE_COLS] = aux[:, :GELU_EDGE_COLS] * 0.05 + edge
    return A, W, bias, aux.to(dtype)


def _phi(u):
    return torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


def gelu64(u):
    return 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))


def gelu_grad64(u):
    return 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0))) + u * _phi(u)


def gelu_both_ref(A, W, bias):
    """(pre float64, aux bound): what EPI_GELU_BOTH's aux is held against."""
    dtype = A.dtype
    K = A.shape[1]
    b = bias.double() if bias is not None else torch.zeros(W.shape[0], dtype=torch.float64)
    pre = A.double() @ W.double().T + b
    eK = (K + 1) * U32 * (A.double().abs() @ W.double().abs().T + b.abs())
    return pre, eK + U[dtype] * (pre.abs() + eK) + sub_abs(dtype)


def gelu_of_aux_ref(aux):
    """(gelu(aux) float64, bound) for the aux tensor as RETURNED (operand dtype)."""
    dtype = aux.dtype
    a = aux.double()
    ref = gelu64(a)
    eg = 0.5 * a.abs() * E_ERF + 3 * U32 * ref.abs()
    return ref, eg + U[dtype] * (ref.abs() + eg) + sub_abs(dtype)


def gelu_bwd_ref(A, W, aux):
    """EPI_GELU_BWD without a bias: (C float64, bound)."""
    dtype = A.dtype
    K = A.shape[1]
    acc = A.double() @ W.double().T
    eK = (K + 1) * U32 * (A.double().abs() @ W.double().abs().T)
    gp = gelu_grad64(aux.double())
    ref = acc * gp
    e32 = gp.abs() * eK + acc.abs() * (0.5 * E_ERF + 8 * U32) + U32 * ref.abs()
    return ref, e32 + U[dtype] * (ref.abs() + e32) + sub_abs(dtype)


def _erf_fast(x):
    """csrc/mra_common.h erf_fast in fp32."""
    ax = x.abs()
    t = 1.0 / (ax * torch.tensor(0.3275911, dtype=F32) + 1.0)
    c = [torch.tensor(v, dtype=F32) for v in (1.061405429, -1.453152027, 1.421413741, -0.284496736, 0.254829592)]
    poly = t * (t * (t * (t * (t * c[0] + c[1]) + c[2]) + c[3]) + c[4])
    r = 1.0 - poly * torch.exp2(torch.tensor(-1.4426950408889634, dtype=F32) * ax * ax)
    return torch.copysign(r, x)


RSQRT2 = torch.tensor(0.70710678118654752440, dtype=F32)


def gelu_emulate(u32):
    return 0.5 * u32 * (1.0 + _erf_fast(u32 * RSQRT2))


def gelu_grad_emulate(u32, mutant=None):
    big = 0.5 * (1.0 + _erf_fast(u32 * RSQRT2))
    if mutant == "no_u_phi":
        return big
    return big + u32 * torch.tensor(0.39894228040143267794, dtype=F32) * torch.exp2(torch.tensor(-0.72134752044448170368, dtype=F32) * u32 * u32)


def gelu_both_emulate(A, W, bias, mutant=None):
    """(aux, C) in the operand dtype."""
    dtype = A.dtype
    pre = A.float() @ W.float().T + (bias if bias is not None else 0.0)
    aux = pre.to(dtype)
    return aux, gelu_emulate(pre if mutant == "c_from_unrounded" else aux.float()).to(dtype)


def gelu_bwd_emulate(A, W, aux, mutant=None):
    return ((A.float() @ W.float().T) * gelu_grad_emulate(aux.float(), mutant)).to(A.dtype)


# =========================================================================================================================================
# transpose16_batch
# =========================================================================================================================================
TR_SHAPES = ((64, 64), (96, 32), (32, 96), (70, 45), (33, 1), (1, 33), (192, 64))
TR_NJOBS = (1, 2, 3, 5, 8)
TR_MUTANTS = ("prev_tiles_x",)


def tr_shapes(njobs: int):
    """The matrices of a launch of ``njobs`` jobs: TR_SHAPES in order from entry ``njobs`` on, so every shape is used and neighbours differ
    in their tile counts."""
    return [TR_SHAPES[(njobs + j) % len(TR_SHAPES)] for j in range(njobs)]


def make_tr(R: int, C: int, dtype, job: int = 0):
    """[R, C]: the linear index (+ 1 + job) as an integer bit pattern of the 16-bit type -- every element of a matrix is distinct."""
    return (torch.arange(R * C, dtype=torch.int32) + 1 + job).to(torch.int16).view(dtype).view(R, C)


def tr_emulate(srcs, mutant=None):
    """The kernel's tile walk: job j owns tiles_x(j) * tiles_y(j) workgroups; tile ``local`` sits at column block local % tiles_x and row
    block local / tiles_x.  Destinations start as -1 bit patterns, as the GPU test's sentinel."""
    outs = []
    tx_of = [(s.shape[1] + 31) // 32 for s in srcs]
    for j, s in enumerate(srcs):
        R, C = s.shape
        si = s.view(torch.int16)
        out = torch.full((C, R), -1, dtype=torch.int16)
        tx = tx_of[j - 1] if (mutant == "prev_tiles_x" and j > 0) else tx_of[j]
        for local in range(tx_of[j] * ((R + 31) // 32)):
            bx, by = (local % tx) * 32, (local // tx) * 32
            if by < R and bx < C:
                out[bx:bx + 32, by:by + 32] = si[by:by + 32, bx:bx + 32].T
        outs.append(out.view(s.dtype))
    return outs


# =========================================================================================================================================
# host arrays of the mra_debug_* entries (ctypes only: shared by the refusal checks on the CPU and the launches on the GPU)
# =========================================================================================================================================
import ctypes as C  # noqa: E402


def c_ptrs(ps):
    """HOST array of pointers; an entry is an int address, a ctypes buffer, an object with ``.ptr`` (c_void_p) or None."""
    def addr(p):
        if p is None:
            return None
        if isinstance(p, int):
            return p
        if hasattr(p, "ptr"):
            return p.ptr.value
        return C.addressof(p)
    return (C.c_void_p * len(ps))(*[addr(p) for p in ps])


def c_views(vs):
    """HOST array of row views, three int64 each; None stands for an unused view."""
    flat = []
    for v in vs:
        flat += list(v) if v is not None else [0, 1, 8]
    return (C.c_int64 * len(flat))(*flat)


def c_i64(xs):
    return (C.c_int64 * len(xs))(*xs)


def c_i32(xs):
    return (C.c_int32 * len(xs))(*xs)
