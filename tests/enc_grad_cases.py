"""Shared by tests/test_enc_grad_cases_cpu.py and tests/test_gpu_enc_grad.py (not a test module): seeded inputs rounded to the operand type,
float64 references, DERIVED per-element bounds and fp32 emulations (with named mutants) for the two kernels of csrc/enc_grad.hip -- the
encoder-side data gradient of the cross K / V projections and the backward of the modality LayerNorm.  Pure torch on the CPU.  Conventions
and notation as tests/train_kernel_cases.py (u32 = 2^-24, every bound worst case and first order, nothing fitted to GPU output).

---- kvgrad GEMM: d_enc[m][e] = sum_k dKV[m][k] W_kv[k][e] ------------------------------------------------------------------------------
m = item * kv + tok over Ne * kv rows, k = (cl * 2 + sel) * hidden + head * 64 + d over K = ncross * 2 * hidden.  The A operand is the
head-major dK / dV tape [ncross * 2][Ne][heads][kv][64]: the 64-wide K step s = k / 64 of row m is the 64 elements at
(((s / heads) * Ne + item) * heads + s % heads) * kv * 64 + tok * 64.  A product of two f16 values has 22 significant bits and of two bf16
values 16: exact in fp32.  K exact products are summed in some order (the MFMA's, assumed no worse than a chain of fp32 additions):
    |d_enc - ref| <= (K + 1) u32 sum_k |dKV W|            (K - 1 links, + 2: first order), against float64 of the rounded operands.
The emulation walks the cache with the kernel's address arithmetic (tiles of 128 rows, one 64-wide step at a time), so the mutants are
address mutants:
    segment_order           cl and sel exchanged in the step's base (the cache read as [k | v][ncross]); shows with ncross >= 2
    item_straddle           every row of a 128-row tile takes the item of the tile's first row; shows where a tile crosses an item
    tail_rows               the short last tile is not computed (the grid rounds M / 128 down): its rows keep the prefill
    last_segment_dropped    the K loop ends one step early

---- modality LayerNorm backward --------------------------------------------------------------------------------------------------------
d_x = r (g - mean(g) - xhat mean(g xhat)), g = d_out gain; d_gain += sum_rows d_out xhat; d_bias += sum_rows d_out; two-pass statistics
from x with eps 1e-5.  The bounds are the ``ln_bwd`` derivation of tests/train_kernel_cases.py with H -> E (``lnb_ref`` is general in the
width; depth(E) = ceil(E / 64) + 6 links -- the kernel's lanes hold ceil(E / 512) chunks of 8, summed pairwise, at most E / 64 links -- and
the means are fp32 divisions by E, one rounding where the derivation allows the two of a product with fl(1 / H)).  eps = 1e-5 is given in
fp32: its rounding moves var + eps by at most u32 relative, the "1" the derivation already carries.  x converted from f16 / bf16 is exact,
so the reference takes float64 of the ROUNDED x.  A constant row (CONSTANT_ROW values: E c and every partial sum are exact, the division
returns c) has xhat = 0 exactly and r = 1e-5^-1/2.  In-place (d_x = d_out) and out-of-place calls are held to the same bound.  Mutants:
    one_pass_variance           var = E[x^2] - mean^2; relative error of order u32 mean^2 / var: 6e-4 at |mean| / sigma = 100
    mean_g_dropped              the mean(g) term missing from d_x
    dgain_overwritten           d_gain / d_bias written, not added to: the prefill is lost
    inplace_read_after_write    in place only: the column sums read d_out after d_x has been written over it"""
import torch

from train_kernel_cases import CONSTANT_ROW, U32, _gen, lnb_emulate, lnb_ref, ratio  # noqa: F401  (re-exported for the tests)

F32 = torch.float32
DTYPES = (torch.float16, torch.bfloat16)
ENC_WIDTHS = (768, 1408)
HIDDEN, HEADS = 768, 12
KG_SHAPES = ((3, 40), (2, 257), (1, 1), (5, 64))        # (Ne, kv): two item boundaries in one short tile; boundary at row 257 and a tail of 2;
                                                        # a single row; whole tiles that end on item boundaries
KG_LAYERS = (2, 4, 12)                                  # cross_freq 2: ncross 1 / 2 / 6, K = 1536 / 3072 / 9216
KG_MUTANTS = ("segment_order", "item_straddle", "tail_rows", "last_segment_dropped")
KG_BM = 128
ENC_LN_EPS = 1e-5
LN_ROWS = (1, 63, 64, 257)
LN_MUTANTS = ("one_pass_variance", "mean_g_dropped", "dgain_overwritten", "inplace_read_after_write")


def kg_cases():
    """(layers, Ne, kv): every shape at layers 2 and 4, the K = 9216 handle at the first shape only."""
    return [(lay, ne, kv) for lay in KG_LAYERS for (ne, kv) in (KG_SHAPES if lay < 12 else KG_SHAPES[:1])]


def ncross_of(layers: int, cross_freq: int = 2) -> int:
    return -(-layers // cross_freq)


# =========================================================================================================================================
# kvgrad GEMM
# =========================================================================================================================================
def make_kvgrad(ncross: int, Ne: int, kv: int, E: int, dtype, seed: int = 0, heads: int = HEADS):
    """dkv [ncross * 2, Ne, heads, kv, 64] and W [ncross * 2 * heads * 64, E] rounded to ``dtype``.  Every (segment, item) block carries its
    own scale (1 + its index / 4), so blocks read from the wrong place do not look alike."""
    g = _gen(ncross, Ne, kv, E, seed, 5)
    nsel = ncross * 2
    dkv = torch.randn(nsel, Ne, heads, kv, 64, generator=g) * 0.5
    scale = 1.0 + torch.arange(nsel * Ne, dtype=F32).view(nsel, Ne, 1, 1, 1) / 4.0
    W = torch.randn(nsel * heads * 64, E, generator=g) * 0.05
    return (dkv * scale).to(dtype), W.to(dtype)


def kvgrad_rows(dkv):
    """The cache as the matrix of the contraction: [Ne * kv, K], row item * kv + tok, column (seg * heads + head) * 64 + d."""
    nsel, Ne, heads, kv, hd = dkv.shape
    return dkv.permute(1, 3, 0, 2, 4).reshape(Ne * kv, nsel * heads * hd)


def kvgrad_ref(dkv, W):
    """(d_enc float64 [Ne * kv, E], bound)."""
    A, Wd = kvgrad_rows(dkv).double(), W.double()
    K = A.shape[1]
    return A @ Wd, (K + 1) * U32 * (A.abs() @ Wd.abs())


def kvgrad_emulate(dkv, W, mutant=None, prefill: float = 0.0):
    """fp32, by the kernel's walk: tiles of 128 rows, per 64-wide step the rows' addresses in the flat cache.  Rows the (mutant) kernel does
    not write keep ``prefill``."""
    nsel, Ne, heads, kv, hd = dkv.shape
    ncross = nsel // 2
    M, E = Ne * kv, W.shape[1]
    flat, Wf = dkv.reshape(-1).float(), W.float()
    out = torch.full((M, E), prefill, dtype=F32)
    nseg = nsel * heads
    ntiles = M // KG_BM if mutant == "tail_rows" else (M + KG_BM - 1) // KG_BM
    d = torch.arange(hd)
    for t in range(ntiles):
        m = torch.arange(t * KG_BM, min(M, (t + 1) * KG_BM))
        item = m // kv
        if mutant == "item_straddle":
            item = torch.full_like(m, (t * KG_BM) // kv)
        tok = m - item * kv
        acc = torch.zeros(m.numel(), E, dtype=F32)
        for s in range(nseg - 1 if mutant == "last_segment_dropped" else nseg):
            seg, head = s // heads, s % heads
            if mutant == "segment_order":
                seg = (seg % 2) * ncross + seg // 2
            base = ((seg * Ne + item) * heads + head) * kv * hd + tok * hd
            a = flat[(base[:, None] + d[None, :]) % flat.numel()]      # (a mutant address may leave the cache: wrapped, it is wrong either way)
            acc = acc + a @ Wf[s * hd:(s + 1) * hd]
        out[m] = acc
    return out


# =========================================================================================================================================
# modality LayerNorm backward
# =========================================================================================================================================
def make_mln(rows: int, E: int, x_dtype, seed: int = 0):
    """dict: x [rows, E] in ``x_dtype`` with |mean| / sigma rising from 0 to 100 over the rows (signs alternate) and the LAST row constant
    (CONSTANT_ROW) when rows > 1; d_out [rows, E] fp32; gain [E] fp32 with zeros (every 7th) and negative entries; dgain0 / dbias0 [E]
    prefills of clearly non-zero size."""
    g = _gen(rows, E, seed, 11)
    x = torch.randn(rows, E, generator=g)
    off = torch.linspace(0.0, 100.0, rows) * (1.0 - 2.0 * (torch.arange(rows) % 2))
    if rows == 1:
        off = torch.tensor([100.0])
    x = x + off[:, None]
    if rows > 1:
        x[-1] = CONSTANT_ROW[rows % len(CONSTANT_ROW)]
    gain = 1.0 + 0.3 * torch.randn(E, generator=g)
    gain[::7] = 0.0
    gain[1::11] = -gain[1::11].abs() - 0.5
    return dict(x=x.to(x_dtype), d_out=torch.randn(rows, E, generator=g), gain=gain, dgain0=torch.randn(E, generator=g) * 5.0,
                dbias0=torch.randn(E, generator=g) * 5.0)


def mln_ref(x, d_out, gain, dgain0=None, dbias0=None):
    """float64 of the rounded x: (d_x, bound, d_gain, bound, d_bias, bound); NULL prefills count as zero."""
    return lnb_ref(x.float(), d_out, gain, ENC_LN_EPS, None, dgain0, dbias0)


def mln_emulate(x, d_out, gain, dgain0=None, dbias0=None, inplace: bool = False, mutant=None):
    """modality_ln_bwd_kernel's fp32 arithmetic (torch's fp32 sums stand in for the wave sums, the LDS and the global atomics).
    Returns (d_x, d_gain, d_bias)."""
    xf = x.float()
    E = xf.shape[1]
    n = torch.tensor(float(E), dtype=F32)
    mean = xf.sum(-1, keepdim=True) / n
    d = xf - mean
    if mutant == "one_pass_variance":
        var = (xf * xf).sum(-1, keepdim=True) / n - mean * mean
    else:
        var = (d * d).sum(-1, keepdim=True) / n
    rstd = 1.0 / torch.sqrt(var + torch.tensor(ENC_LN_EPS, dtype=F32))
    xh = d * rstd
    g = d_out * gain
    sg = g.sum(-1, keepdim=True) / n
    sgx = (g * xh).sum(-1, keepdim=True) / n
    if mutant == "mean_g_dropped":
        sg = torch.zeros_like(sg)
    dx = rstd * (g - sg - xh * sgx)
    src = dx if (mutant == "inplace_read_after_write" and inplace) else d_out
    g0 = dgain0 if (dgain0 is not None and mutant != "dgain_overwritten") else 0.0
    b0 = dbias0 if (dbias0 is not None and mutant != "dgain_overwritten") else 0.0
    return dx, (src * xh).sum(0) + g0, src.sum(0) + b0
