"""Shared by tests/test_proj_grad_cases_cpu.py and tests/test_gpu_proj_grad.py (not a test module): seeded inputs rounded to the operand
type, float64 references, DERIVED per-element bounds and fp32 emulations (with named mutants) for ``mra_llm_proj_backward``
(csrc/proj_grad.hip), the backward of the LLM projection y = op(z) W^T + b.  Pure torch on the CPU.  Conventions and notation as
tests/train_kernel_cases.py (u32 = 2^-24, every bound worst case and first order, nothing fitted to GPU output).

dY = op(d_out): an fp32 upstream gradient is rounded to the operand type first, and that rounding is part of the definition -- every
reference below takes the ROUNDED d_out (a d_out given in the operand type is its own rounding).  z16 = op(z) likewise.

---- d_z[r][h] = sum_k dY[r][k] W[k][h], k over llm_hidden = Lh ---------------------------------------------------------------------------
The derivation of the kvgrad GEMM in tests/enc_grad_cases.py with K -> Lh: products of two f16 / bf16 values are exact in fp32, Lh exact
products are summed in some order:
    |d_z - ref| <= (Lh + 1) u32 sum_k |dY W|          against float64 of the rounded operands.
The emulation walks the kernel's tiles (128 rows, one 64-wide K step at a time).  Mutants:
    tail_rows               the short last row tile is not computed (the grid rounds R / 128 down): its rows keep the prefill
    last_k_step_dropped     the K loop ends one step early
    w_not_transposed        W's memory read as [H][Lh]: element (k, h) taken from flat index h * Lh + k
    dy_unrounded            an fp32 d_out enters the product unrounded (shows with an fp32 d_out only)

---- d_W[k][h] += sum_r dY[r][k] z16[r][h],  d_b[k] += sum_r dY[r][k] -----------------------------------------------------------------------
One launch_gemm_tn with its db output: reference, bound, split count and emulation are ``tn_ref`` / ``tn_splits`` / ``tn_emulate`` of
tests/train_kernel_cases.py with M = R, N = Lh, K = H.  d_b asked for alone runs the same launch on the first 64 columns of z16 (K = 64:
``db_alone_splits``).  Mutant: prefill_overwritten (d_W written, not added to)."""
import torch

from train_kernel_cases import U32, _gen, ratio, tn_emulate, tn_ref, tn_splits  # noqa: F401  (re-exported for the tests)

F32 = torch.float32
DTYPES = (torch.float16, torch.bfloat16)
ROWS = (1, 32, 127, 128, 129, 257, 640)          # a single row, a short tile, one row short of / exactly / one past a 128-row tile, 2 tiles + 1, 5 tiles
LLM_HIDDEN = (64, 128, 320, 256)                 # one, two, an odd number (5) and four K steps of 64
HIDDEN = 256                                     # two 128-column tiles of d_z
BIG = (129, 4096, 768)                           # the shipped projection (64 K steps, six column tiles) at one tile + 1 row
PG_BM = 128
DZ_MUTANTS = ("tail_rows", "last_k_step_dropped", "w_not_transposed", "dy_unrounded")
DW_MUTANTS = ("prefill_overwritten",)


def cases():
    """(rows, llm_hidden, hidden): every rows value at every small llm_hidden, llm_hidden = 4096 at rows = 129 only."""
    return [(r, lh, HIDDEN) for lh in LLM_HIDDEN for r in ROWS] + [BIG]


def make_proj(rows: int, Lh: int, H: int, dtype, dout_f32: bool, seed: int = 0):
    """dict: z [rows, H] fp32; W [Lh, H] in ``dtype`` (row k scaled by 1 + k / Lh so rows read from the wrong place do not look alike);
    d_out [rows, Lh] fp32 (unrounded) or already in ``dtype``; dW0 [Lh, H], db0 [Lh] fp32 prefills of clearly non-zero size."""
    g = _gen(rows, Lh, H, seed, 17)
    z = torch.randn(rows, H, generator=g)
    W = (torch.randn(Lh, H, generator=g) * 0.05 * (1.0 + torch.arange(Lh, dtype=F32)[:, None] / Lh)).to(dtype)
    d_out = torch.randn(rows, Lh, generator=g) * 0.5
    return dict(z=z, W=W, d_out=d_out if dout_f32 else d_out.to(dtype), dW0=torch.randn(Lh, H, generator=g) * 3.0,
                db0=torch.randn(Lh, generator=g) * 3.0)


def dz_ref(d_out, W):
    """(d_z float64 [rows, H], bound) from the operand-rounded d_out."""
    dy, Wd = d_out.to(W.dtype).double(), W.double()
    Lh = Wd.shape[0]
    return dy @ Wd, (Lh + 1) * U32 * (dy.abs() @ Wd.abs())


def dz_emulate(d_out, W, mutant=None, prefill: float = float("nan")):
    """fp32, by the kernel's walk: tiles of 128 rows, 64-wide K steps in ascending order.  Rows the (mutant) kernel does not write keep
    ``prefill``."""
    Lh, H = W.shape
    dy = d_out.float() if mutant == "dy_unrounded" else d_out.to(W.dtype).float()
    Wf = W.reshape(-1).view(H, Lh).T.float() if mutant == "w_not_transposed" else W.float()
    R = dy.shape[0]
    out = torch.full((R, H), prefill, dtype=F32)
    nseg = Lh // 64
    ntiles = R // PG_BM if mutant == "tail_rows" else (R + PG_BM - 1) // PG_BM
    for t in range(ntiles):
        m0, m1 = t * PG_BM, min(R, (t + 1) * PG_BM)
        acc = torch.zeros(m1 - m0, H, dtype=F32)
        for s in range(nseg - 1 if mutant == "last_k_step_dropped" else nseg):
            acc = acc + dy[m0:m1, s * 64:(s + 1) * 64] @ Wf[s * 64:(s + 1) * 64]
        out[m0:m1] = acc
    return out


def db_alone_splits(rows: int, Lh: int) -> int:
    """Pieces of the contraction when d_bias is asked for without d_weight: the launch over one 64-column block of z16."""
    return tn_splits(rows, Lh, 64)


def dw_ref(d_out, z, W_dtype, dW0, db0, splits: int):
    """(d_W float64, bound, d_b float64, bound) from the operand-rounded d_out and z; prefills None = zero."""
    return tn_ref(d_out.to(W_dtype), z.to(W_dtype), dW0, db0, splits)


def dw_emulate(d_out, z, W_dtype, dW0, db0, splits: int, mutant=None):
    return tn_emulate(d_out.to(W_dtype), z.to(W_dtype), dW0, db0, splits, mutant)
