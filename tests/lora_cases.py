"""Shared by tests/test_lora_cases_cpu.py and tests/test_gpu_lora.py (not a test module): seeded inputs rounded to the operand type, float64
references, DERIVED per-element bounds and fp32 emulations (with named mutants) for the three kernels of csrc/lora.hip behind
``mra_lora_down`` / ``mra_lora_up_add`` / ``mra_lora_wgrad``.  Pure torch on the CPU.  Conventions and notation as tests/train_kernel_cases.py:
u32 = 2^-24, u = U[T] (2^-11 f16, 2^-8 bf16), every bound worst case and first order, nothing fitted to GPU output; a sum whose order is
not fixed (the MFMA's internal order) is bounded as a sum in ANY order at one u32 per link.

A small fp32 matrix over (width index n, rank index j) is handled here in its LOGICAL form W [R, width]; ``as_memory`` lays it out as the
entries take it (``NR`` = [width][R], ``RN`` = [R][width]).  The dropout mask is ``mraudio_amd.models.lora.keep_mask`` (element (m, n) has
index m * width + n: the width, not the pitch); masked inputs enter every reference already masked, so the references do not hash.

---- down: out[m][j] = scale sum_k xd[m][k] op(W)[j][k],  xd = keep x --------------------------------------------------------------------
A product of two f16 values has 22 significant bits and of two bf16 values 16: exact in fp32.  K products meet in K - 1 additions, in the
order of the MFMA steps, of the four waves that share the K steps and of their fixed-order sum through LDS; the product with the scale is
one more rounding:
    |out - ref| <= (K + 2) u32 |scale| sum_k |xd op(W)|                      (+ 2: first order; with scale = 1/q this is (K + 2) u32 sum|x A| / q)
The emulation walks the kernel: 16-row workgroups, 32-wide K steps dealt round robin to 4 waves, ((w0 + w1) + w2) + w3, times the scale.
Mutants:  tail_rows (the short last 16-row tile is not computed), last_k_step_dropped, layout_ignored (W's memory read in the other layout),
          mask_ld (the mask indexed with the pitch instead of K; shows on a pitched x with p > 0), scale_twice (1/q applied twice).

---- up_add: y[m][n] = T(float(y0) + sc sum_j u[m][j] W[j][n]),  sc = scale keep(m, n) -----------------------------------------------------
t = the fma chain from 0 over j ascending: R roundings, R u32 sum_j |u W|; v = fma(sc, t, y0): one rounding, u32 |v|; then T(v):
    e    = (R + 1) u32 |sc| sum_j |u W| + u32 |ref|
    |y - ref| <= e + u (|ref| + e) + 2^-25 [f16]                                 (half an ulp of the output dtype, the f16 subnormal spacing)
Mutants:  tail_rows (the short last 64-row tile), layout_ignored, mask_ld, scale_twice.

---- wgrad: dW[j][n] = dW0[j][n] + scale sum_m xd[m][n] op(u)[m][j] ------------------------------------------------------------------------
M exact products in M - 1 additions (MFMA steps over 32 rows, 4 waves, fixed-order LDS sum), one fma onto the prefilled value:
    |dW - ref| <= (M + 2) u32 (|scale| sum_m |xd op(u)| + |dW0|)
Mutants:  tail_rows (the short last 32-row step), prefill_overwritten (dW written, not added to), u_unrounded (u enters the product in fp32),
          layout_ignored, mask_ld."""
import torch

from mraudio_amd.models.lora import keep_mask
from train_kernel_cases import F16_SUB, U, U32, _gen, ratio  # noqa: F401  (re-exported for the tests)

F32, F64 = torch.float32, torch.float64
DTYPES = (torch.float16, torch.bfloat16)
NR, RN = 0, 1                                    # MRA_LORA_NR / MRA_LORA_RN
ROWS = (1, 15, 16, 17, 67)                       # a single row; one short of, exactly and one past a 16-row tile; past a 64-row tile (and two 32-row steps + 3)
WIDTHS = (8, 32, 40, 264)                        # one vector; one MFMA step; a step and a tail; several steps and a tail
RANKS = (1, 5, 8, 16)
PS = (0.0, 0.05, 0.5)
SEED = 0x1234_5678_9ABC_DEF1
DOWN_MUTANTS = ("tail_rows", "last_k_step_dropped", "layout_ignored", "mask_ld", "scale_twice")
UP_MUTANTS = ("tail_rows", "layout_ignored", "mask_ld", "scale_twice")
WGRAD_MUTANTS = ("tail_rows", "prefill_overwritten", "u_unrounded", "layout_ignored", "mask_ld")


def cases():
    return [(m, w, r, p) for m in ROWS for w in WIDTHS for r in RANKS for p in PS]


def pitch(rows: int, width: int, R: int) -> int:
    """Every other case is a pitched view (ld = width + 8)."""
    return width + (8 if (rows + width // 8 + R) % 2 else 0)


def as_memory(Wl: torch.Tensor, layout: int) -> torch.Tensor:
    return Wl.t().contiguous() if layout == NR else Wl.contiguous()


def from_memory(mem: torch.Tensor, layout: int, R: int, width: int) -> torch.Tensor:
    return mem.reshape(width, R).t() if layout == NR else mem.reshape(R, width)


def _misread(Wl: torch.Tensor, layout: int) -> torch.Tensor:
    """The logical matrix a kernel sees that ignores the layout flag."""
    R, width = Wl.shape
    return from_memory(as_memory(Wl, layout).reshape(-1), RN if layout == NR else NR, R, width)


def make_case(rows: int, width: int, R: int, dtype, seed: int = 0):
    """x, y0 [rows, width] in ``dtype``; W [R, width] fp32 (row j scaled by 1 + j / R, so rows read from the wrong place do not look alike);
    u [rows, R] fp32; dW0 [R, width] fp32 prefill of clearly non-zero size."""
    g = _gen(rows, width, R, seed, 23)
    x = torch.randn(rows, width, generator=g).to(dtype)
    y0 = torch.randn(rows, width, generator=g).to(dtype)
    W = torch.randn(R, width, generator=g) * 0.2 * (1.0 + torch.arange(R, dtype=F32)[:, None] / R)
    u = torch.randn(rows, R, generator=g) * 0.5
    return dict(x=x, y0=y0, W=W, u=u, dW0=torch.randn(R, width, generator=g) * 3.0)


def mask(rows: int, width: int, p: float, seed: int = SEED, ld=None) -> torch.Tensor:
    """bool [rows, width]; ``ld``: the mutant's mask, indexed with the pitch."""
    return keep_mask(seed, rows, width, p) if ld is None else keep_mask(seed, rows, ld, p)[:, :width]


def inv_q(p: float) -> float:
    return float(torch.tensor(1.0 / (1.0 - p), dtype=F32))          # the fp32 value the entries receive


# ---- down ---------------------------------------------------------------------------------------------------------------------------------
def down_ref(x, W, scale: float, keep):
    xd, Wd = (x * keep.to(x.dtype)).double(), W.to(x.dtype).double()
    return scale * (xd @ Wd.t()), (x.shape[1] + 2) * U32 * abs(scale) * (xd.abs() @ Wd.abs().t())


def down_emulate(x, W, layout: int, scale: float, p: float, seed: int = SEED, ld=None, mutant=None, prefill: float = float("nan")):
    M, K = x.shape
    keep = mask(M, K, p, seed, ld if mutant == "mask_ld" else None)
    xd = (x * keep.to(x.dtype)).float()
    Wf = (_misread(W, layout) if mutant == "layout_ignored" else W).to(x.dtype).float()
    out = torch.full((M, W.shape[0]), prefill, dtype=F32)
    nsteps = (K + 31) // 32 - (1 if mutant == "last_k_step_dropped" else 0)
    ntiles = M // 16 if mutant == "tail_rows" else (M + 15) // 16
    for t in range(ntiles):
        m0, m1 = t * 16, min(M, t * 16 + 16)
        waves = []
        for w in range(4):
            acc = torch.zeros(m1 - m0, W.shape[0], dtype=F32)
            for s in range(w, nsteps, 4):
                acc = acc + xd[m0:m1, s * 32:(s + 1) * 32] @ Wf[:, s * 32:(s + 1) * 32].t()
            waves.append(acc)
        tot = ((waves[0] + waves[1]) + waves[2]) + waves[3]
        tot = tot * torch.tensor(scale, dtype=F32)
        out[m0:m1] = tot * torch.tensor(scale, dtype=F32) if mutant == "scale_twice" else tot
    return out


# ---- up_add -------------------------------------------------------------------------------------------------------------------------------
def up_ref(y0, u, W, scale: float, keep):
    dtype = y0.dtype
    sc = scale * keep.double()
    t_abs = u.double().abs() @ W.double().abs()
    ref = y0.double() + sc * (u.double() @ W.double())
    e = (W.shape[0] + 1) * U32 * sc.abs() * t_abs + U32 * ref.abs()
    return ref, e + U[dtype] * (ref.abs() + e) + (F16_SUB if dtype == torch.float16 else 0.0)


def _fma(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in float64."""
    return (a.double() * b.double() + c.double()).float()


def up_emulate(y0, u, W, layout: int, scale: float, p: float, seed: int = SEED, ld=None, mutant=None):
    M, N = y0.shape
    keep = mask(M, N, p, seed, ld if mutant == "mask_ld" else None)
    Wf = _misread(W, layout) if mutant == "layout_ignored" else W
    acc = torch.zeros(M, N, dtype=F32)
    for j in range(W.shape[0]):
        acc = _fma(u[:, j:j + 1].expand(M, N), Wf[j:j + 1].expand(M, N), acc)
    s = torch.tensor(scale * scale if mutant == "scale_twice" else scale, dtype=F32)
    out = torch.where(keep, _fma(s.expand(M, N), acc, y0.float()).to(y0.dtype), y0)      # a dropped element keeps its bits
    if mutant == "tail_rows":
        out[M // 64 * 64:] = y0[M // 64 * 64:]
    return out


# ---- wgrad --------------------------------------------------------------------------------------------------------------------------------
def wgrad_ref(x, u, dW0, scale: float, keep):
    xd, ud = (x * keep.to(x.dtype)).double(), u.to(x.dtype).double()
    return dW0.double() + scale * (ud.t() @ xd), (x.shape[0] + 2) * U32 * (abs(scale) * (ud.abs().t() @ xd.abs()) + dW0.double().abs())


def wgrad_emulate(x, u, dW0, layout: int, scale: float, p: float, seed: int = SEED, ld=None, mutant=None):
    """Returns the LOGICAL [R, N] result; ``layout`` matters to the layout_ignored mutant only (the prefill is read, and the result written,
    through the other layout)."""
    M, N = x.shape
    R = u.shape[1]
    keep = mask(M, N, p, seed, ld if mutant == "mask_ld" else None)
    xd = (x * keep.to(x.dtype)).float()
    uf = u.float() if mutant == "u_unrounded" else u.to(x.dtype).float()
    nsteps = M // 32 if mutant == "tail_rows" else (M + 31) // 32
    waves = []
    for w in range(4):
        acc = torch.zeros(R, N, dtype=F32)
        for s in range(w, nsteps, 4):
            acc = acc + uf[s * 32:(s + 1) * 32].t() @ xd[s * 32:(s + 1) * 32]
        waves.append(acc)
    tot = ((waves[0] + waves[1]) + waves[2]) + waves[3]
    s32 = torch.tensor(scale, dtype=F32).expand(R, N)
    if mutant == "prefill_overwritten":
        return tot * s32
    if mutant == "layout_ignored":       # the kernel addresses dW as the other layout: in memory, element (j, n) sits where that layout puts it
        other = RN if layout == NR else NR
        mem = as_memory(dW0, layout).reshape(-1).clone()
        seen = from_memory(mem, other, R, N)                       # a view of the same memory
        seen.copy_(_fma(s32, tot, seen.clone()))
        return from_memory(mem, layout, R, N).clone()
    return _fma(s32, tot, dW0)
