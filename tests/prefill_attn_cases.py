"""Shared by tests/test_prefill_attn_cases_cpu.py and tests/test_gpu_prefill_attn.py (not a test module): the case table, seeded inputs rounded
to the operand type, the float64 reference, a DERIVED per-element bound and the fp32 emulation (with named mutants) of the kernel of
csrc/prefill_attn.hip behind ``mra_prefill_attention``.  Pure torch on the CPU.  Conventions as tests/decode_attn_cases.py: u32 = 2^-24,
u = U[T] (2^-11 f16, 2^-8 bf16), every bound worst case and first order, nothing fitted to GPU output; a sum whose order is not fixed here is
bounded as a sum in ANY order at one u32 per link.  The reference is float64 on the ROUNDED operands q, k, v.

    attended(b, i) = {s : s <= q_offset + i, s < Skv, mask[b, s]}
    z_s = scale q[b,h,i] . k[b, h / G, s],   lse = log sum_s exp z_s,   p = softmax(z),   out = sum_s p_s v[b, h / G, s]      (attended s only)
    a row with no attended key: out = +0, lse = -inf (asserted as such, not through a bound)

Geometry read off the kernel: a workgroup owns QB query rows, a wave 32-row blocks; key tiles of KT = 32 keys are walked in ascending order up
to the diagonal of a block's last row (nt <= ceil(Skv / KT) tiles); a tile without an attended key below the workgroup's last diagonal is
skipped.  Per processed tile, in log2 units (z2 = z log2e): m_new = max(m_run, max z2), alpha = exp2(m_run - m_new), p~ = exp2(z2 - m_new),
l = l alpha + sum p~ (fp32, the UNROUNDED p~), O = O alpha + round_T(p~) V (MFMA, fp32 accumulation).  out = O / l, lse = m ln2 + log l.

---- logits -----------------------------------------------------------------------------------------------------------------------------
Products of two 16-bit values are exact in fp32; D of them meet in D - 1 additions inside the MFMAs (any order), then one product with
scale log2e:                           e_z[s] = (D + 2) u32 |scale| sum_d |q_d| |k_sd|

---- the terms --------------------------------------------------------------------------------------------------------------------------
With m_t(s) the running maximum once the tile of s is in, and M the final one (both maxima of computed values: exact, and they cancel):
    eta[s]   = 3 u32 |z_s - m_t(s)| + 2 u32        the exp2 argument (subtraction, constant, product) and the hardware exp2 (1 ulp; 2 u32 taken)
    zeta[s]  = 3 u32 |m_t(s) - M| + 3 u32 nt       the alphas behind it: their arguments telescope to m_t(s) - M; at most nt of them, each an
                                                   exp2 (2 u32) and a product (u32)
    rel[s]   = e_z[s] + eta[s] + zeta[s]           relative error of the term exp(z_s - M) as it enters either sum
---- lse --------------------------------------------------------------------------------------------------------------------------------
l: 15 additions inside a tile's partial sum, a product and an addition per later tile, one addition across the two half-waves:
N_l = 2 nt + 18 links.      lse_b = sum_s p_s rel[s] + N_l u32 + u32 (4 |lse - M| + |lse| + 2 |M|)
(logf to 2 ulp, twice for first order; the rounding of the sum; m ln2: the constant and the product.)

---- out --------------------------------------------------------------------------------------------------------------------------------
P is rounded once to T in front of the second product: |round(p~) - p~| <= u p~, and for f16 at least 2^-25 (the subnormal spacing), which
enters O at weight exp(m_t(s) - M) <= 1.  O: 32 products per tile in any order, a product and an addition per later tile, 1 / l and the
product with it: N_o = 2 nt + 36 links.
    e[d]     = sum_s p_s |v_sd| (rel[s] + u + N_o u32) + [f16] 2^-25 sum_s exp(m_t(s) - M) |v_sd| / l_M
               + |out_d| (sum_s p_s rel[s] + N_l u32) + 2 u32 |out_d|                              (l_M = sum_s exp(z_s - M) >= 1)
    out_b[d] = e + u (|out_d| + e) + 2^-25 [f16: the subnormal spacing of the output]

Cases.  Sizes with Sq = Skv = S for S in {1, 2, KT - 1, KT, KT + 1, QB - 1, QB, QB + 1, 2 QB + 3, 4 QB + 17}, and (Sq, Skv, q_offset) in
{(5, KT + 6, KT + 1), (QB + 1, 3 QB, QB - 1), (3, 2 QB + 40, 0)} (the last: a static cache), each under seven mask families; D, (Hq, Hkv) and
B are dealt so that every value of one meets every value of every other (asserted in the CPU test).  Masked K / V slots and every slot at or
behind q_offset + Sq (above every diagonal: the unwritten tail of a static cache) hold NaN and +-Inf.
Mask families: null (no mask), ones, left_pad, holes, mid_tile (one whole key tile masked in the middle), first_qb (the first QB keys masked,
or all below the last row's diagonal key when that comes first), row_masked (holes, and the last batch row has no attended key at all).
Score families, by (b Hq + h + offset) % 6: mild; peak_diag (every query about 30 above the rest on its own diagonal key); peak_first (on the
sequence's first attended key: in the first tile); plus90 / minus90 (column 0 of K is 4 everywhere, q_0 = +-90 / (4 scale): fp32 exp(+-90)
overflows / flushes without the running maximum); equal (q = 0: out = the mean of the attended V rows, lse = log count).

Mutants (``emulate(..., mutant=)``): diag_exclusive (s < i), offset_dropped (q_offset taken as 0), masked_zero (a logit masked by its key
byte enters as 0), skip_resets_max (a skipped tile puts the running maximum back to its start), no_rescale (O is not multiplied by alpha),
ragged_counted (the slots past Skv of the last tile enter as zero logits with zero V), head_mod (the K/V head of query head h taken as
h % Hkv), scale_twice, empty_div0 (a row with no attended key is divided by its zero sum)."""
import functools

import torch

from train_kernel_cases import F16_SUB, U, U32, _gen, ratio  # noqa: F401  (re-exported for the tests)

F32, F64 = torch.float32, torch.float64
DTYPES = (torch.float16, torch.bfloat16)
QB, KT = 256, 32                              # PREFILL_QB, PREFILL_KT of csrc/kernels.h
SIZES = tuple((S, S, 0) for S in (1, 2, KT - 1, KT, KT + 1, QB - 1, QB, QB + 1, 2 * QB + 3, 4 * QB + 17)) + \
    ((5, KT + 6, KT + 1), (QB + 1, 3 * QB, QB - 1), (3, 2 * QB + 40, 0))
DIMS = (64, 128)
HEADS = ((4, 4), (4, 2), (8, 2), (8, 1), (3, 3))
BATCHES = (1, 3)
MASKS = ("null", "ones", "left_pad", "holes", "mid_tile", "first_qb", "row_masked")
FAMILIES = ("mild", "peak_diag", "peak_first", "plus90", "minus90", "equal")
MUTANTS = ("diag_exclusive", "offset_dropped", "masked_zero", "skip_resets_max", "no_rescale", "ragged_counted", "head_mod", "scale_twice",
           "empty_div0")
L2E = 1.4426950408889634
LN2 = 0.6931471805599453
M_START = -1e30                               # the running maximum's start: finite, below every logit


def cases():
    """(B, Hq, Hkv, Sq, Skv, q_offset, D, mask family): every size with every mask family; D, heads and B dealt over them."""
    out = []
    for si, (Sq, Skv, off) in enumerate(SIZES):
        for mi, mask in enumerate(MASKS):
            Hq, Hkv = HEADS[(si + 2 * mi) % 5]
            out.append((BATCHES[(si + mi // 2 + mi // 4) % 2], Hq, Hkv, Sq, Skv, off, DIMS[(si + mi) % 2], mask))
    return out


def layout(Hq: int, Sq: int, Skv: int, D: int):
    """dict(Smax, k_ss, v_ss, o_sh, o_ss): K / V as views of a longer, possibly pitched buffer, out with padded head and position strides
    (elements).  q is always handed as the transposed view of a [B, Sq, Hq, D] tensor."""
    o_sh = D + 8 * (1 + Hq % 3)
    return dict(Smax=Skv + 3 + 8 * (Skv % 3), k_ss=D + (8 if Skv % 2 else 0), v_ss=D + (16 if (Skv + Hq) % 3 == 0 else 0), o_sh=o_sh,
                o_ss=Hq * o_sh + 8 * (Sq % 2))


def make_mask(name: str, B: int, Skv: int, gen, last=None):
    """bool [B, Skv] (True = attend) or None.  ``last`` = q_offset + Sq: the keys below it are the ones a row can attend."""
    last = Skv if last is None else last
    if name == "null":
        return None
    m = torch.ones(B, Skv, dtype=torch.bool)
    if name == "left_pad":
        for b in range(B):
            m[b, :min(last - 1, 5 + 31 * b)] = False
    elif name in ("holes", "row_masked"):
        m = torch.rand(B, Skv, generator=gen) >= 0.25
        m[:, (Skv - 1) // 2] = True
        if name == "row_masked":
            m[B - 1] = False
    elif name == "mid_tile":
        nt = (Skv + KT - 1) // KT
        if nt >= 3:
            m[:, (nt // 2) * KT:(nt // 2 + 1) * KT] = False
        else:
            m[:, Skv // 3: max(Skv // 3, 2 * Skv // 3)] = False
            m[:, 0] = True
    elif name == "first_qb":
        m[:, :min(QB, last - 1)] = False
    return m


def _poison(t: torch.Tensor, where: torch.Tensor) -> None:
    """NaN, +Inf, -Inf in turn over the elements of ``t`` selected by the boolean ``where`` (same shape)."""
    n = int(where.sum())
    if n:
        vals = torch.tensor([float("nan"), float("inf"), float("-inf")]).repeat((n + 2) // 3)[:n]
        t[where] = vals.to(t.dtype)


def attended(mask, B: int, Sq: int, Skv: int, q_offset: int, exclusive: bool = False):
    """bool [B, Sq, Skv]."""
    i = torch.arange(Sq)[:, None] + q_offset
    s = torch.arange(Skv)[None, :]
    on = (s < i) if exclusive else (s <= i)
    on = on[None].expand(B, Sq, Skv)
    return on if mask is None else on & mask.reshape(B, 1, Skv).bool()


@functools.lru_cache(maxsize=None)
def make_case(B: int, Hq: int, Hkv: int, Sq: int, Skv: int, q_offset: int, D: int, mask_name: str, dtype):
    """q [B, Hq, Sq, D], k, v [B, Hkv, Skv, D] in ``dtype`` (masked slots and the slots behind q_offset + Sq poisoned), mask bool [B, Skv] or
    None, scale (a Python float that is exact in fp32), family [B][Hq]."""
    gen = _gen(B, Hq, Hkv, Sq, Skv, q_offset, D, MASKS.index(mask_name), 53)
    G = Hq // Hkv
    scale = float(torch.tensor(D ** -0.5, dtype=F32))
    mask = make_mask(mask_name, B, Skv, gen, last=q_offset + Sq)
    att = torch.ones(B, Skv, dtype=torch.bool) if mask is None else mask.clone()
    att[:, q_offset + Sq:] = False
    k = torch.randn(B, Hkv, Skv, D, generator=gen)
    k[..., 0] = 4.0
    k = k.to(dtype)
    v = torch.randn(B, Hkv, Skv, D, generator=gen).to(dtype)
    q = torch.randn(B, Hq, Sq, D, generator=gen)
    off = (Skv + D // 64) % 6
    family = [[FAMILIES[(b * Hq + h + off) % 6] for h in range(Hq)] for b in range(B)]
    kd = k.double()
    for b in range(B):
        idx = torch.nonzero(att[b]).squeeze(1)
        for h in range(Hq):
            fam = family[b][h]
            if fam == "peak_diag" or (fam == "peak_first" and idx.numel()):
                d = kd[b, h // G, q_offset:q_offset + Sq].clone() if fam == "peak_diag" else kd[b, h // G, int(idx[0])].clone()[None]
                d[:, 0] = 0.0                                # the shared column would lift every logit alike
                q[b, h] += ((30.0 / scale) * (d / (d * d).sum(1, keepdim=True))).float()
            elif fam in ("plus90", "minus90"):
                q[b, h, :, 0] = (90.0 if fam == "plus90" else -90.0) / (4.0 * scale)
            elif fam == "equal":
                q[b, h] = 0.0
    dead = ~att[:, None, :, None].expand(B, Hkv, Skv, D)
    _poison(k, dead)
    _poison(v, dead)
    return dict(q=q.to(dtype), k=k, v=v, mask=mask, scale=scale, family=family)


def reference_tensors(q, k, v, mask, scale: float, q_offset: int, dtype):
    """float64 values and the bounds of the module docstring for ANY operands: q [B, Hq, Sq, D], k, v [B, Hkv, Skv, D] (16-bit values; what
    unattended slots hold is ignored), mask bool [B, Skv] or None.  dict(out [B, Sq, Hq, D], lse [B, Hq, Sq], out_b, lse_b, empty [B, Hq, Sq])."""
    B, Hq, Sq, D = q.shape
    Hkv, Skv = k.shape[1], k.shape[2]
    G = Hq // Hkv
    u = U[dtype]
    nt = (Skv + KT - 1) // KT
    N_l, N_o = 2 * nt + 18, 2 * nt + 36
    att = attended(mask, B, Sq, Skv, q_offset)
    zero, ninf = torch.zeros((), dtype=F64), torch.full((), float("-inf"), dtype=F64)
    res = dict(out=[], lse=[], out_b=[], lse_b=[], empty=[])
    for b in range(B):                                       # one sequence at a time: [Hq, Sq, Skv] float64 temporaries
        a3 = att[b][None].expand(Hq, Sq, Skv)
        some = att[b].any(0)[None, :, None]                  # [1, Skv, 1]: attended by a row
        kd = torch.where(some, k[b].double(), zero).repeat_interleave(G, dim=0)      # [Hq, Skv, D]
        vd = torch.where(some, v[b].double(), zero).repeat_interleave(G, dim=0)
        qd = q[b].double()                                   # [Hq, Sq, D]
        z = torch.where(a3, scale * (qd @ kd.transpose(1, 2)), ninf)
        e_z = (D + 2) * U32 * abs(scale) * (qd.abs() @ kd.abs().transpose(1, 2))
        empty = ~a3.any(2)
        lse = torch.logsumexp(z, dim=2)
        lse_safe = torch.where(empty, zero, lse)
        p = torch.where(a3, torch.exp(z - lse_safe[:, :, None]), zero)
        out = p @ vd                                         # [Hq, Sq, D]
        zt = torch.cat([z, ninf.expand(Hq, Sq, nt * KT - Skv)], 2).view(Hq, Sq, nt, KT).max(3).values
        m_t = torch.cummax(zt, dim=2).values                 # -inf in front of the row's first attended key
        M = m_t[:, :, -1]
        M_safe = torch.where(empty, zero, M)
        m_s = m_t.repeat_interleave(KT, dim=2)[:, :, :Skv]
        eta = torch.where(a3, 3 * U32 * (z - m_s).abs() + 2 * U32, zero)
        zeta = torch.where(a3, 3 * U32 * (m_s - M_safe[:, :, None]).abs() + 3 * U32 * nt, zero)
        rel = torch.where(a3, e_z, zero) + eta + zeta
        prel = (p * rel).sum(2)
        lse_b = prel + N_l * U32 + U32 * (4 * (lse_safe - M_safe).abs() + lse_safe.abs() + 2 * M_safe.abs())
        va = vd.abs()
        e = (p * (rel + u + N_o * U32)) @ va + out.abs() * (prel + N_l * U32)[:, :, None] + 2 * U32 * out.abs()
        if dtype == torch.float16:
            l_M = torch.where(a3, torch.exp(z - M_safe[:, :, None]), zero).sum(2)
            w = torch.where(a3, torch.exp(m_s - M_safe[:, :, None]), zero)
            e = e + 2.0 ** -25 * (w @ va) / torch.where(empty, torch.ones((), dtype=F64), l_M)[:, :, None]
        out_b = e + u * (out.abs() + e) + (F16_SUB if dtype == torch.float16 else 0.0)
        for name, t in (("out", out.transpose(0, 1)), ("lse", lse), ("out_b", out_b.transpose(0, 1)), ("lse_b", lse_b), ("empty", empty)):
            res[name].append(t)
    return {name: torch.stack(ts) for name, ts in res.items()}


@functools.lru_cache(maxsize=None)
def reference(B: int, Hq: int, Hkv: int, Sq: int, Skv: int, q_offset: int, D: int, mask_name: str, dtype):
    c = make_case(B, Hq, Hkv, Sq, Skv, q_offset, D, mask_name, dtype)
    return reference_tensors(c["q"], c["k"], c["v"], c["mask"], c["scale"], q_offset, dtype)


def emulate_tensors(q, k, v, mask, scale: float, q_offset: int, dtype, mutant=None):
    """The kernel in fp32 torch ops, tile by tile in ascending order with its skips: (out [B, Sq, Hq, D] in ``dtype``, lse f32 [B, Hq, Sq])."""
    B, Hq, Sq, D = q.shape
    Hkv, Skv = k.shape[1], k.shape[2]
    G = Hq // Hkv
    off = 0 if mutant == "offset_dropped" else q_offset
    heads = torch.arange(Hq) % Hkv if mutant == "head_mod" else torch.arange(Hq) // G
    zf, ninf = torch.zeros((), dtype=F32), torch.full((), float("-inf"), dtype=F32)
    key = torch.ones(B, Skv, dtype=torch.bool) if mask is None else mask.reshape(B, Skv).bool()
    rows = torch.arange(Sq)
    qend = torch.clamp((rows // QB + 1) * QB, max=Sq)                   # the end of the row's workgroup
    kend = off + qend                                                    # [Sq]: keys below it may be staged with their V
    blast = off + torch.clamp((rows // 32) * 32 + 31, max=Sq - 1)        # the last key a row of the 32-row block can attend
    sl2 = torch.tensor(scale, dtype=F32) * torch.tensor(L2E, dtype=F32)
    if mutant == "scale_twice":
        sl2 = sl2 * torch.tensor(scale, dtype=F32)
    qf = q.float()
    m_run = torch.full((B, Hq, Sq), M_START, dtype=F32)
    l_run = torch.zeros(B, Hq, Sq, dtype=F32)
    O = torch.zeros(B, Hq, Sq, D, dtype=F32)
    nt = (int(kend.max()) + KT - 1) // KT
    for t in range(nt):
        s0 = t * KT
        s = torch.arange(s0, s0 + KT)
        inb = s < Skv
        sc = torch.clamp(s, max=Skv - 1)
        bits = key[:, None, sc] & inb[None, None, :] & (s[None, None, :] < kend[None, :, None])       # [B, Sq, KT]: the staged tile's bits
        if mutant == "ragged_counted":
            bits = bits | ~inb[None, None, :]
        live = bits.any(2)                                               # [B, Sq]: the workgroup loads the tile
        proc = live & (s0 <= blast)[None, :]                             # ... and the row's block computes it
        kt = k[:, :, sc].float()[:, heads]                               # [B, Hq, KT, D]
        vt = v[:, :, sc].float()[:, heads]
        diag = (s[None, :] < (rows + off)[:, None]) if mutant == "diag_exclusive" else (s[None, :] <= (rows + off)[:, None])      # [Sq, KT]
        on = bits & diag[None]
        if mutant == "ragged_counted":
            on = on | (bits & ~inb[None, None, :])
        kt_clean = torch.where(torch.isfinite(kt), kt, zf)               # poisoned rows are replaced by the select below, as in the kernel
        z2 = (qf @ kt_clean.transpose(2, 3)) * sl2                       # [B, Hq, Sq, KT]
        if mutant == "ragged_counted":
            z2 = torch.where(inb[None, None, None, :], z2, zf)
        y = torch.where(on[:, None], z2, ninf)
        if mutant == "masked_zero":                                      # a key-byte mask adds nothing instead of replacing
            y = torch.where((diag[None] & ~bits)[:, None] & inb[None, None, None, :], zf, y)
        vkeep = bits.any(1)                                              # [B, KT]: staged as zeros unless a row of the workgroup attends it
        vt = torch.where((vkeep & inb[None, :])[:, None, :, None] & torch.isfinite(vt), vt, zf)
        mx = y.max(3).values
        m_new = torch.maximum(m_run, mx)
        alpha = torch.exp2(m_run - m_new)
        p = torch.exp2(y - m_new[..., None])
        l_new = l_run * alpha + p.sum(3)
        pv = p.to(dtype).float() @ vt
        O_new = (O if mutant == "no_rescale" else O * alpha[..., None]) + pv
        pr = proc[:, None, :]
        m_run = torch.where(pr, m_new, m_run)
        l_run = torch.where(pr, l_new, l_run)
        O = torch.where(pr[..., None], O_new, O)
        if mutant == "skip_resets_max":
            m_run = torch.where((~live)[:, None, :] & (s0 <= blast)[None, None, :], torch.full((), M_START, dtype=F32), m_run)
    some = l_run > 0
    if mutant == "empty_div0":
        out = O / l_run[..., None]
    else:
        out = torch.where(some[..., None], O * (1.0 / torch.where(some, l_run, torch.ones((), dtype=F32)))[..., None], zf)
    lse = torch.where(some, m_run * torch.tensor(LN2, dtype=F32) + torch.log(torch.where(some, l_run, torch.ones((), dtype=F32))), ninf)
    return out.transpose(1, 2).contiguous().to(dtype), lse


def emulate(B: int, Hq: int, Hkv: int, Sq: int, Skv: int, q_offset: int, D: int, mask_name: str, dtype, mutant=None):
    c = make_case(B, Hq, Hkv, Sq, Skv, q_offset, D, mask_name, dtype)
    return emulate_tensors(c["q"], c["k"], c["v"], c["mask"], c["scale"], q_offset, dtype, mutant=mutant)


def ratios_against(ref, out, lse):
    """(out, lse) worst |d| / bound over the rows with an attended key; inf where a row without one is not exactly (+0, -inf).
    ``out`` [B, Sq, Hq, D], ``lse`` [B, Hq, Sq] or None."""
    out, empty = out.double().cpu(), ref["empty"]            # empty [B, Hq, Sq]
    e_out = empty.transpose(1, 2)                            # [B, Sq, Hq]
    r_lse = 0.0
    if empty.any():
        o = out[e_out]
        if not bool((o == 0).all()) or bool(torch.signbit(o).any()):
            return float("inf"), float("inf")
        if lse is not None and not bool((lse.double().cpu()[empty] == float("-inf")).all()):
            return float("inf"), float("inf")
    if lse is not None:
        r_lse = ratio(lse.cpu()[~empty], ref["lse"][~empty], ref["lse_b"][~empty])
    return ratio(out[~e_out], ref["out"][~e_out], ref["out_b"][~e_out]), r_lse


def ratios(B: int, Hq: int, Hkv: int, Sq: int, Skv: int, q_offset: int, D: int, mask_name: str, dtype, out, lse):
    return ratios_against(reference(B, Hq, Hkv, Sq, Skv, q_offset, D, mask_name, dtype), out, lse)
