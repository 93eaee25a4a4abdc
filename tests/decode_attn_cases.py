"""Shared by tests/test_decode_attn_cases_cpu.py and tests/test_gpu_decode_attn.py (not a test module): the case
table, seeded inputs rounded to the operand type, the float64 reference, a DERIVED per-element bound and the fp32 emulation (with named mutants)
of the kernels of csrc/decode_attn.hip behind ``mra_decode_attention``.  Pure torch on the CPU.  Conventions as tests/lm_head_cases.py:
u32 = 2^-24, u = U[T] (2^-11 f16, 2^-8 bf16), every bound worst case and first order, nothing fitted to GPU output; a sum whose order is not
fixed here is bounded as a sum in ANY order at one u32 per link.  The reference is float64 on the ROUNDED operands q, k, v.

    z_s = scale q[b,h] . k[b, h / G, s]   (attended s only),   lse = log sum_s exp z_s,   p = softmax(z),   out = sum_s p_s v[b, h / G, s]
    a row with no attended key: out = +0, lse = -inf (asserted as such, not through a bound)

Geometry read off the kernels: chunks of C = CHUNK keys (nc = ceil(S / C)); per chunk m_c = max z, p~_s = exp2((z_s - m_c) log2e),
l_c = sum p~, acc_c = sum p~ v; the merge walks the chunks in ascending order with w_c = exp2((m_c - M) log2e), M = max m_c.

---- logits -----------------------------------------------------------------------------------------------------------------------------
Products of two 16-bit values are exact in fp32; D of them meet in D - 1 additions (8 fmas per lane, a butterfly over D / 8 lanes), then one
product with scale:                    e_z[s] = (D + 2) u32 |scale| sum_d |q_d| |k_sd|

---- lse --------------------------------------------------------------------------------------------------------------------------------
m_c and M are maxima of computed values (exact, and they cancel: exp(z - m_c) exp(m_c - M) = exp(z - M) whatever m_c is).  The exp2
argument (z - m) log2e: the subtraction, the constant and the product are three roundings, the hardware exp2 is good to 1 ulp (2 u32 taken):
    eta[s]   = 3 u32 |z_s - m_c(s)| + 2 u32        relative error of p~_s beyond e_z
    zeta[c]  = 3 u32 |m_c - M| + 2 u32 + u32       relative error of w_c, and the product with it
    rel[s]   = e_z[s] + eta[s] + zeta[c(s)]        relative error of the term exp(z_s - M) as it enters either sum
The sum l: at most C terms per chunk in any order, nc fmas in the merge: N = C + nc + 2 links.  A relative error of a term moves log l by at
most its softmax share:
    lse_b = sum_s p_s rel[s] + N u32 + u32 (4 |lse - M| + |lse|)          (logf to 2 ulp, twice for first order, and the rounding of M + log l)

---- out --------------------------------------------------------------------------------------------------------------------------------
out_d = A_d / l with A_d = sum_s exp(z_s - M) v_sd, each product p~ v one fma (the same N links), the division correctly rounded (2 u32 taken):
    e[d]     = sum_s p_s |v_sd| (rel[s] + N u32) + |out_d| (sum_s p_s rel[s] + N u32) + 2 u32 |out_d|
    out_b[d] = e + u (|out_d| + e) + 2^-25 [f16: the subnormal spacing]
P is never rounded to 16 bits, so no u-sized term multiplies sum_s p_s |v_sd|: where the sum cancels, the bound is small.

Cases.  S in {1, 63, 64, 65, C - 1, C, C + 1, 2 C + 3, 4 C + 17} x eight mask families; D, (Hq, Hkv) and B are dealt so that every value of
one meets every value of every other (asserted in the CPU test).  K / V live in a longer buffer ([B][Hkv][Smax][k_ss], Smax > S, so the head
stride is not S * D), q and out have padded head strides (``layout``).  Masked K / V slots and everything past S hold NaN and +-Inf.
Mask families: null (no mask), ones, left_pad, holes, mid_chunk (one whole chunk masked in the middle when S > 2 C, the middle third
otherwise), first_chunk (the whole first chunk masked, or all but the last key when S <= C), last_only, row_masked (holes, and the last batch
row has no attended key at all).
Logit families, by row (b Hq + h + offset) % 6: mild; peaked on the row's first attended key (about 30 above the rest); peaked on its LAST
attended key (in the ragged last chunk); shifted +90; shifted -90 (column 0 of K is 4 everywhere, q_0 = +-90 / (4 scale): fp32 exp(+-90)
overflows / flushes, so a kernel without the running maximum cannot pass); all-equal (q = 0: out = the mean of the attended V rows,
lse = log count).

Mutants (``emulate(..., mutant=)``): masked_zero (masked keys enter as zero logits with zero V), first_chunk_max (the chunk maxima are not
merged: every chunk's partials are taken as relative to chunk 0's maximum), last_chunk_dropped, ragged_counted (the tail past S of the last
chunk enters as zero logits with zero V), scale_twice, head_mod (the K/V head of query head h taken as h % Hkv instead of h / G), p_rounded
(P rounded to the operand type in front of P V), empty_chunk_weight1 (a chunk with no attended key is not skipped: its exp(-inf - (-inf)) is
"repaired" to 1, so each of its keys counts 1 into l at weight 1)."""
import functools
import math

import torch

from train_kernel_cases import F16_SUB, U, U32, _gen, ratio  # noqa: F401  (re-exported for the tests)

F32, F64 = torch.float32, torch.float64
DTYPES = (torch.float16, torch.bfloat16)
CHUNK = 256                                   # keys per workgroup: DECODE_CHUNK of csrc/kernels.h
C = CHUNK
SEQS = (1, 63, 64, 65, C - 1, C, C + 1, 2 * C + 3, 4 * C + 17)
DIMS = (64, 128)
HEADS = ((4, 4), (4, 2), (8, 2), (8, 1), (3, 3))
BATCHES = (1, 3)
MASKS = ("null", "ones", "left_pad", "holes", "mid_chunk", "first_chunk", "last_only", "row_masked")
FAMILIES = ("mild", "peak_first", "peak_last", "plus90", "minus90", "equal")
MUTANTS = ("masked_zero", "first_chunk_max", "last_chunk_dropped", "ragged_counted", "scale_twice", "head_mod", "p_rounded", "empty_chunk_weight1")
L2E = 1.4426950408889634


def cases():
    """(B, Hq, Hkv, S, D, mask family): every S with every mask family; D, heads and B dealt over them."""
    out = []
    for si, S in enumerate(SEQS):
        for mi, mask in enumerate(MASKS):
            Hq, Hkv = HEADS[(si + 2 * mi) % 5]
            out.append((BATCHES[(si + mi // 2 + mi // 4) % 2], Hq, Hkv, S, DIMS[(si + mi) % 2], mask))
    return out


def chunks(S: int) -> int:
    return (S + C - 1) // C


def up256(n: int) -> int:
    return (n + 255) // 256 * 256


def workspace_bytes(B: int, Hq: int, S: int, D: int) -> int:
    """include/mra.h: 2 up(4 B Hq C) + up(4 B Hq C D) with C = ceil(S / 256) chunks."""
    rows = B * Hq * chunks(S)
    return 2 * up256(4 * rows) + up256(4 * rows * D)


def layout(B: int, Hq: int, Hkv: int, S: int, D: int):
    """dict(Smax, k_ss, v_ss, q_sh, o_sh): K / V as views of a longer, possibly pitched buffer, q / out with padded head strides (elements)."""
    return dict(Smax=S + 3 + 8 * (S % 3), k_ss=D + (8 if S % 2 else 0), v_ss=D + (16 if (S + Hq) % 3 == 0 else 0), q_sh=D + 8 * (1 + S % 2),
                o_sh=D + 8 * (1 + Hq % 3))


def make_mask(name: str, B: int, S: int, gen):
    """bool [B, S] (True = attend) or None."""
    if name == "null":
        return None
    m = torch.ones(B, S, dtype=torch.bool)
    if name == "left_pad":
        for b in range(B):
            m[b, :min(S - 1, 5 + 11 * b)] = False
    elif name in ("holes", "row_masked"):
        m = torch.rand(B, S, generator=gen) >= 0.25
        m[:, (S - 1) // 2] = True
        if name == "row_masked":
            m[B - 1] = False
    elif name == "mid_chunk":
        if S > 2 * C:
            m[:, C:2 * C] = False
        else:
            m[:, S // 3: max(S // 3, 2 * S // 3)] = False
            m[:, 0] = True
    elif name == "first_chunk":
        m[:, :min(C, S - 1)] = False
    elif name == "last_only":
        m[:] = False
        m[:, S - 1] = True
    return m


def _poison(t: torch.Tensor, where: torch.Tensor) -> None:
    """NaN, +Inf, -Inf in turn over the elements of ``t`` selected by the boolean ``where`` (same shape)."""
    n = int(where.sum())
    if n:
        vals = torch.tensor([float("nan"), float("inf"), float("-inf")]).repeat((n + 2) // 3)[:n]
        t[where] = vals.to(t.dtype)


@functools.lru_cache(maxsize=None)
def make_case(B: int, Hq: int, Hkv: int, S: int, D: int, mask_name: str, dtype):
    """q [B, Hq, D], k, v [B, Hkv, S, D] in ``dtype`` (masked slots poisoned), mask bool [B, S] or None, scale (a Python float that is exact
    in fp32), family [B][Hq]."""
    gen = _gen(B, Hq, Hkv, S, D, MASKS.index(mask_name), 47)
    G = Hq // Hkv
    scale = float(torch.tensor(D ** -0.5, dtype=F32))
    mask = make_mask(mask_name, B, S, gen)
    att = torch.ones(B, S, dtype=torch.bool) if mask is None else mask
    k = torch.randn(B, Hkv, S, D, generator=gen)
    k[..., 0] = 4.0
    k = k.to(dtype)
    v = torch.randn(B, Hkv, S, D, generator=gen).to(dtype)
    q = torch.randn(B, Hq, D, generator=gen)
    off = (S + D // 64) % 6
    family = [[FAMILIES[(b * Hq + h + off) % 6] for h in range(Hq)] for b in range(B)]
    kd = k.double()
    for b in range(B):
        idx = torch.nonzero(att[b]).squeeze(1)
        for h in range(Hq):
            fam = family[b][h]
            if fam in ("peak_first", "peak_last") and idx.numel():
                d = kd[b, h // G, int(idx[0] if fam == "peak_first" else idx[-1])].clone()
                d[0] = 0.0                                   # the shared column would lift every logit alike
                q[b, h] += (30.0 / scale) * (d / (d * d).sum()).float()
            elif fam in ("plus90", "minus90"):
                q[b, h, 0] = (90.0 if fam == "plus90" else -90.0) / (4.0 * scale)
            elif fam == "equal":
                q[b, h] = 0.0
    dead = ~att[:, None, :, None].expand(B, Hkv, S, D)
    _poison(k, dead)
    _poison(v, dead.roll(1, -1) | dead)
    return dict(q=q.to(dtype), k=k, v=v, mask=mask, scale=scale, family=family)


def reference_tensors(q, k, v, mask, scale: float, dtype):
    """float64 values and the bounds of the module docstring for ANY operands: q [B, Hq, D], k, v [B, Hkv, S, D] (16-bit values; what masked
    slots hold is ignored), mask bool [B, S] or None.  dict(out [B, Hq, D], lse [B, Hq], out_b, lse_b, empty bool [B, Hq])."""
    B, Hq, D = q.shape
    Hkv, S = k.shape[1], k.shape[2]
    G = Hq // Hkv
    u = U[dtype]
    att = torch.ones(B, S, dtype=torch.bool) if mask is None else mask.reshape(B, S).bool()
    a4 = att[:, None, :, None]
    kd = torch.where(a4, k.double(), torch.zeros((), dtype=F64)).repeat_interleave(G, dim=1)      # [B, Hq, S, D]
    vd = torch.where(a4, v.double(), torch.zeros((), dtype=F64)).repeat_interleave(G, dim=1)
    qd = q.double()
    a3 = att[:, None, :].expand(B, Hq, S)
    ninf = torch.full((), float("-inf"), dtype=F64)
    z = torch.where(a3, scale * torch.einsum("bhd,bhsd->bhs", qd, kd), ninf)
    e_z = (D + 2) * U32 * abs(scale) * torch.einsum("bhd,bhsd->bhs", qd.abs(), kd.abs())
    empty = ~att.any(1)[:, None].expand(B, Hq)
    lse = torch.logsumexp(z, dim=2)
    lse_safe = torch.where(empty, torch.zeros((), dtype=F64), lse)
    p = torch.where(a3, torch.exp(z - lse_safe[:, :, None]), torch.zeros((), dtype=F64))
    out = torch.einsum("bhs,bhsd->bhd", p, vd)
    nc = chunks(S)
    pad = nc * C - S
    zc = torch.cat([z, ninf.expand(B, Hq, pad)], 2).view(B, Hq, nc, C)
    m_c = zc.max(3).values                                                                   # -inf for a chunk with no attended key
    M = m_c.max(2).values
    m_s = m_c.repeat_interleave(C, dim=2)[:, :, :S]
    zero = torch.zeros((), dtype=F64)
    eta = torch.where(a3, 3 * U32 * (z - m_s).abs() + 2 * U32, zero)
    zeta = torch.where(a3, 3 * U32 * (m_s - M[:, :, None]).abs() + 3 * U32, zero)
    rel = torch.where(a3, e_z, zero) + eta + zeta
    N = C + nc + 2
    prel = (p * rel).sum(2)
    lse_b = prel + N * U32 + U32 * (4 * (lse_safe - torch.where(empty, zero, M)).abs() + lse_safe.abs())
    e = (torch.einsum("bhs,bhsd->bhd", p * (rel + N * U32), vd.abs()) + out.abs() * (prel + N * U32)[:, :, None] + 2 * U32 * out.abs())
    out_b = e + u * (out.abs() + e) + (F16_SUB if dtype == torch.float16 else 0.0)
    return dict(out=out, lse=lse, out_b=out_b, lse_b=lse_b, empty=empty)


@functools.lru_cache(maxsize=None)
def reference(B: int, Hq: int, Hkv: int, S: int, D: int, mask_name: str, dtype):
    c = make_case(B, Hq, Hkv, S, D, mask_name, dtype)
    return reference_tensors(c["q"], c["k"], c["v"], c["mask"], c["scale"], dtype)


def _exp2(x):
    return torch.exp2(x.to(F32))


def emulate_tensors(q, k, v, mask, scale: float, dtype, mutant=None):
    """The kernels in fp32 torch ops, chunk by chunk and merged in ascending order: (out [B, Hq, D] in ``dtype``, lse f32 [B, Hq])."""
    B, Hq, D = q.shape
    Hkv, S = k.shape[1], k.shape[2]
    G = Hq // Hkv
    att = torch.ones(B, S, dtype=torch.bool) if mask is None else mask.reshape(B, S).bool()
    a4 = att[:, None, :, None]
    heads = torch.arange(Hq) % Hkv if mutant == "head_mod" else torch.arange(Hq) // G
    zf = torch.zeros((), dtype=F32)
    kf = torch.where(a4, k.float(), zf)[:, heads]                                            # [B, Hq, S, D]; a masked key is never read
    vf = torch.where(a4, v.float(), zf)[:, heads]
    qf = q.float()
    sc = torch.tensor(scale, dtype=F32)
    l2e = torch.tensor(L2E, dtype=F32)
    ninf = torch.full((), float("-inf"), dtype=F32)
    nc = chunks(S)
    ms, ls, accs = [], [], []
    for c in range(nc):
        s0, s1 = c * C, min(S, c * C + C)
        z = sc * torch.einsum("bhd,bhsd->bhs", qf, kf[:, :, s0:s1])
        if mutant == "scale_twice":
            z = sc * z
        on = att[:, None, s0:s1].expand(B, Hq, s1 - s0)
        z = torch.where(on, z, zf if mutant == "masked_zero" else ninf)
        vc = vf[:, :, s0:s1]
        if mutant == "ragged_counted" and s1 - s0 < C:
            z = torch.cat([z, torch.zeros(B, Hq, C - (s1 - s0), dtype=F32)], 2)
            vc = torch.cat([vc, torch.zeros(B, Hq, C - (s1 - s0), D, dtype=F32)], 2)
        m = z.max(2).values
        p = torch.where(z > ninf, _exp2((z - m[:, :, None]) * l2e), zf)
        l = p.sum(2)
        if mutant == "p_rounded":
            p = p.to(dtype).float()
        ms.append(m)
        ls.append(l)
        accs.append(torch.einsum("bhs,bhsd->bhd", p, vc))
        if mutant == "empty_chunk_weight1":
            ls[-1] = torch.where(m > ninf, l, torch.full_like(l, float(s1 - s0)))
    if mutant == "last_chunk_dropped" and nc > 1:
        ms, ls, accs = ms[:-1], ls[:-1], accs[:-1]
    mt = torch.stack(ms, 2)
    M = mt[:, :, 0] if mutant == "first_chunk_max" else mt.max(2).values
    l = torch.zeros(B, Hq, dtype=F32)
    acc = torch.zeros(B, Hq, D, dtype=F32)
    for m, lc, ac in zip(ms, ls, accs):
        if mutant == "first_chunk_max":
            w = torch.where(m > ninf, torch.ones((), dtype=F32), zf)
        elif mutant == "empty_chunk_weight1":
            w = torch.where(m > ninf, _exp2((m - M) * l2e), torch.where(M > ninf, torch.ones((), dtype=F32), zf))
        else:
            w = torch.where(m > ninf, _exp2((m - M) * l2e), zf)
        l = l + lc * w
        acc = acc + ac * w[:, :, None]
    some = M > ninf
    out = torch.where(some[:, :, None], acc / torch.where(some, l, torch.ones((), dtype=F32))[:, :, None], zf)
    lse = torch.where(some, M + torch.log(torch.where(some, l, torch.ones((), dtype=F32))), ninf)
    return out.to(dtype), lse


def emulate(B: int, Hq: int, Hkv: int, S: int, D: int, mask_name: str, dtype, mutant=None):
    c = make_case(B, Hq, Hkv, S, D, mask_name, dtype)
    return emulate_tensors(c["q"], c["k"], c["v"], c["mask"], c["scale"], dtype, mutant=mutant)


def ratios_against(ref, out, lse):
    """(out, lse) worst |d| / bound over the rows with an attended key; inf where a row without one is not exactly (+0, -inf)."""
    out, empty = out.double().cpu(), ref["empty"]
    r_lse = 0.0
    if empty.any():
        o = out[empty]
        if not bool((o == 0).all()) or bool(torch.signbit(o).any()):
            return float("inf"), float("inf")
        if lse is not None and not bool((lse.double().cpu()[empty] == float("-inf")).all()):
            return float("inf"), float("inf")
    live = ~empty
    if lse is not None:
        r_lse = ratio(lse.cpu()[live], ref["lse"][live], ref["lse_b"][live])
    return ratio(out[live], ref["out"][live], ref["out_b"][live]), r_lse


def ratios(B: int, Hq: int, Hkv: int, S: int, D: int, mask_name: str, dtype, out, lse):
    return ratios_against(reference(B, Hq, Hkv, S, D, mask_name, dtype), out, lse)
