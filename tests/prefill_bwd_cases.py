"""Shared by tests/test_prefill_bwd_cases_cpu.py and tests/test_gpu_prefill_bwd.py (not a test module): the case table, seeded inputs rounded
to the operand type, the float64 reference, a DERIVED per-element bound and the fp32 emulation (with named mutants) of the two kernels of
csrc/prefill_attn_bwd.hip behind ``mra_prefill_attention_backward``.  Pure torch on the CPU.  Conventions as tests/prefill_attn_cases.py, whose
generators, mask families and score families are reused: u32 = 2^-24, u = U[T] (2^-11 f16, 2^-8 bf16), every bound worst case and first
order, nothing fitted to GPU output; a sum whose order is not fixed here is bounded as a sum in ANY order at one u32 per link.

The reference is float64 on the ROUNDED operands q, k, v, dO and on the lse (fp32) and out (T) it is GIVEN, so the backward is tested on its
own; the cases take those two from the float64 forward, rounded.

    att(b, i) = {s : s <= q_offset + i, s < Skv, mask[b, s]}            G = Hq / Hkv
    z_is = scale q[b,h,i] . k[b,h/G,s]      p_is = exp(z_is - lse_i) on att, 0 elsewhere and in a row with lse = -inf
    delta_i = dO[b,i,h] . out[b,i,h]        dp_is = dO[b,i,h] . v[b,h/G,s]        ds_is = p_is (dp_is - delta_i)
    dV[b,g,s] = sum_{h in g} sum_i p_is dO[b,i,h]      dQ[b,h,i] = scale sum_s ds_is k[b,h/G,s]      dK[b,g,s] = scale sum_{h in g} sum_i ds_is q[b,h,i]
    dQ of a row that attends nothing and dK / dV of a key no row attends are +0 (asserted as such, not through a bound)

Geometry read off the kernels: the dQ launch gives a workgroup QB = 128 query rows and walks the KT = 32-key tiles in ascending order (nt <=
ceil(Skv / 32)); the dK/dV launch gives a workgroup KB = 128 keys and walks the group's query heads in ascending order, each over the QT =
32-row query tiles in ascending order (ntq = ceil(Sq / 32)); accumulators are fp32 and live across the whole walk.

---- p ------------------------------------------------------------------------------------------------------------------------------------
Products of two 16-bit values are exact in fp32; D of them meet in D - 1 additions inside the MFMAs (any order), then the product with
scale log2e (the constant's two roundings and the product):     e_z[i,s] = (D + 2) u32 |scale| sum_d |q_id| |k_sd|
The exp2 argument z2 - lse log2e: the product with the constant and its rounding (2 u32 |lse|), the subtraction (u32 |z - lse|); the
hardware exp2 (1 ulp; 2 u32 taken); a result below the fp32 normals may be flushed (2^-126 absolute):
    rel[i,s] = e_z + 2 u32 |lse_i| + u32 |z_is - lse_i| + 2 u32                 relative error of p as computed
    ep[i,s]  = p (rel + u) + 2^-126 + [f16] 2^-25                               ... and as the MFMA operand, rounded once to T
---- ds -----------------------------------------------------------------------------------------------------------------------------------
dp: D exact products in D - 1 additions: e_dp = D u32 sum_d |dO_id| |v_sd|.  delta: the same over out, and one addition across the two
half-waves: e_dl = (D + 1) u32 sum_d |dO_id| |out_id|.  The subtraction and the product with p: 2 u32.  One rounding to T:
    eds[i,s] = p (e_dp + e_dl) + |ds| (rel + 2 u32 + u) + 2^-126 |dp - delta| + [f16] 2^-25
---- the sums -----------------------------------------------------------------------------------------------------------------------------
dV, dK: 32 products per tile in any order, then one addition per later tile of the walk over G heads x ntq tiles: N_kv = 32 + G ntq links;
dK is multiplied by scale (one more).  dQ: N_q = 32 + nt links and the product with scale.
    e_dV[s,d] = sum_{h,i} (ep |dO_id| + p |dO_id| N_kv u32)                       dV_b = e + u (|dV| + e) + [f16] F16_SUB
    e_dK[s,d] = |scale| sum_{h,i} (eds |q_id| + |ds| |q_id| (N_kv + 1) u32)       dK_b likewise
    e_dQ[i,d] = |scale| sum_s (eds |k_sd| + |ds| |k_sd| (N_q + 1) u32)            dQ_b likewise
(the last line of each: the output's one rounding, with the f16 subnormal spacing).

Cases.  Sq = Skv = S for S in {1, 2, 31, 32, 33, KB - 1, KB, KB + 1, QB + 1, 2 max(KB, QB) + 3, 1041} and (Sq, Skv, q_offset) in
{(5, 38, 33), (KB + 1, 3 KB, KB - 1), (3, 2 KB + 40, 0)}, each under the seven mask families; D, the five head shapes and B in {1, 3} are
dealt so that every value meets every other (asserted in the CPU test).  K / V hold NaN and +-Inf in masked slots and at or behind
q_offset + Sq (from prefill_attn_cases.make_case); the GPU test also poisons the dO / out rows of query rows that attend nothing.

Mutants (``emulate_tensors(..., mutant=)``): diag_exclusive (s < i), offset_dropped (q_offset taken as 0), delta_omitted, dk_unscaled (scale
missing on dK), group_first_head (the group sum takes only the group's first query head), head_mod (the K/V head of query head h taken as
h % Hkv), masked_ds_kept (a key masked by its byte keeps its p and ds), block_unwritten (a key block without an attended key is left as it
was: NaN here), dead_row_exp (a row with lse = -inf is exponentiated and multiplied by 0 instead of selected)."""
import functools

import torch

import prefill_attn_cases as pa
from train_kernel_cases import F16_SUB, U, U32, _gen, ratio  # noqa: F401  (re-exported for the tests)

F32, F64 = torch.float32, torch.float64
DTYPES = pa.DTYPES
KB, QT, QB, KT = 128, 32, 128, 32             # PREFILL_BWD_KB, PREFILL_BWD_QT, PREFILL_BWD_QB of csrc/kernels.h; the dQ launch's key tile
_S = []
for _s in (1, 2, 31, 32, 33, KB - 1, KB, KB + 1, QB + 1, 2 * max(KB, QB) + 3, 1041):
    if _s not in _S:
        _S.append(_s)
SIZES = tuple((S, S, 0) for S in _S) + ((5, 38, 33), (KB + 1, 3 * KB, KB - 1), (3, 2 * KB + 40, 0))
DIMS, HEADS, BATCHES, MASKS = pa.DIMS, pa.HEADS, pa.BATCHES, pa.MASKS
MUTANTS = ("diag_exclusive", "offset_dropped", "delta_omitted", "dk_unscaled", "group_first_head", "head_mod", "masked_ds_kept",
           "block_unwritten", "dead_row_exp")
L2E = 1.4426950408889634
TINY = 2.0 ** -126


def cases():
    """(B, Hq, Hkv, Sq, Skv, q_offset, D, mask family): every size with every mask family; D, heads and B dealt over them."""
    out = []
    for si, (Sq, Skv, off) in enumerate(SIZES):
        for mi, mask in enumerate(MASKS):
            Hq, Hkv = HEADS[(si + 2 * mi) % 5]
            out.append((BATCHES[(si + mi // 2 + mi // 4) % 2], Hq, Hkv, Sq, Skv, off, DIMS[(si + mi) % 2], mask))
    return out


def workspace_bytes(B: int, Hq: int, Sq: int) -> int:
    """delta, fp32 [B][Hq][Sq], rounded up to 256 bytes."""
    return (4 * B * Hq * Sq + 255) // 256 * 256


def _forward64(q, k, v, mask, scale, q_offset):
    """float64 forward on cleaned operands: dict(att [B, Sq, Skv], kd, vd [B, Hq, Skv, D], z, lse [B, Hq, Sq], out [B, Hq, Sq, D], empty)."""
    B, Hq, Sq, D = q.shape
    Hkv, Skv = k.shape[1], k.shape[2]
    G = Hq // Hkv
    att = pa.attended(mask, B, Sq, Skv, q_offset)
    zero, ninf = torch.zeros((), dtype=F64), torch.full((), float("-inf"), dtype=F64)
    some = att.any(1)[:, None, :, None]                                  # [B, 1, Skv, 1]
    kd = torch.where(some, k.double(), zero).repeat_interleave(G, dim=1)
    vd = torch.where(some, v.double(), zero).repeat_interleave(G, dim=1)
    a4 = att[:, None]
    z = torch.where(a4, scale * (q.double() @ kd.transpose(2, 3)), ninf)
    empty = ~a4.any(3).expand(B, Hq, Sq)
    lse = torch.logsumexp(z, dim=3)
    lse_safe = torch.where(empty, zero, lse)
    p = torch.where(a4, torch.exp(z - lse_safe[..., None]), zero)
    return dict(att=att, kd=kd, vd=vd, z=z, lse=lse, out=p @ vd, empty=empty)


@functools.lru_cache(maxsize=None)
def make_case(B: int, Hq: int, Hkv: int, Sq: int, Skv: int, q_offset: int, D: int, mask_name: str, dtype):
    """prefill_attn_cases.make_case (q, k, v, mask, scale, family) plus dout [B, Sq, Hq, D] in ``dtype``, and the forward it belongs to, from
    float64 and rounded: out [B, Sq, Hq, D] in ``dtype``, lse fp32 [B, Hq, Sq] (-inf for a row that attends nothing)."""
    c = dict(pa.make_case(B, Hq, Hkv, Sq, Skv, q_offset, D, mask_name, dtype))
    gen = _gen(B, Hq, Hkv, Sq, Skv, q_offset, D, MASKS.index(mask_name), 71)
    c["dout"] = torch.randn(B, Sq, Hq, D, generator=gen).to(dtype)
    f = _forward64(c["q"], c["k"], c["v"], c["mask"], c["scale"], q_offset)
    c["out"] = f["out"].transpose(1, 2).contiguous().to(dtype)
    c["lse"] = f["lse"].to(F32)
    return c


def reference_tensors(q, k, v, mask, dout, out, lse, scale: float, q_offset: int, dtype, lse_err=None, out_err=None):
    """float64 values and the bounds of the module docstring for ANY operands: q [B, Hq, Sq, D], k, v [B, Hkv, Skv, D], dout, out
    [B, Sq, Hq, D], lse [B, Hq, Sq] (any float type; what unattended K / V slots and the dout / out rows of a row with lse = -inf hold is
    ignored), mask bool [B, Skv] or None.  ``lse_err`` [B, Hq, Sq] / ``out_err`` [B, Sq, Hq, D]: the kernels were handed an lse / out within
    that of the ones given here (the chained test: the forward entry's own, inside the forward's bounds); d lse moves p by p |d lse| and
    d out moves delta by |dO| . |d out|, which enter rel and e_dl and flow through the same sums.  dict(dq [B, Hq, Sq, D], dk, dv [B, Hkv, Skv, D], dq_b, dk_b, dv_b, empty [B, Hq, Sq], dead [B, Skv])."""
    B, Hq, Sq, D = q.shape
    Hkv, Skv = k.shape[1], k.shape[2]
    G = Hq // Hkv
    u = U[dtype]
    f16 = dtype == torch.float16
    sub = 2.0 ** -25 if f16 else 0.0
    nt, ntq = (Skv + KT - 1) // KT, (Sq + QT - 1) // QT
    N_kv, N_q = 32 + G * ntq, 32 + nt
    zero = torch.zeros((), dtype=F64)
    att = pa.attended(mask, B, Sq, Skv, q_offset)
    res = {n: [] for n in ("dq", "dk", "dv", "dq_b", "dk_b", "dv_b", "empty", "dead")}
    for b in range(B):                                       # one sequence at a time: [Hq, Sq, Skv] float64 temporaries
        lse_b = lse[b].double()                              # [Hq, Sq]
        dead_row = ~(lse_b > float("-inf"))
        a3 = att[b][None] & ~dead_row[:, :, None]            # [Hq, Sq, Skv]
        some = att[b].any(0)[None, :, None]
        kd = torch.where(some, k[b].double(), zero).repeat_interleave(G, dim=0)      # [Hq, Skv, D]
        vd = torch.where(some, v[b].double(), zero).repeat_interleave(G, dim=0)
        qd = q[b].double()
        live3 = ~dead_row[:, :, None]
        dod = torch.where(live3, dout[b].double().transpose(0, 1), zero)              # [Hq, Sq, D]
        od = torch.where(live3, out[b].double().transpose(0, 1), zero)
        lse_safe = torch.where(dead_row, zero, lse_b)
        z = scale * (qd @ kd.transpose(1, 2))
        p = torch.where(a3, torch.exp(torch.where(a3, z, zero) - lse_safe[:, :, None]), zero)
        dp = dod @ vd.transpose(1, 2)
        delta = (dod * od).sum(2)
        dpd = dp - delta[:, :, None]
        ds = p * dpd
        dv_h, dk_h, dq = p.transpose(1, 2) @ dod, scale * (ds.transpose(1, 2) @ qd), scale * (ds @ kd)
        # the bounds
        e_z = (D + 2) * U32 * abs(scale) * (qd.abs() @ kd.abs().transpose(1, 2))
        on = a3.double()
        rel = torch.where(a3, e_z + 2 * U32 * lse_safe.abs()[:, :, None] + U32 * (torch.where(a3, z, zero) - lse_safe[:, :, None]).abs() + 2 * U32, zero)
        if lse_err is not None:
            rel = rel + on * torch.where(dead_row, zero, lse_err[b].double())[:, :, None]
        ep = p * (rel + u) + on * (TINY + sub)
        e_dp = D * U32 * (dod.abs() @ vd.abs().transpose(1, 2))
        e_dl = (D + 1) * U32 * (dod.abs() * od.abs()).sum(2)
        if out_err is not None:
            e_dl = e_dl + (dod.abs() * torch.where(live3, out_err[b].double().transpose(0, 1), zero)).sum(2)
        eds = p * (e_dp + e_dl[:, :, None]) + ds.abs() * (rel + 2 * U32 + u) + on * (TINY * dpd.abs() + sub)
        e_dv = (ep + p * (N_kv * U32)).transpose(1, 2) @ dod.abs()
        e_dk = abs(scale) * ((eds + ds.abs() * ((N_kv + 1) * U32)).transpose(1, 2) @ qd.abs())
        e_dq = abs(scale) * ((eds + ds.abs() * ((N_q + 1) * U32)) @ kd.abs())
        grp = lambda t: t.view(Hkv, G, Skv, D).sum(1)        # noqa: E731
        dv_, dk_, e_dv, e_dk = grp(dv_h), grp(dk_h), grp(e_dv), grp(e_dk)
        fin = lambda val, e: e + u * (val.abs() + e) + (F16_SUB if f16 else 0.0)     # noqa: E731
        for name, t in (("dq", dq), ("dk", dk_), ("dv", dv_), ("dq_b", fin(dq, e_dq)), ("dk_b", fin(dk_, e_dk)), ("dv_b", fin(dv_, e_dv)),
                        ("empty", ~a3.any(2)), ("dead", ~a3.any(0).any(0))):
            res[name].append(t)
    return {name: torch.stack(ts) for name, ts in res.items()}


@functools.lru_cache(maxsize=None)
def reference(B: int, Hq: int, Hkv: int, Sq: int, Skv: int, q_offset: int, D: int, mask_name: str, dtype):
    c = make_case(B, Hq, Hkv, Sq, Skv, q_offset, D, mask_name, dtype)
    return reference_tensors(c["q"], c["k"], c["v"], c["mask"], c["dout"], c["out"], c["lse"], c["scale"], q_offset, dtype)


def emulate_tensors(q, k, v, mask, dout, out, lse, scale: float, q_offset: int, dtype, mutant=None):
    """The two kernels in fp32 torch ops, tile by tile in their order: (dq [B, Hq, Sq, D], dk, dv [B, Hkv, Skv, D]) in ``dtype``."""
    B, Hq, Sq, D = q.shape
    Hkv, Skv = k.shape[1], k.shape[2]
    G = Hq // Hkv
    off = 0 if mutant == "offset_dropped" else q_offset
    heads = torch.arange(Hq) % Hkv if mutant == "head_mod" else torch.arange(Hq) // G
    zf = torch.zeros((), dtype=F32)
    sc = torch.tensor(scale, dtype=F32)
    sl2 = sc * torch.tensor(L2E, dtype=F32)
    key = torch.ones(B, Skv, dtype=torch.bool) if mask is None else mask.reshape(B, Skv).bool()
    klast = min(Skv, off + Sq)
    if mutant == "masked_ds_kept":
        key = torch.ones_like(key)
    klive = key & (torch.arange(Skv) < klast)[None]                      # [B, Skv]: what the dK/dV launch takes for an attended key
    lse = lse.float()
    live = lse > float("-inf")                                           # [B, Hq, Sq]
    lse2 = torch.where(live, lse, zf) * torch.tensor(L2E, dtype=F32)
    clean = lambda t: torch.where(torch.isfinite(t), t, zf)              # noqa: E731  (what is replaced by the kernels' selects)
    qf = q.float()
    kf, vf = clean(k.float())[:, heads], clean(v.float())[:, heads]      # [B, Hq, Skv, D]
    dof = dout.float().transpose(1, 2)
    of = out.float().transpose(1, 2)
    if mutant == "dead_row_exp":
        delta = (dof * of).sum(3)
        lse2 = lse * torch.tensor(L2E, dtype=F32)
    else:
        dof, of = torch.where(live[..., None], dof, zf), torch.where(live[..., None], of, zf)
        delta = (dof * of).sum(3)
    if mutant == "delta_omitted":
        delta = torch.zeros_like(delta)
    rows, cols = torch.arange(Sq), torch.arange(Skv)
    diag = (cols[None, :] < (rows + off)[:, None]) if mutant == "diag_exclusive" else (cols[None, :] <= (rows + off)[:, None])      # [Sq, Skv]

    def p_ds(r0, r1, c0, c1):
        """p, ds (fp32, before the operand rounding) of query rows r0:r1 against keys c0:c1, [B, Hq, r, c]."""
        z2 = (qf[:, :, r0:r1] @ kf[:, :, c0:c1].transpose(2, 3)) * sl2
        on = klive[:, None, None, c0:c1] & diag[None, None, r0:r1, c0:c1]
        e = torch.exp2(z2 - lse2[:, :, r0:r1, None])
        dpd = dof[:, :, r0:r1] @ vf[:, :, c0:c1].transpose(2, 3) - delta[:, :, r0:r1, None]
        if mutant == "dead_row_exp":
            p = e * on.float()
            return p, p * dpd
        on = on & live[:, :, r0:r1, None]
        p = torch.where(on, e, zf)
        return p, torch.where(on, p * dpd, zf)

    # ---- the dQ launch: per row, the key tiles in ascending order up to the diagonal of its 32-row block ----
    dq = torch.zeros(B, Hq, Sq, D, dtype=F32)
    for t in range((min(Skv, off + Sq) + KT - 1) // KT):
        c0, c1 = t * KT, min(t * KT + KT, Skv)
        r0 = max(0, (c0 - off) // 32 * 32)                               # the first 32-row block whose last row reaches the tile
        if r0 >= Sq:
            break
        _, ds = p_ds(r0, Sq, c0, c1)
        dq[:, :, r0:] += ds.to(dtype).float() @ kf[:, :, c0:c1]
    dq = torch.where(live[..., None], dq * sc, zf) if mutant != "dead_row_exp" else dq * sc
    # ---- the dK/dV launch: heads of a group ascending, query tiles ascending ----
    dk, dv = torch.zeros(B, Hkv, Skv, D, dtype=F32), torch.zeros(B, Hkv, Skv, D, dtype=F32)
    members = [[h for h in range(Hq) if int(heads[h]) == g] for g in range(Hkv)]
    for j in range(max(len(m) for m in members)):
        if mutant == "group_first_head" and j > 0:
            break
        gs = [g for g in range(Hkv) if j < len(members[g])]
        hs = [members[g][j] for g in gs]
        for r0 in range(0, Sq, QT):
            r1 = min(r0 + QT, Sq)
            c1 = min(Skv, off + r1)
            p, ds = p_ds(r0, r1, 0, c1)
            dv[:, gs, :c1] += p[:, hs].to(dtype).float().transpose(2, 3) @ dof[:, hs, r0:r1]
            dk[:, gs, :c1] += ds[:, hs].to(dtype).float().transpose(2, 3) @ qf[:, hs, r0:r1]
    if mutant != "dk_unscaled":
        dk = dk * sc
    kl = klive[:, None, :, None]
    dk, dv = torch.where(kl, dk, zf), torch.where(kl, dv, zf)
    if mutant == "block_unwritten":
        nkb = (Skv + KB - 1) // KB
        blk = torch.cat([klive, torch.zeros(B, nkb * KB - Skv, dtype=torch.bool)], 1).view(B, nkb, KB).any(2)
        unwritten = ~blk.repeat_interleave(KB, dim=1)[:, :Skv]
        nan = torch.full((), float("nan"), dtype=F32)
        dk, dv = torch.where(unwritten[:, None, :, None], nan, dk), torch.where(unwritten[:, None, :, None], nan, dv)
    return dq.to(dtype), dk.to(dtype), dv.to(dtype)


def emulate(B: int, Hq: int, Hkv: int, Sq: int, Skv: int, q_offset: int, D: int, mask_name: str, dtype, mutant=None):
    c = make_case(B, Hq, Hkv, Sq, Skv, q_offset, D, mask_name, dtype)
    return emulate_tensors(c["q"], c["k"], c["v"], c["mask"], c["dout"], c["out"], c["lse"], c["scale"], q_offset, dtype, mutant=mutant)


def _plus_zero(t) -> bool:
    return bool((t == 0).all()) and not bool(torch.signbit(t).any())


def ratios_against(ref, dq, dk, dv):
    """(dq, dk, dv) worst |d| / bound over the rows with an attended key / the keys some row attends; inf where a row without one, or a key
    no row attends, is not exactly +0.  ``dq`` [B, Hq, Sq, D], ``dk`` / ``dv`` [B, Hkv, Skv, D]."""
    dq, dk, dv = dq.double().cpu(), dk.double().cpu(), dv.double().cpu()
    empty = ref["empty"]                                                 # [B, Hq, Sq]
    dead = ref["dead"][:, None, :].expand(dk.shape[:3])                  # [B, Hkv, Skv]
    r_q = ratio(dq[~empty], ref["dq"][~empty], ref["dq_b"][~empty]) if _plus_zero(dq[empty]) else float("inf")
    r_k = ratio(dk[~dead], ref["dk"][~dead], ref["dk_b"][~dead]) if _plus_zero(dk[dead]) else float("inf")
    r_v = ratio(dv[~dead], ref["dv"][~dead], ref["dv_b"][~dead]) if _plus_zero(dv[dead]) else float("inf")
    return r_q, r_k, r_v


def ratios(B: int, Hq: int, Hkv: int, Sq: int, Skv: int, q_offset: int, D: int, mask_name: str, dtype, dq, dk, dv):
    return ratios_against(reference(B, Hq, Hkv, Sq, Skv, q_offset, D, mask_name, dtype), dq, dk, dv)
