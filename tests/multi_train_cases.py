"""Shared by tests/test_multi_train_cpu.py and tests/test_gpu_multi_train.py (not a test module): the backward attention core over a shared
K/V item -- ``share`` chain items (the prompts of a clip) read the K / V of one item and their dK / dV are summed into it.  Seeded
inputs (the families of tests/multi_query_cases.py plus an upstream gradient), the float64 reference, a plain torch emulation of the
kernel's arithmetic with named mutants, and the project's gradient bars.  Pure torch on the CPU.

Shapes: q, o, d_o, dq [kv_items * share, heads, q_rows, 64] (chain item n = i * share + p), k, v, dk, dv [kv_items, heads, kv, 64],
lse [kv_items * share, heads, q_rows] in log2 units of the scaled scores (what AttnArgs::lse holds: log2 sum_j 2^(s_j log2 e / 8)).

The bars are those of tests/test_gpu_backward.py for a gradient tensor: relative Frobenius error 2e-2 and peak error 5e-2 of the
tensor's largest entry in f16, 8 x both in bf16 (8 significand bits instead of 11).

The emulation (``emulate_bwd``) does what csrc/backward.hip does: delta = sum_d dO O in fp32 from the 16-bit tensors, scores and dP as
fp32 products of the 16-bit operands, P = exp2(s sl2 - lse), dS = P (dP - delta) / 8, P and dS rounded to T before the dV / dK / dQ
products, fp32 accumulation over all query blocks and prompt slots, one rounding to T at the end.  Mutants:
    lse_slot0   the lse of prompt slot 0 used for every slot of the K/V item
    dkv_last    dK / dV from the last slot only (an accumulator reset per slot instead of per K/V block)
    dq_slot0    dQ of slot p written to slot 0 (the other slots never written: they keep the zero fill)
Each needs share > 1 and kv > 1 (at kv = 1 the softmax is constant and dQ = dK = 0).  dkv_last and dq_slot0 are far outside the bars on
every family; lse_slot0 on ``peaked`` in both dtypes and on ``mild`` in f16 (the lse of two slots of ``mild`` differ by ~0.1 log2 units,
which the 8 x wider bf16 bars admit)."""
import math

import torch

from multi_query_cases import HD, LOG2E, make_multi

BARS = {torch.float16: (2e-2, 5e-2), torch.bfloat16: (1.6e-1, 4e-1)}   # (relative Frobenius, peak / largest entry)
MUTANTS = ("lse_slot0", "dkv_last", "dq_slot0")
SCALE = 1.0 / math.sqrt(HD)


def make_bwd(kind: str, kv_items: int, share: int, heads: int, q_rows: int, kv: int, dtype=torch.float16):
    """q [kv_items * share, heads, q_rows, 64], k, v [kv_items, heads, kv, 64] (multi_query_cases.make_multi, its first q_rows query rows)
    and an upstream gradient d_o like q, all rounded to ``dtype``."""
    q, k, v = make_multi(kind, kv_items, share, heads, kv, dtype)
    q = q[:, :, :q_rows].contiguous()
    g = torch.Generator().manual_seed(977 * kv + 31 * share + 7 * kv_items + q_rows + (0 if dtype == torch.float16 else 1))
    d_o = (torch.randn(q.shape, generator=g) * 0.5).to(dtype)
    return q, k, v, d_o


def bwd_ref(q, k, v, d_o, share: int):
    """float64: (o, lse, dq, dk, dv).  dq per chain item; dk / dv summed over the ``share`` slots of a K/V item."""
    kv_items = k.shape[0]
    qd, gd = q.double(), d_o.double()
    kd, vd = k.double().repeat_interleave(share, 0), v.double().repeat_interleave(share, 0)
    s = qd @ kd.transpose(-1, -2) * SCALE
    lse = torch.logsumexp(s, -1) * LOG2E
    p = torch.softmax(s, -1)
    o = p @ vd
    delta = (gd * o).sum(-1, keepdim=True)
    ds = p * (gd @ vd.transpose(-1, -2) - delta) * SCALE
    dq = ds @ kd
    dk = (ds.transpose(-1, -2) @ qd).view(kv_items, share, *k.shape[1:]).sum(1)
    dv = (p.transpose(-1, -2) @ gd).view(kv_items, share, *v.shape[1:]).sum(1)
    return o, lse, dq, dk, dv


def emulate_bwd(q, k, v, o, d_o, lse, share: int, mutant=None):
    """The kernel's arithmetic in fp32 / T torch (module docstring).  o: the forward's output rounded to T; lse fp32.  Returns dq, dk, dv in T."""
    T = q.dtype
    N, kv_items = q.shape[0], k.shape[0]
    n = torch.arange(N)
    lse = lse.float()
    if mutant == "lse_slot0":
        lse = lse[(n // share) * share]
    kk, vv = k.float().repeat_interleave(share, 0), v.float().repeat_interleave(share, 0)
    qf, gf = q.float(), d_o.float()
    delta = (gf * o.float()).sum(-1, keepdim=True)
    sl2 = torch.tensor(LOG2E * SCALE, dtype=torch.float32)
    p = torch.exp2((qf @ kk.transpose(-1, -2)) * sl2 - lse[..., None])
    ds = p * (gf @ vv.transpose(-1, -2) - delta) * torch.tensor(SCALE, dtype=torch.float32)
    p16, ds16 = p.to(T).float(), ds.to(T).float()
    dq = ds16 @ kk
    dk = (ds16.transpose(-1, -2) @ qf).view(kv_items, share, *k.shape[1:])
    dv = (p16.transpose(-1, -2) @ gf).view(kv_items, share, *v.shape[1:])
    if mutant == "dkv_last":
        dk, dv = dk[:, -1], dv[:, -1]
    else:
        dk, dv = dk.sum(1), dv.sum(1)
    if mutant == "dq_slot0":
        out = torch.zeros_like(dq).view(kv_items, share, *dq.shape[1:])
        out[:, 0] = dq.view(kv_items, share, *dq.shape[1:])[:, -1]   # every slot lands on slot 0: the last write stays
        dq = out.view_as(dq)
    return dq.to(T), dk.to(T), dv.to(T)


def grad_errors(got, ref, scale_ref=None):
    """(relative Frobenius error, peak error / largest |ref| entry) of a gradient tensor against the float64 reference.  Where the true
    gradient is exactly zero -- dQ and dK at kv = 1: a softmax over one key is constant -- the kernel's value is rounding noise and the
    two errors are taken relative to ``scale_ref`` (the dV reference of the same case, whose entries P^T dO are of the size of the
    terms that cancel in dQ / dK), as tests/test_gpu_backward.py measures the key-bias gradient against the query-bias one."""
    d = got.double() - ref
    den = ref if ref.abs().max().item() > 0 or scale_ref is None else scale_ref
    return (d.norm() / den.norm()).item(), (d.abs().max() / den.abs().max()).item()


def inside(got, ref, dtype, scale_ref=None) -> bool:
    rel, peak = grad_errors(got, ref, scale_ref)
    return rel < BARS[dtype][0] and peak < BARS[dtype][1]

