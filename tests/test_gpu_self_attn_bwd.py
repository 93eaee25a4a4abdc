"""``-m gpu``: the attention backward core (``attn_bwd_mfma_kernel``) in the masked self-attention form of ``mra_qformer_backward`` -- Q, K, V
in place in the packed ``[items][S][3 H]`` rows, dQ | dK | dV into rows of the same layout, an int64 key mask, q_rows = kv_len = S -- through
``mra_debug_self_attention_bwd`` (the training step's own argument builder) against the float64 reference of
``tests/self_attn_bwd_cases.py`` under its DERIVED per-element bound: |d| / bound <= 1 for every element of dQ, dK and dV.  Nothing in the
bound was fitted to this file's output; the fp32 emulation sits inside it and the named mutants far outside
(tests/test_self_attn_bwd_cases_cpu.py).  Every test prints its worst ratios.

What each S exercises: 33 / 65 a one-row ragged block; 129 one active wave in the second round of key blocks; 160 the longest production
prompt; 161 two active waves and a ragged tail; 257 three rounds; 448 the LDS limit (14 query blocks)."""
import functools
import time

import pytest
import torch

import qformer_kernel_cases as K
import self_attn_bwd_cases as SB
from mraudio_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 256     # elements on either side of the output (a multiple of 8: 16-byte alignment survives)
DT = {"f16": torch.float16, "bf16": torch.bfloat16}
CHAINED_S = (33, 160, 257)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def case(kind, items, heads, S, dtype, mask_kind, chained=False):
    """Inputs, float64 gradients and bounds of one case, computed once and left unchanged."""
    return SB.build(kind, items, heads, S, dtype, mask_kind, chained=chained)


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def guarded(shape, dtype, dev):
    """A NaN-filled output of ``shape`` between two NaN guards: (whole buffer, the output's view)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((GUARD + n + GUARD,), float("nan"), dtype=dtype, device=dev)
    return buf, buf[GUARD: GUARD + n].view(shape)


def run_bwd(c, dev, fwd_ctx=None, fwd_lse=None, mask="case", expect=0, **override):
    """One call of the entry on the case's inputs (``fwd_ctx`` [items, S, H] / ``fwd_lse`` on the device: the forward kernel's instead of the case's;
    ``override``: an argument replaced, for the refusals).  Checks the guards, that a refused call wrote nothing and a successful one every
    element, and that the inputs came back bit for bit.  Returns (dq, dk, dv) on the CPU, each [items, heads, S, 64]."""
    L = _lib.lib()
    items, heads, S, _ = c.q.shape
    mask = c.mask if isinstance(mask, str) else mask
    qkv = K.pack_qkv(c.q, c.k, c.v).to(dev)
    ctx = SB.pack_rows(c.o).to(dev) if fwd_ctx is None else fwd_ctx
    d_ctx = SB.pack_rows(c.d_o).to(dev)
    lse_d = c.lse.contiguous().to(dev) if fwd_lse is None else fwd_lse
    mk = mask.contiguous().to(dev) if mask is not None else None
    before = [t.clone() for t in (qkv, ctx, d_ctx, lse_d)]
    buf, dqkv = guarded(qkv.shape, c.q.dtype, dev)
    args = dict(qkv=_lib.ptr(qkv), mask=_lib.ptr(mk) if mk is not None else None, ctx=_lib.ptr(ctx), d_ctx=_lib.ptr(d_ctx), lse=_lib.ptr(lse_d),
                dtype=_lib.mra_dtype(c.q.dtype), items=items, S=S, heads=heads, dqkv=_lib.ptr(dqkv))
    args.update(override)
    with torch.cuda.device(dev):
        rc = L.mra_debug_self_attention_bwd(args["qkv"], args["mask"], args["ctx"], args["d_ctx"], args["lse"], args["dtype"], args["items"],
                                            args["S"], args["heads"], args["dqkv"], _lib.current_stream())
    torch.cuda.synchronize(dev)
    assert rc == expect, (rc, L.mra_last_error())
    assert torch.isnan(buf[:GUARD]).all().item() and torch.isnan(buf[-GUARD:]).all().item(), "a guard was written"
    if rc != 0:
        assert torch.isnan(buf).all().item(), "a refused call wrote"
    else:       # every column of the three thirds, for every head and every row < S
        unwritten = torch.isnan(dqkv)
        assert not unwritten.any().item(), f"{int(unwritten.sum())} elements of dqkv left unwritten or NaN, first at {unwritten.nonzero()[0].tolist()}"
    for t, b in zip((qkv, ctx, d_ctx, lse_d), before):
        assert torch.equal(_bits(t), _bits(b)), "an input was written"
    return tuple(t.contiguous() for t in SB.unpack_dqkv(dqkv.cpu(), heads))


def run_fwd(c, dev):
    """ctx [items, S, H] in T and lse [items, heads, S] fp32 of ``mra_debug_self_attention`` on the case's inputs, left on the device."""
    L = _lib.lib()
    items, heads, S, _ = c.q.shape
    qkv = K.pack_qkv(c.q, c.k, c.v).to(dev)
    mk = c.mask.contiguous().to(dev) if c.mask is not None else None
    ctx = torch.full((items, S, heads * 64), float("nan"), dtype=c.q.dtype, device=dev)
    lse = torch.full((items, heads, S), float("nan"), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = L.mra_debug_self_attention(_lib.ptr(qkv), _lib.ptr(mk) if mk is not None else None, _lib.mra_dtype(c.q.dtype), items, S, heads, _lib.ptr(ctx),
                                        _lib.ptr(lse), _lib.current_stream())
    torch.cuda.synchronize(dev)
    assert rc == 0, L.mra_last_error()
    return ctx, lse


# ---- 1. the core against float64 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("S", SB.BWD_S)
def test_core_against_float64(S, dt, dev):
    """items 1 and 3, heads 2 and 3, both families, all five mask kinds; o and lse are the float64 values rounded once."""
    t0 = time.time()
    worst, failures = [(0.0, None)] * 3, []
    for items in (1, 3):
        for heads in (2, 3):
            for kind in SB.FAMILIES:
                for mk in SB.MASK_KINDS:
                    c = case(kind, items, heads, S, DT[dt], mk)
                    r = SB.ratios(run_bwd(c, dev), c.ref, c.bound)
                    worst = [max(w, (x, (items, heads, kind, mk))) for w, x in zip(worst, r)]
                    failures += [(name, items, heads, kind, mk, round(x, 3)) for name, x in zip(("dq", "dk", "dv"), r) if not x <= 1.0]
    print(f"self-attention backward {dt} S={S}: |d| / bound dq {worst[0][0]:.3f} at {worst[0][1]}, dk {worst[1][0]:.3f} at {worst[1][1]}, "
          f"dv {worst[2][0]:.3f} at {worst[2][1]}  [{time.time() - t0:.1f} s]")
    assert not failures, failures


# ---- 2. chained with the forward kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("S", CHAINED_S)
def test_chained_with_the_forward_kernel(S, dt, dev):
    """ctx and lse as ``mra_debug_self_attention`` leaves them on the GPU feed the backward: what the two kernels share without stating it
    (lse in log2 units with the mask included) holds, inside the bound with the forward's own ctx and lse bounds added."""
    worst, failures = [(0.0, None)] * 3, []
    for kind in SB.FAMILIES:
        for mk in SB.MASK_KINDS:
            c = case(kind, 3, 2, S, DT[dt], mk, True)
            ctx, lse = run_fwd(c, dev)
            r = SB.ratios(run_bwd(c, dev, fwd_ctx=ctx, fwd_lse=lse), c.ref, c.chained_bound)
            worst = [max(w, (x, (kind, mk))) for w, x in zip(worst, r)]
            failures += [(name, kind, mk, round(x, 3)) for name, x in zip(("dq", "dk", "dv"), r) if not x <= 1.0]
    print(f"forward -> backward {dt} S={S}: |d| / bound dq {worst[0][0]:.3f} at {worst[0][1]}, dk {worst[1][0]:.3f} at {worst[1][1]}, "
          f"dv {worst[2][0]:.3f} at {worst[2][1]}")
    assert not failures, failures


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_every_column_of_the_three_thirds_is_written_and_nothing_else(dt, dev):
    """``run_bwd`` holds dqkv NaN-filled between two NaN guards and asserts, after every successful call of this file, that the guards are
    intact and no element inside is NaN; here on its own at three heads, a ragged last block and a mask that leaves rows without an attended
    text key: a store into a neighbouring third or head would leave its own column NaN."""
    for S, mk in ((33, "zero_row"), (161, "holes")):
        c = case("peaked", 3, 3, S, DT[dt], mk)
        got = run_bwd(c, dev)
        assert all(torch.isfinite(g).all().item() for g in got)
        assert max(SB.ratios(got, c.ref, c.bound)) <= 1.0


# ---- 3. no mask is a mask of ones --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_a_null_mask_is_a_mask_of_ones(dt, dev):
    """dK and dV accumulate in registers in a fixed order: bit for bit.  dQ crosses the key blocks through LDS float adds in no fixed order:
    inside the bound."""
    for S in (41, 160):
        c = case("mild", 3, 2, S, DT[dt], "null")
        assert c.mask is None
        dq0, dk0, dv0 = run_bwd(c, dev)
        dq1, dk1, dv1 = run_bwd(c, dev, mask=torch.ones(3, S, dtype=torch.int64))
        assert torch.equal(dk0.view(torch.int16), dk1.view(torch.int16)) and torch.equal(dv0.view(torch.int16), dv1.view(torch.int16)), S
        assert SB.worst_ratio(dq1, c.ref[0], c.bound[0]) <= 1.0 and SB.worst_ratio(dq0, c.ref[0], c.bound[0]) <= 1.0, S


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(dev):
    """MRA_EINVAL with a message and an untouched output (the S = 449 buffers have the size that S claims)."""
    L = _lib.lib()
    c = case("mild", 1, 2, 33, torch.float16, "ragged")
    for name in ("qkv", "ctx", "d_ctx", "lse", "dqkv"):
        run_bwd(c, dev, expect=-1, **{name: None})
        assert b"null" in L.mra_last_error(), name
    for name in ("items", "S", "heads"):
        run_bwd(c, dev, expect=-1, **{name: 0})
        assert b"sizes" in L.mra_last_error(), name
    run_bwd(c, dev, expect=-1, dtype=_lib.MRA_F32)
    assert b"dtype" in L.mra_last_error()
    for dtype in DT.values():
        big = case("mild", 1, 2, SB.MAX_S + 1, dtype, "ones")
        run_bwd(big, dev, expect=-1)
        assert b"448" in L.mra_last_error()
