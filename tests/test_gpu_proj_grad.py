"""``mra_llm_proj_backward`` on the GPU (``-m gpu``), through the C ABI on a 2-layer handle: every case of tests/proj_grad_cases.py against
the float64 references under the derived bounds on EVERY element, outputs between sentinel guards, d_W / d_b added onto a prefill, d_z
written over NaN, each output alone against the joint call, and every refusal of the entry.

Bit for bit, alone against joint: d_z always (no atomics on its path); d_W and d_b wherever the summation order is fixed, i.e. where
launch_gemm_tn does not split the contraction over rows (``tn_splits == 1``: every case below 256 rows).  From 256 rows on the pieces meet
in fp32 atomics whose order the hardware does not fix, so two runs of one call need not agree in the last bit either; there each run is
held to its derived bound, which already counts the pieces."""
import ctypes as C
import functools

import pytest
import torch

import proj_grad_cases as PG

pytestmark = pytest.mark.gpu

GUARD = 4096
MRA_EINVAL, MRA_ESTATE, MRA_ENOMEM = -1, -2, -4      # include/mra.h
SENTINEL = -7.25


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _id(v):
    return str(v).replace("torch.", "")


def _lib_():
    from mraudio_amd import _lib
    return _lib


def _handle(dev, Lh, H, op_dtype):
    from mraudio_amd.qformer import QFormer, QFormerConfig

    return QFormer(QFormerConfig(enc_width=64, hidden=H, heads=H // 64, inter=256, layers=2, vocab=16, max_pos=8, llm_hidden=Lh, op_dtype=op_dtype),
                   device=dev)


@functools.lru_cache(maxsize=None)
def pg_case(rows, Lh, H, dtype, dout_f32):
    """The inputs and the references, computed once: joint call (prefilled), and each parameter gradient alone (same prefill)."""
    c = PG.make_proj(rows, Lh, H, dtype, dout_f32)
    dz = PG.dz_ref(c["d_out"], c["W"])
    dw = PG.dw_ref(c["d_out"], c["z"], dtype, c["dW0"], c["db0"], PG.tn_splits(rows, Lh, H))
    db_alone = PG.dw_ref(c["d_out"], c["z"][:, :64], dtype, None, c["db0"], PG.db_alone_splits(rows, Lh))[2:]
    return c, dz, dw, db_alone


def _guarded(n, fill, dev, dtype=torch.float32):
    g = GUARD // torch.empty((), dtype=dtype).element_size()
    buf = torch.full((g + n + g,), SENTINEL, dtype=dtype, device=dev)
    if fill is not None:
        buf[g: g + n] = fill.reshape(-1).to(dev) if torch.is_tensor(fill) else fill
    return buf, g


def run(qf, c, dev, want_z=True, want_w=True, want_b=True, rows=None, dout_dtype=None, ws_short=0, expect=0, null_z=False, null_dout=False,
        fill=True):
    """One mra_llm_proj_backward call.  d_z starts as NaN, d_W / d_b as the case's prefills (``fill=False``: everything stays the sentinel);
    all three sit between sentinel guards.  Returns (d_z, d_W, d_b) on the CPU, None where not asked for."""
    _lib = _lib_()
    L = _lib.lib()
    R, H = c["z"].shape
    Lh = c["W"].shape[0]
    z, d_out = c["z"].to(dev), c["d_out"].to(dev).contiguous()
    zb, zg = _guarded(R * H, float("nan") if fill else None, dev)
    wb, wg = _guarded(Lh * H, c["dW0"] if fill else None, dev)
    bb, bg = _guarded(Lh, c["db0"] if fill else None, dev)
    before = [t.clone() for t in (zb, wb, bb)]
    dt = _lib.mra_dtype(d_out.dtype) if dout_dtype is None else dout_dtype
    call_rows = R if rows is None else rows
    with torch.cuda.device(dev):
        need = int(L.mra_llm_proj_backward_workspace_bytes(qf._handle, max(R, 1), _lib.mra_dtype(d_out.dtype)))
        assert need % 256 == 0
        ws = torch.zeros(max(need, 256), dtype=torch.uint8, device=dev)
        rc = L.mra_llm_proj_backward(qf._handle, None if null_z else _lib.ptr(z), call_rows, None if null_dout else _lib.ptr(d_out), dt,
                                     C.c_void_p(zb.data_ptr() + GUARD) if want_z else None, C.c_void_p(wb.data_ptr() + GUARD) if want_w else None,
                                     C.c_void_p(bb.data_ptr() + GUARD) if want_b else None, _lib.ptr(ws), need - ws_short, _lib.current_stream())
    torch.cuda.synchronize(dev)
    assert rc == expect, (rc, L.mra_last_error())
    outs = []
    for buf, g, n, want, was in ((zb, zg, R * H, want_z, before[0]), (wb, wg, Lh * H, want_w, before[1]), (bb, bg, Lh, want_b, before[2])):
        o = buf.cpu()
        assert (o[:g] == SENTINEL).all() and (o[-g:] == SENTINEL).all()
        if rc != 0 or not want or call_rows == 0:       # refused, not asked for, or a no-op: not one bit moved
            assert torch.equal(o.view(torch.int32), was.cpu().view(torch.int32))
        outs.append(o[g: g + n] if want and rc == 0 else None)
    return (None if outs[0] is None else outs[0].view(R, H)), (None if outs[1] is None else outs[1].view(Lh, H)), outs[2]


@pytest.mark.parametrize("Lh,H", sorted({(lh, h) for _, lh, h in PG.cases()}))
@pytest.mark.parametrize("dtype", PG.DTYPES, ids=_id)
def test_backward_against_float64(dtype, Lh, H, dev):
    qf = _handle(dev, Lh, H, dtype)
    pushed = None
    for rows in [r for r, lh, h in PG.cases() if (lh, h) == (Lh, H)]:
        for dout_f32 in (True, False):
            c, (z_ref, z_b), (w_ref, w_b, b_ref, b_b), (ba_ref, ba_b) = pg_case(rows, Lh, H, dtype, dout_f32)
            if pushed is None or not torch.equal(pushed, c["W"]):
                qf.push("llm_proj.weight", c["W"])
                qf.push("llm_proj.bias", torch.zeros(Lh))
                pushed = c["W"]
            d_z, d_W, d_b = run(qf, c, dev)
            assert torch.isfinite(d_z).all()                   # the NaN prefill is gone from every row < R
            rs = (PG.ratio(d_z, z_ref, z_b), PG.ratio(d_W, w_ref, w_b), PG.ratio(d_b, b_ref, b_b))
            print(f"proj bwd rows {rows} Lh {Lh} H {H} {_id(dtype)} f32 d_out {dout_f32}: d_z {rs[0]:.3g} d_W {rs[1]:.3g} d_b {rs[2]:.3g}")
            assert max(rs) <= 1.0, (rows, Lh, H, dtype, dout_f32, rs)
            # each output alone
            z1, _, _ = run(qf, c, dev, True, False, False)
            assert torch.equal(z1.view(torch.int32), d_z.view(torch.int32))
            _, w1, _ = run(qf, c, dev, False, True, False)
            _, _, b1 = run(qf, c, dev, False, False, True)
            assert PG.ratio(w1, w_ref, w_b) <= 1.0 and PG.ratio(b1, ba_ref, ba_b) <= 1.0
            if PG.tn_splits(rows, Lh, H) == 1:
                assert torch.equal(w1.view(torch.int32), d_W.view(torch.int32))
                if PG.db_alone_splits(rows, Lh) == 1:
                    assert torch.equal(b1.view(torch.int32), d_b.view(torch.int32))


@pytest.mark.parametrize("Lh", PG.LLM_HIDDEN)
def test_forward_runs_at_the_table_s_llm_hidden(Lh, dev):
    """Handles with llm_hidden a multiple of 64 (not only of 256) exist for the cases above; the forward they also serve is right there:
    fp32 output against float64 of the rounded operands, |y - ref| <= (H + 2) u32 (|z16| |W|^T + |b|) (H exact products and the bias)."""
    dtype, H, rows = torch.bfloat16, PG.HIDDEN, 129
    c = PG.make_proj(rows, Lh, H, dtype, True)
    qf = _handle(dev, Lh, H, dtype)
    b = torch.linspace(-1.0, 1.0, Lh)
    qf.push("llm_proj.weight", c["W"])
    qf.push("llm_proj.bias", b)
    y = qf.llm_proj(c["z"].to(dev)).cpu()
    z16, Wd = c["z"].to(dtype).double(), c["W"].double()
    ref, bound = z16 @ Wd.T + b.double(), (H + 2) * PG.U32 * (z16.abs() @ Wd.abs().T + b.double().abs())
    assert PG.ratio(y, ref, bound) <= 1.0


def test_refusals_leave_the_outputs_untouched(dev):
    _lib = _lib_()
    L = _lib.lib()
    dtype, Lh, H = torch.bfloat16, 256, 256
    c = pg_case(32, Lh, H, dtype, True)[0]
    bare = _handle(dev, Lh, H, dtype)
    run(bare, c, dev, expect=MRA_ESTATE, fill=False)
    assert b"llm_proj not loaded" in L.mra_last_error()
    qf = _handle(dev, Lh, H, dtype)
    qf.push("llm_proj.weight", c["W"])
    qf.push("llm_proj.bias", torch.zeros(Lh))
    run(qf, c, dev, rows=-1, expect=MRA_EINVAL, fill=False)
    assert b"negative rows" in L.mra_last_error()
    run(qf, c, dev, rows=0, expect=0, fill=False)                                   # a no-op
    run(qf, c, dev, dout_dtype=_lib.MRA_F16, expect=MRA_EINVAL, fill=False)        # the other 16-bit type
    assert b"d_out_dtype" in L.mra_last_error()
    run(qf, c, dev, dout_dtype=7, expect=MRA_EINVAL, fill=False)
    assert b"d_out_dtype" in L.mra_last_error()
    run(qf, c, dev, null_z=True, expect=MRA_EINVAL, fill=False)
    assert b"null z or d_out" in L.mra_last_error()
    run(qf, c, dev, null_dout=True, expect=MRA_EINVAL, fill=False)
    assert b"null z or d_out" in L.mra_last_error()
    run(qf, c, dev, ws_short=1, expect=MRA_ENOMEM, fill=False)
    assert b"workspace too small: need" in L.mra_last_error()
    run(qf, c, dev, rows=(1 << 31) // Lh, expect=MRA_EINVAL, fill=False)            # rows * llm_hidden = 2^31
    assert b"exceeds int32" in L.mra_last_error()
    with torch.cuda.device(dev):
        assert L.mra_llm_proj_backward_workspace_bytes(qf._handle, 0, _lib.MRA_F32) == 0
        assert L.mra_llm_proj_backward_workspace_bytes(qf._handle, -3, _lib.MRA_F32) == 0
        f32, op = (int(L.mra_llm_proj_backward_workspace_bytes(qf._handle, 32, d)) for d in (_lib.MRA_F32, _lib.MRA_BF16))
        assert f32 - op == 32 * Lh * 2                                              # the rounded copy of an fp32 d_out
    # llm_hidden not a multiple of 64 never reaches the entry: no such handle can be created
    with pytest.raises(_lib.MraError, match="multiple of 64"):
        _handle(dev, 96, H, dtype)
