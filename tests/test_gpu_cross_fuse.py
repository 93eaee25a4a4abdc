"""``-m gpu``: the fused query launch of the folded cross-attention (csrc/fold.hip fold_query_kernel; mra_qformer_set_option "cross_fuse").

Launch level: ``mra_debug_fold_query`` on the cases of tests/cross_fuse_cases.py, f16 and bf16, every buffer between sentinel guards -- against
float64 under that file's derived bounds, and BIT FOR BIT against the two launches it replaces (the cross query projection and the per-head
Q' GEMM, each through ``mra_debug_gemm`` with the forward's own descriptors).

Forward level: the small Q-Former of tests/test_gpu_raw_features.py (4 layers = two cross layers, E = 704, folded mode forced) with raw
features and with the normalised copy: with the option on the outputs equal those of mask 0 bit for bit, the launch counters show one fused
launch per cross layer in place of a cross query GEMM and a Q' GEMM; a probing forward and a split-precision forward never take the launch.

Bit 2 (the row factors inside the P . enc launch, mra_gemm_desc.ps_stats): statistics from REAL scores launches (diffuse and peaked inputs,
kv 176 / 300 / 1000), then P . enc twice -- mra_debug_fold_rowfactor + the pscale launch, and the statistics-fed launch on a copy of P~ whose
unwritten columns still hold NaN -- bit for bit equal and inside the float64 bound; in a forward no fold_rowfactor launch is issued.

Bit 4 (the context GEMM on the 64 x 64 tile with 128-deep K steps): the launch at M = 96 and 1024 against float64 and against the present
64 x 128 tile bit for bit, and a forward at E = 1408 with 16 items, where the forward takes that tile."""
import ctypes
import time

import pytest
import torch

import cross_fuse_cases as X
from mraudio_amd import _lib as L
from test_gpu_qformer_kernels import DEV, Buf, _bits, _ok, _stream, _view
from test_gpu_raw_features import _features, _run
from test_gpu_parity import build_qformer, oracle_cfg

pytestmark = pytest.mark.gpu
GF_V1_64, GF_V1_128, GF_K128_64x128, GF_K128_64x64, EPI_OP, GT_AUTO, GT_64, GT_128, GT_K128_64x128 = 0, 1, 7, 10, 0, 0, 1, 2, 6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device(DEV)


# =========================================================================================================================================
# launch level
# =========================================================================================================================================
def _desc(**kw):
    d = L.mra_gemm_desc()
    d.struct_bytes = ctypes.sizeof(L.mra_gemm_desc)
    for k, v in kw.items():
        if k.endswith("_view"):
            getattr(d, k)[:] = v
        else:
            setattr(d, k, v)
    return d


def _two_launches(x, wq, bq, wk, items, Lt, dtype):
    """Steps 5 and 6a as mra_abi.hip issues them without the option: Q [M][H] (automatic tile), then Q' per head (batch = heads, K = 64)."""
    M = items * X.Q
    qc = Buf(M * X.H, dtype)
    qp = Buf(items * X.HEADS * X.Q * X.E, dtype)
    nb = lambda b: b.numel * b.inner.element_size()
    d5 = _desc(A=x.inner.data_ptr(), a_bytes=nb(x), W=wq.inner.data_ptr(), w_bytes=nb(wq), bias=bq.inner.data_ptr(), bias_bytes=nb(bq),
               C=qc.inner.data_ptr(), c_bytes=nb(qc), a_view=X.x_view(Lt), c_view=(0, M, X.H), M=M, N=X.H, K=X.H, tile_cfg=GT_AUTO)
    _ok(L.lib().mra_debug_gemm(d5, 1, EPI_OP, L.mra_dtype(dtype), _stream()), "cross q gemm")
    R = X.HEADS * X.Q
    d6 = _desc(A=qc.inner.data_ptr(), a_bytes=nb(qc), W=wk.inner.data_ptr(), w_bytes=nb(wk), C=qp.inner.data_ptr(), c_bytes=nb(qp),
               a_view=(0, M, X.H), c_view=(R * X.E, X.Q, X.E), M=M, N=X.E, K=64, batch=X.HEADS, a_bs=64, w_bs=X.E * 64, c_bs_bytes=X.Q * X.E * 2,
               tile_cfg=GT_128 if M % 128 == 0 and X.E % 128 == 0 else GT_64)
    _ok(L.lib().mra_debug_gemm(d6, 1, EPI_OP, L.mra_dtype(dtype), _stream()), "fold q' gemm")
    return qp.result(True, "q' of the two launches")


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("Lt", X.TEXT)
@pytest.mark.parametrize("items", X.ITEMS)
@pytest.mark.parametrize("kind", X.KINDS)
def test_fused_query_launch(kind, items, Lt, dt, dev):
    t0 = time.time()
    dtype = X.DTYPES[dt]
    wq_, bq_, wk_ = X.weights(kind, dt)
    x_ = X.inputs(kind, items, Lt, dt)
    x, wq, bq, wk = (Buf(t.numel(), t.dtype, t) for t in (x_, wq_, bq_, wk_))
    qp = Buf(items * X.HEADS * X.Q * X.E, dtype)
    nb = lambda b: b.numel * b.inner.element_size()
    before = L.lib().mra_debug_fold_query_launches()
    _ok(L.lib().mra_debug_fold_query(x.ptr, _view(*X.x_view(Lt)), nb(x), wq.ptr, nb(wq), bq.ptr, nb(bq), wk.ptr, nb(wk), qp.ptr, nb(qp), items * X.Q,
                                     X.H, X.E, X.Q, X.HEADS, L.mra_dtype(dtype), _stream()), "mra_debug_fold_query")
    assert L.lib().mra_debug_fold_query_launches() - before == 1
    for name, b in (("x", x), ("w_q", wq), ("b_q", bq), ("w_k", wk)):
        b.unchanged(name)
    got = qp.result(True, "q_prime").view(items, X.HEADS * X.Q, X.E)
    r = X.worst_ratio(got, kind, items, Lt, dt)
    two = _two_launches(x, wq, bq, wk, items, Lt, dtype).view_as(got)
    same = torch.equal(_bits(got), _bits(two))
    print(f"fused query {kind} items {items} L {Lt} {dt}: |d| / bound {r:.3f}, bit-identical to the two launches: {same}  [{time.time() - t0:.1f} s]")
    assert r <= 1.0
    assert same, f"{int((_bits(got) != _bits(two)).sum())} elements differ from the two-launch path"


def _context(u, wv, bv, M, dtype, tile, k128, family):
    """Step 6e through mra_debug_gemm with the forward's descriptor: batch = heads, U behind an item view, ctx [M][H]."""
    ctx = Buf(M * X.HEADS * 64, dtype)
    nb = lambda b: b.numel * b.inner.element_size()
    R, K = X.HEADS * X.Q, X.CTX_K
    d = _desc(A=u.inner.data_ptr(), a_bytes=nb(u), W=wv.inner.data_ptr(), w_bytes=nb(wv), bias=bv.inner.data_ptr(), bias_bytes=nb(bv),
              C=ctx.inner.data_ptr(), c_bytes=nb(ctx), a_view=(R * K, X.Q, K), c_view=(0, M, X.HEADS * 64), M=M, N=64, K=K, batch=X.HEADS,
              a_bs=X.Q * K, w_bs=64 * K, c_bs_bytes=128, bias_bs=64, tile_cfg=tile, k128=k128)
    before = L.gemm_launches(family, EPI_OP)
    _ok(L.lib().mra_debug_gemm(d, 1, EPI_OP, L.mra_dtype(dtype), _stream()), "fold context gemm")
    assert L.gemm_launches(family, EPI_OP) - before == 1
    return ctx.result(True, "ctx").view(M, X.HEADS * 64)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("M", X.CTX_M)
def test_context_gemm_on_the_64x64_k128_tile(M, dt, dev):
    dtype = X.DTYPES[dt]
    u_, wv_, bv_ = X.ctx_inputs(M, dt)
    u, wv, bv = (Buf(t.numel(), t.dtype, t) for t in (u_, wv_, bv_))
    got = _context(u, wv, bv, M, dtype, GT_64, 1, GF_K128_64x64)
    present = _context(u, wv, bv, M, dtype, GT_K128_64x128, 0, GF_K128_64x128)
    for name, b in (("u", u), ("w_v", wv), ("b_v", bv)):
        b.unchanged(name)
    ref, bound = X.ctx_reference(M, dt)
    r = float(((got.double() - ref).abs() / bound).max())
    same = torch.equal(_bits(got), _bits(present))
    print(f"context M {M} {dt}: |d| / bound {r:.3f}, bit-identical to the 64 x 128 tile: {same}")
    assert r <= 1.0 and same


GF_WS_176x384, EPI_SOFTPART, GT_WS_176x384 = 6, 5, 5


def _penc(pt, enc, kv, dtype, **extra):
    """Step 6d through mra_debug_gemm with the forward's descriptor: batch = items, the encoder tokens as the K-major operand."""
    B, R, E, kvp = X.ST_B, X.ST_R, X.E, X.fold_kvp(kv)
    u = Buf(B * R * E, dtype)
    nb = lambda b: b.numel * b.inner.element_size()
    d = _desc(A=pt.inner.data_ptr(), a_bytes=nb(pt), W=enc.inner.data_ptr(), w_bytes=nb(enc), C=u.inner.data_ptr(), c_bytes=nb(u),
              a_view=(0, R, kvp), c_view=(0, R, E), M=R, N=E, K=kvp, batch=B, a_bs=R * kvp, w_bs=kv * E, c_bs_bytes=R * E * 2, w_ld=E, k_rows=kv,
              tile_cfg=GT_WS_176x384, ps_ntiles=X.st_ntiles(kv))
    for k, b in extra.items():
        if isinstance(b, Buf):
            setattr(d, k, b.inner.data_ptr())
            setattr(d, k + "_bytes", nb(b))
        else:
            setattr(d, k, b)
    _ok(L.lib().mra_debug_gemm(d, 1, EPI_OP, L.mra_dtype(dtype), _stream()), "fold p.enc gemm")
    return u.result(True, "U").view(B, R, E)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("kind", X.ST_KINDS)
@pytest.mark.parametrize("kv", X.ST_KV)
def test_statistics_fed_penc_launch(kv, kind, dt, dev):
    dtype = X.DTYPES[dt]
    B, R, E, kvp, nt = X.ST_B, X.ST_R, X.E, X.fold_kvp(kv), X.st_ntiles(kv)
    qp_, enc_ = X.st_inputs(kv, kind, dt)
    qp, enc = Buf(qp_.numel(), dtype, qp_), Buf(enc_.numel(), dtype, enc_)
    pt, sm, sl = Buf(B * R * kvp, dtype), Buf(B * R * nt, torch.float32), Buf(B * R * nt, torch.float32)
    nb = lambda b: b.numel * b.inner.element_size()
    d = _desc(A=qp.inner.data_ptr(), a_bytes=nb(qp), W=enc.inner.data_ptr(), w_bytes=nb(enc), C=pt.inner.data_ptr(), c_bytes=nb(pt),
              stat_m=sm.inner.data_ptr(), stat_m_bytes=nb(sm), stat_l=sl.inner.data_ptr(), stat_l_bytes=nb(sl), a_view=(0, R, E), c_view=(0, R, kvp),
              M=R, N=kv, K=E, batch=B, a_bs=R * E, w_bs=kv * E, c_bs_bytes=R * kvp * 2, n_ragged=1, alpha=X.ALPHA, tile_cfg=GT_WS_176x384)
    _ok(L.lib().mra_debug_gemm(d, 1, EPI_SOFTPART, L.mra_dtype(dtype), _stream()), "fold scores gemm")
    # the statistics-fed launch first, on P~ as the scores launch left it: every column from ntiles * 176 on is still the sentinel (NaN)
    pt_cpu = pt.inner.cpu().view(B, R, kvp)
    assert nt * 176 == kvp or torch.isnan(pt_cpu[:, :, nt * 176:].float()).all()
    n0 = L.lib().mra_debug_fold_rowfactor_launches()
    got = _penc(pt, enc, kv, dtype, stat_m=sm, stat_l=sl, ps_stats=1)
    assert L.lib().mra_debug_fold_rowfactor_launches() == n0
    sm_cpu, sl_cpu = sm.inner.cpu().view(B, R, nt), sl.inner.cpu().view(B, R, nt)
    ref, bound = X.penc_reference(pt_cpu, sm_cpu, sl_cpu, enc_, dtype)
    r = float(((got.double() - ref).abs() / bound).max())
    # the present pair of launches on the same P~ and statistics
    gfac = Buf(B * nt * 512, torch.float32)
    _ok(L.lib().mra_debug_fold_rowfactor(sm.ptr, sl.ptr, gfac.ptr, B * R, R, nt, pt.ptr, kvp, 176, kvp, None, _stream()), "fold_rowfactor")
    assert (pt.inner.view(B, R, kvp)[:, :, nt * 176:] == 0).all()
    present = _penc(pt, enc, kv, dtype, pscale=gfac)
    same = torch.equal(_bits(got), _bits(present))
    print(f"statistics-fed P.enc kv {kv} {kind} {dt}: |d| / bound {r:.3f}, bit-identical to rowfactor + pscale: {same}")
    assert r <= 1.0
    assert same, f"{int((_bits(got) != _bits(present)).sum())} elements differ"


# =========================================================================================================================================
# forward level
# =========================================================================================================================================
@pytest.fixture(scope="module")
def small(dev):
    qf, cfg = build_qformer(dev, X.E, seed=11, layers=4)
    assert (cfg.heads, cfg.n_query, cfg.hidden, cfg.cross_freq) == (12, 32, 768, 2)
    qf.set_cross_mode("fold")
    return qf, cfg


def _counts():
    return (L.lib().mra_debug_fold_query_launches(), L.gemm_launches(GF_V1_64, EPI_OP), L.gemm_launches(GF_V1_128, EPI_OP))


def _forward(qf, dev, ids, att, x, mask):
    qf.set_option("cross_fuse", mask)
    c0 = _counts()
    try:
        raw, out = _run(qf, dev, ids, att, x)
        torch.cuda.synchronize()
    finally:
        qf.set_option("cross_fuse", 1)
    return raw, {k: v.cpu() for k, v in out.items() if v is not None}, [b - a for a, b in zip(c0, _counts())]


@pytest.mark.parametrize("raw_features", [1, 0])
@pytest.mark.parametrize("kv", [176, 300])
def test_forward_with_the_fused_launch_equals_mask_zero(kv, raw_features, small, dev):
    qf, cfg = small
    ids, att, x16 = _features(oracle_cfg(cfg), kv, 60 + kv)
    x = x16.to(dev)
    qf.set_option("raw_features", raw_features)
    try:
        raw1, on, n_on = _forward(qf, dev, ids, att, x, 1)
        raw0, off, n_off = _forward(qf, dev, ids, att, x, 0)
    finally:
        qf.set_option("raw_features", 1)
    assert raw1 == raw0 == bool(raw_features)
    for k in off:
        assert torch.equal(_bits(on[k]), _bits(off[k])), f"{k}: the fused launch changed the forward's output"
    # two cross layers: two fused launches in place of two cross query GEMMs and two Q' GEMMs (E = 704: both on the 64 x 64 tile)
    print(f"kv {kv} raw {raw_features}: launches (fused, 64x64 OP, 128x128 OP) on {n_on} off {n_off}")
    assert n_on[0] == 2 and n_off[0] == 0
    assert n_off[1] - n_on[1] == 4 and n_off[2] == n_on[2]


def test_probing_and_split_forwards_do_not_take_the_fused_launch(small, dev):
    qf, cfg = small
    ids, att, x16 = _features(oracle_cfg(cfg), 300, 77)
    x = x16.to(dev)
    results = {}
    try:
        for mode in ("auto", "split"):
            for mask in (7, 0):
                qf.set_cross_precision("op")
                qf.set_cross_precision(mode)    # "auto": unresolved again, the next forward probes
                _, out, n = _forward(qf, dev, ids, att, x, mask)
                assert n[0] == 0, f"{mode} forward took the fused launch"
                results[(mode, mask)] = out
    finally:
        qf.set_cross_precision("op")
    for mode in ("auto", "split"):
        for k, v in results[(mode, 0)].items():
            assert torch.equal(_bits(results[(mode, 7)][k]), _bits(v)), f"{mode} {k}: the option changed a forward that must not take it"


def test_context_tile_in_a_forward_at_width_1408(dev):
    """Bit 4 needs E % 128 == 0 and >= 512 query rows (where the forward takes the 64 x 128 tile today): 16 items at E = 1408, kv 176."""
    from tools.make_golden import make_inputs
    qf, cfg = build_qformer(dev, 1408, seed=12, layers=4)
    qf.set_cross_mode("fold")
    ids, tmask, att, feats = make_inputs(oracle_cfg(cfg), 16, 5, 176, 91, True)
    x = feats.half().to(dev)
    fams = (GF_K128_64x128, GF_K128_64x64)
    outs, ran = {}, {}
    for mask in (5, 0, 4):
        qf.set_option("cross_fuse", mask)
        c0 = [L.gemm_launches(f, EPI_OP) for f in fams]
        raw, out = _run(qf, dev, ids, att, x)
        torch.cuda.synchronize()
        outs[mask] = {k: v.cpu() for k, v in out.items() if v is not None}
        ran[mask] = [L.gemm_launches(f, EPI_OP) - a for f, a in zip(fams, c0)]
        assert raw
    print("context launches (64x128, 64x64 k128) per mask", ran)
    assert ran[0] == [2, 0] and ran[4] == [0, 2] and ran[5] == [0, 2]
    for mask in (5, 4):
        for k, v in outs[0].items():
            assert torch.equal(_bits(outs[mask][k]), _bits(v)), f"mask {mask} {k}: the option changed the forward's output"


@pytest.mark.parametrize("raw_features", [1, 0])
@pytest.mark.parametrize("kv", [176, 300])
def test_forward_with_in_launch_row_factors_equals_mask_zero(kv, raw_features, small, dev):
    qf, cfg = small
    ids, att, x16 = _features(oracle_cfg(cfg), kv, 80 + kv)
    x = x16.to(dev)
    qf.set_option("raw_features", raw_features)
    outs, ran = {}, {}
    try:
        for mask in (7, 2, 0):
            n0 = L.lib().mra_debug_fold_rowfactor_launches()
            _, outs[mask], _ = _forward(qf, dev, ids, att, x, mask)
            ran[mask] = L.lib().mra_debug_fold_rowfactor_launches() - n0
    finally:
        qf.set_option("raw_features", 1)
    assert ran == {7: 0, 2: 0, 0: 2}, ran
    for mask in (7, 2):
        for k, v in outs[0].items():
            assert torch.equal(_bits(outs[mask][k]), _bits(v)), f"mask {mask} {k}: the option changed the forward's output"


def test_option_accepts_its_bits_and_refuses_every_other_value(small):
    from mraudio_amd.qformer import MraError
    qf, _ = small
    try:
        for mask in range(8):
            qf.set_option("cross_fuse", mask)
        for bad in (8, 9, 16, 255, -1):
            with pytest.raises(MraError):
                qf.set_option("cross_fuse", bad)
    finally:
        qf.set_option("cross_fuse", 1)
