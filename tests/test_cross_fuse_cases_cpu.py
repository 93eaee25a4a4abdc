"""CPU side of ``mra_qformer_set_option "cross_fuse"`` (tests/cross_fuse_cases.py).  Bit 1, the fused query launch: the fp32 emulation sits
inside the derived bounds, every named mutant outside the bound of the input kind that must reject it, and ``mra_debug_fold_query`` refuses
every null, misaligned or short buffer with nothing launched (there is no GPU here: a launch would fail with another code).  Bit 2, the
row factors inside the P . enc launch: the emulation of the statistics-fed launch inside the bound, the wrong tile's maximum and a stale
ring slot outside it, and every refusal of the ``mra_gemm_desc.ps_stats`` form through ``mra_debug_gemm_plan``, which launches nothing.
Bit 4, the context GEMM on the 64 x 64 tile: the refusals of ``mra_gemm_desc.k128`` the same way."""
import ctypes as C

import pytest

import cross_fuse_cases as X
from mraudio_amd import _lib as L

SMALL = (3, 9)   # items, L: a ragged 96-row tile behind a strided view


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("kind", X.KINDS)
def test_emulation_inside_bound(kind, dt):
    items, Lt = SMALL
    r = X.worst_ratio(X.emulate(kind, items, Lt, dt), kind, items, Lt, dt)
    print(f"{kind} {dt}: |d| / bound {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("mutant", X.MUTANTS)
def test_mutants_outside_bound(mutant, dt):
    items, Lt = SMALL
    kind = X.REJECTED_BY[mutant]
    r = X.worst_ratio(X.emulate(kind, items, Lt, dt, mutant=mutant), kind, items, Lt, dt)
    print(f"{mutant} on {kind} {dt}: |d| / bound {r:.3f}")
    assert r > 1.0


def test_grid_inputs_make_phase_one_exact():
    """The premise of the "grid" kind: the fp32 accumulator of phase 1 equals the float64 sum, in ascending and in descending K order."""
    import torch
    wq, bq, _ = X.weights("grid", "bf16")
    x = X.inputs("grid", 3, 0, "bf16")[:, :X.Q].reshape(-1, X.H)
    exact = x.double() @ wq.double().T
    for order in (range(0, X.H, 64), range(X.H - 64, -1, -64)):
        acc = torch.zeros(x.shape[0], X.H)
        for k0 in order:
            acc = acc + x.float()[:, k0:k0 + 64] @ wq.float()[:, k0:k0 + 64].T
        assert torch.equal(acc.double(), exact)
    assert torch.equal((acc + bq).double(), exact + bq.double())


def _call(items=3, Lt=9, rows=None, view=None, sizes=None, ptrs=None, H=X.H, E=X.E, Q=X.Q, heads=X.HEADS, dtype=L.MRA_F16):
    nbytes = list(X.buffer_bytes(items, Lt) if sizes is None else sizes)
    p = [1 << 20, 2 << 20, 3 << 20, 4 << 20, 8 << 20] if ptrs is None else ptrs   # never dereferenced: every call here is refused
    v = (C.c_int64 * 3)(*(X.x_view(Lt) if view is None else view))
    return L.lib().mra_debug_fold_query(p[0], v, nbytes[0], p[1], nbytes[1], p[2], nbytes[2], p[3], nbytes[3], p[4], nbytes[4],
                                        items * X.Q if rows is None else rows, H, E, Q, heads, dtype, None)


def test_debug_entry_refusals():
    lib = L.lib()
    launched = lib.mra_debug_fold_query_launches()
    ok = list(X.buffer_bytes(3, 9))
    bad = []
    bad.append(_call(rows=-32))
    bad.append(_call(dtype=L.MRA_F32))
    bad.append(_call(H=760))
    bad.append(_call(E=700))
    bad.append(_call(rows=100))                                   # not a multiple of Q
    bad.append(_call(heads=0))
    bad.append(_call(view=(41 * X.H, 32, X.H - 8)))                # row stride below H
    bad.append(_call(view=(41 * X.H + 4, 32, X.H)))                # item stride not a multiple of 8
    bad.append(_call(view=(41 * X.H, 0, X.H)))
    for i in (0, 1, 3, 4):                                         # null x, w_q, w_k, q_prime
        p = [1 << 20, 2 << 20, 3 << 20, 4 << 20, 8 << 20]
        p[i] = None
        bad.append(_call(ptrs=p))
    for i in range(5):                                             # misaligned
        p = [1 << 20, 2 << 20, 3 << 20, 4 << 20, 8 << 20]
        p[i] += 8
        bad.append(_call(ptrs=p))
    view_bytes = ((3 - 1) * (X.Q + 9) * X.H + X.Q * X.H) * 2       # x is needed up to the last query row of the last item
    for i in range(5):                                             # short by one element
        s = list(ok)
        s[i] = (view_bytes if i == 0 else s[i]) - 2
        bad.append(_call(sizes=s))
    bad.append(_call(items=5, sizes=ok))                           # sizes of 3 items, rows of 5
    assert all(rc == -1 for rc in bad), bad
    assert lib.mra_last_error()
    assert _call(rows=0) == 0                                      # rows == 0 is a no-op after the shape checks
    assert lib.mra_debug_fold_query_launches() == launched        # nothing was launched by any call above


def test_option_values():
    """mra_qformer_set_option "cross_fuse" without a handle is refused like every other option (no GPU needed)."""
    assert L.lib().mra_qformer_set_option(None, b"cross_fuse", 1) == -1


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("kind", X.ST_KINDS)
@pytest.mark.parametrize("kv", X.ST_KV)
def test_statistics_fed_penc_emulation_inside_bound_and_mutants_outside(kv, kind, dt):
    dtype = X.DTYPES[dt]
    qp, enc = X.st_inputs(kv, kind, dt)
    pt, sm, sl = X.emulate_scores(qp, enc, kv, dtype)
    ref, bound = X.penc_reference(pt, sm, sl, enc, dtype)
    ratio = lambda out: float(((out.double() - ref).abs() / bound).max())
    r = ratio(X.emulate_penc(pt, sm, sl, enc, dtype))
    rm = {m: ratio(X.emulate_penc(pt, sm, sl, enc, dtype, mutant=m)) for m in X.ST_MUTANTS}
    print(f"kv {kv} {kind} {dt}: |d| / bound {r:.3f}, mutants {rm}")
    assert r <= 1.0
    if X.st_ntiles(kv) > 1:
        assert rm["factor_from_wrong_tile"] > 1.0
    if X.st_ntiles(kv) > 4:
        assert rm["stale_ring_slot"] > 1.0


# =========================================================================================================================================
# the new fields of mra_gemm_desc (ps_stats, k128): every refusal through mra_debug_gemm_plan -- host only, no pointer followed, no launch
# =========================================================================================================================================
EPI_OP, EPI_GELU_OP, GT_AUTO, GT_64, GT_128, GT_WS_176x384, GT_K128_64x128, GF_WS_176x384, GF_K128_64x64 = 0, 1, 0, 1, 2, 5, 6, 6, 10
CUS = 256


def _plan(d, epi=EPI_OP):
    out = (C.c_int32 * 7)()
    arr = (L.mra_gemm_desc * 1)(d)
    return L.lib().mra_debug_gemm_plan(arr, 1, epi, L.MRA_F16, CUS, out), list(out)


def _penc_desc(kv=300, **kw):
    """Step 6d as the forward describes it with "cross_fuse" bit 2 (tests/test_gpu_cross_fuse.py _penc): addresses never dereferenced."""
    B, R, E, kvp, nt = X.ST_B, X.ST_R, X.E, X.fold_kvp(kv), X.st_ntiles(kv)
    f = dict(A=1 << 20, a_bytes=B * R * kvp * 2, W=1 << 24, w_bytes=B * kv * E * 2, C=1 << 26, c_bytes=B * R * E * 2,
             stat_m=1 << 28, stat_m_bytes=B * R * nt * 4, stat_l=1 << 29, stat_l_bytes=B * R * nt * 4,
             a_view=(0, R, kvp), c_view=(0, R, E), M=R, N=E, K=kvp, batch=B, a_bs=R * kvp, w_bs=kv * E, c_bs_bytes=R * E * 2, w_ld=E, k_rows=kv,
             tile_cfg=GT_WS_176x384, ps_ntiles=nt, ps_stats=1)
    f.update(kw)
    d = L.mra_gemm_desc()
    d.struct_bytes = C.sizeof(L.mra_gemm_desc)
    for k, v in f.items():
        if k.endswith("_view"):
            getattr(d, k)[:] = v
        else:
            setattr(d, k, v)
    return d


@pytest.mark.parametrize("kv", X.ST_KV)
def test_statistics_fed_descriptor_passes_the_host_checks(kv):
    rc, out = _plan(_penc_desc(kv))
    assert rc == 0, L.lib().mra_last_error()
    assert out[1] == GF_WS_176x384


def test_statistics_fed_descriptor_refusals():
    """Each line breaks ONE thing of a descriptor that passes (the test above): ps_stats beside pscale, without K-major weights, under
    another epilogue, null or misaligned statistics, more than one row tile, no tile count, statistics one float short, another tile."""
    lib = L.lib()
    before = (L.gemm_launches(GF_WS_176x384, EPI_OP), lib.mra_debug_fold_rowfactor_launches())
    kv = 300
    B, R, nt = X.ST_B, X.ST_R, X.st_ntiles(kv)
    full = B * R * nt * 4
    bad = {
        "ps_stats 2": _plan(_penc_desc(kv, ps_stats=2)),
        "ps_stats -1": _plan(_penc_desc(kv, ps_stats=-1)),
        "with pscale": _plan(_penc_desc(kv, pscale=1 << 30, pscale_bytes=B * nt * 512 * 4)),
        "no w_ld": _plan(_penc_desc(kv, w_ld=0, k_rows=0, N=176, w_bytes=B * 176 * X.fold_kvp(kv) * 2, w_bs=176 * X.fold_kvp(kv))),
        "EPI_GELU_OP": _plan(_penc_desc(kv), epi=EPI_GELU_OP),
        "null stat_m": _plan(_penc_desc(kv, stat_m=None)),
        "null stat_l": _plan(_penc_desc(kv, stat_l=None)),
        "stat_m off by 2 bytes": _plan(_penc_desc(kv, stat_m=(1 << 28) + 2)),
        "stat_l off by 2 bytes": _plan(_penc_desc(kv, stat_l=(1 << 29) + 2)),
        "M 385": _plan(_penc_desc(kv, M=R + 1, a_view=(0, R + 1, X.fold_kvp(kv)), c_view=(0, R + 1, X.E), a_bytes=1 << 30, c_bytes=1 << 30,
                                  a_bs=(R + 1) * X.fold_kvp(kv), c_bs_bytes=(R + 1) * X.E * 2, stat_m_bytes=1 << 30, stat_l_bytes=1 << 30)),
        "ps_ntiles 0": _plan(_penc_desc(kv, ps_ntiles=0)),
        "ps_ntiles -1": _plan(_penc_desc(kv, ps_ntiles=-1)),
        "stat_m one float short": _plan(_penc_desc(kv, stat_m_bytes=full - 4)),
        "stat_l one float short": _plan(_penc_desc(kv, stat_l_bytes=full - 4)),
        "statistics of one item, batch of two": _plan(_penc_desc(kv, stat_m_bytes=full // 2, stat_l_bytes=full // 2)),
        "K far past the tiles counted": _plan(_penc_desc(kv, ps_ntiles=1, K=X.fold_kvp(1000), a_view=(0, R, X.fold_kvp(1000)),
                                                         a_bs=R * X.fold_kvp(1000), a_bytes=B * R * X.fold_kvp(1000) * 2)),
        "another tile": _plan(_penc_desc(kv, tile_cfg=GT_128)),
    }
    assert all(rc == -1 for rc, _ in bad.values()), {k: rc for k, (rc, _) in bad.items()}
    assert lib.mra_last_error()
    assert (L.gemm_launches(GF_WS_176x384, EPI_OP), lib.mra_debug_fold_rowfactor_launches()) == before


def _ctx_desc(M=96, **kw):
    """Step 6e as the forward describes it with "cross_fuse" bit 4 (tests/test_gpu_cross_fuse.py _context)."""
    R, K = X.HEADS * X.Q, X.CTX_K
    items = M // X.Q
    f = dict(A=1 << 20, a_bytes=items * R * K * 2, W=1 << 24, w_bytes=X.HEADS * 64 * K * 2, bias=1 << 25, bias_bytes=X.HEADS * 64 * 4,
             C=1 << 26, c_bytes=M * X.HEADS * 64 * 2, a_view=(R * K, X.Q, K), c_view=(0, M, X.HEADS * 64), M=M, N=64, K=K, batch=X.HEADS,
             a_bs=X.Q * K, w_bs=64 * K, c_bs_bytes=128, bias_bs=64, tile_cfg=GT_64, k128=1, ps_ntiles=0, ps_stats=0,
             stat_m=None, stat_l=None, stat_m_bytes=0, stat_l_bytes=0, w_ld=0, k_rows=0)
    f.update(kw)
    return _penc_desc(**f)


def test_k128_descriptor_and_its_refusals():
    rc, out = _plan(_ctx_desc())
    assert rc == 0, L.lib().mra_last_error()
    assert out[1] == GF_K128_64x64
    before = L.gemm_launches(GF_K128_64x64, EPI_OP)
    K = X.CTX_K + 64   # a multiple of 64 and not of 128
    bad = {
        "k128 2": _plan(_ctx_desc(k128=2)),
        "k128 -1": _plan(_ctx_desc(k128=-1)),
        "GT_AUTO": _plan(_ctx_desc(tile_cfg=GT_AUTO)),
        "GT_128": _plan(_ctx_desc(tile_cfg=GT_128)),
        "GT_K128_64x128": _plan(_ctx_desc(tile_cfg=GT_K128_64x128)),
        "K % 128": _plan(_ctx_desc(K=K, a_view=(X.HEADS * X.Q * K, X.Q, K), a_bs=X.Q * K, w_bs=64 * K, a_bytes=1 << 30, w_bytes=1 << 30)),
    }
    assert all(rc == -1 for rc, _ in bad.values()), {k: rc for k, (rc, _) in bad.items()}
    assert L.gemm_launches(GF_K128_64x64, EPI_OP) == before
