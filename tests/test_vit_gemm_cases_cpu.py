"""Without a GPU: the case table of tests/vit_gemm_cases.py is what tests/test_gpu_gemm_vit.py will launch, so here it is held to account first
-- every case resolves (mra_debug_gemm_plan, host only) to the kernel family it names, the table covers exactly the (family, epilogue) pairs
PAIRS lists for csrc/vit.hip, the fp32 emulation of every form sits inside its derived bound (the ratios are printed), every named mutant falls
outside, and every refusal the ViT's forms add to mra_debug_gemm, and every one of the mra_debug_vit_* entries, refuses before any launch."""
import ctypes as C

import pytest
import torch

import vit_gemm_cases as V
from mraudio_amd import _lib as L

DTS = ("f16", "bf16")
ROWS = sorted({c["row"] for c in V.CASES})


def test_the_codes_repeat_the_bindings():
    for n in ("EPI_OP", "EPI_GELU_OP", "EPI_RES_F32", "EPI_RES_OP", "EPI_RES_F32_STAT", "EPI_LNF_OP", "EPI_LNF_GELU_OP", "EPI_RES_OP_STAT", "GT_AUTO",
              "GT_128", "GT_256", "GT_P8_TAIL", "GT_P8_MIXED", "GF_V1_64", "GF_V1_128", "GF_P8_256", "GF_P8_MIXED"):
        assert getattr(V, n) == getattr(L, n), n
    assert C.sizeof(L.mra_gemm_desc) % 8 == 0 and L.mra_gemm_desc.aux.offset == L.mra_gemm_desc.col_scale_bytes.offset + 8


def test_the_table_covers_exactly_the_pairs_the_vit_reaches():
    have = {(c["family"], c["epi"]) for c in V.CASES}
    assert have == set(V.PAIRS), (sorted(set(V.PAIRS) - have), sorted(have - set(V.PAIRS)))
    assert ROWS == list(range(1, 10))
    assert all(V.ROW_MUTANTS[r] for r in ROWS)


def _plan(c, dt, cus=V.CUS, persist=None):
    out = (C.c_int32 * 7)()
    arr = V.descriptor(c, dt, V.fake_addr(c, dt), persist)
    rc = L.lib().mra_debug_gemm_plan(arr, 1, c["epi"], L.mra_dtype(V.DTYPES[dt]), cus, out)
    return rc, list(out)


@pytest.mark.parametrize("name", [c["name"] for c in V.CASES] + ["chain proj RES_F32_STAT M300 N384 K256", "chain qkv LNF_OP M300 N256 K384"])
def test_every_case_resolves_to_the_family_it_names(name):
    c = V.BY_NAME[name]
    M, N = c["M"], c["N"]
    for dt in DTS:
        rc, (tile, family, threads, lds, grid, persistent, tiles) = _plan(c, dt)
        assert rc == 0, (name, L.lib().mra_last_error())
        assert family == c["family"] and c["tile"] in (V.GT_AUTO, tile), (name, family, tile)
        if family == V.GF_P8_MIXED:      # per pair of row tiles 2 k full tiles and one tail tile
            assert tiles == ((M + 255) // 256 + 1) // 2 * (2 * (N // 256) + 1)
        else:
            tn = {V.GF_V1_64: 64, V.GF_V1_128: 128, V.GF_P8_256: 256}[family]
            assert tiles == ((M + tn - 1) // tn) * (N // tn)
        assert persistent == c["persist"]
        assert grid == ((V.CUS & ~7) if c["persist"] else tiles)
        if c["persist"]:
            assert tiles == 289 and V.CUS < tiles < 2 * V.CUS
            rc, plan0 = _plan(c, dt, persist=0)
            assert rc == 0 and plan0[5] == 0 and plan0[4] == tiles


def test_the_edges_the_cases_name():
    """Case 1: six workgroups (the remap's remainder branch), an odd number of row tiles; case 3: 11 K steps, 8 live rows in the last row tile."""
    rc, plan = _plan(V.BY_NAME["mixed RES_F32 M600 N384 K128"], "f16")
    assert plan[6] == 6 and plan[6] % 8 and (600 + 255) // 256 == 3
    c = V.BY_NAME["mixed RES_F32_STAT M776 N1408 K1408"]
    assert c["K"] // 128 == 11 and c["M"] - 3 * 256 == 8 and c["y16"]["view"][2] > c["N"]
    assert V.persist_shape(256) == 16 * 256 + 40 and V.persist_shape(304) == 18 * 256 + 40
    assert len(V.persistent_tiles(16 * 256 + 40, 17 * 256, 256)) == 33


@pytest.mark.parametrize("row", ROWS)
def test_faithful_emulations_are_inside_their_bounds(row):
    worst, failures = {}, []
    for c in V.cases_of(row):
        for dt in DTS:
            ratios, fails = V.check(c["name"], dt, V.emulate(c["name"], dt))
            for k, v in ratios.items():
                worst[(dt, k)] = max(worst.get((dt, k), (0.0, "")), (v, c["name"]))
            failures += [(c["name"], dt, f) for f in fails]
    print(f"row {row}: worst emulated |d| / bound " + ", ".join(f"{dt} {k} {v:.3f} ({n})" for (dt, k), (v, n) in sorted(worst.items())))
    assert not failures, failures[:10]
    assert all(0.0 <= v <= 1.0 for v, _ in worst.values())


@pytest.mark.parametrize("row,mutant", [(r, m) for r in ROWS for m in V.ROW_MUTANTS[r]])
def test_every_mutant_is_outside_its_bound(row, mutant):
    for dt in DTS:
        caught = None
        for c in V.cases_of(row):
            ratios, fails = V.check(c["name"], dt, V.emulate(c["name"], dt, mutant))
            if fails:
                caught = (c["name"], fails[0])
                break
        assert caught, f"{mutant} ({dt}) passes every case of row {row}"
        print(f"{mutant} {dt}: caught by {caught[0]}: {caught[1]}")


@pytest.mark.parametrize("dt", DTS)
def test_the_chain_emulation_and_its_mutants(dt):
    r = V.chain_check(dt, *V.chain_emulate(dt))
    print(f"chain {dt}: emulated |d| / bound {r:.3f}")
    assert r <= 1.0
    for m in V.CHAIN_MUTANTS:
        rm = V.chain_check(dt, *V.chain_emulate(dt, m))
        print(f"  {m}: {rm:.3g}")
        assert not rm <= 1.0, m


@pytest.mark.parametrize("dt", DTS)
def test_the_companion_emulations_and_their_mutants(dt):
    dtype = V.DTYPES[dt]
    for N, K, wb in V.FOLD_CASES:
        f = V.fold_case(N, K, wb, dt)
        r = V.fold_weight_check(f, *V.fold_weight_emulate(f, dtype), dtype)
        print(f"fold_weight N{N} K{K} bias {wb} {dt}: {r}")
        assert all(v <= 1.0 for v in r.values()), r
        for m in V.FOLD_MUTANTS:
            rm = V.fold_weight_check(f, *V.fold_weight_emulate(f, dtype, m), dtype)
            assert not all(v <= 1.0 for v in rm.values()), (m, rm)
    for M, Gn, n in V.GROUP_CASES:
        x, groups = V.group_case(M, Gn, n)
        st = V.group_stats_emulate(groups, n, V.VIT_EPS)
        ra, _ = V.group_stats_check(groups, n, V.VIT_EPS, st)
        rb, _ = V.group_stats_check(groups, n, V.VIT_EPS, st, row=x)
        print(f"group_stats M{M} G{Gn} n{n}: merge {ra}, rows {rb}")
        assert all(v <= 1.0 for v in list(ra.values()) + list(rb.values()))
        for m in V.GROUP_MUTANTS:
            rm, _ = V.group_stats_check(groups, n, V.VIT_EPS, V.group_stats_emulate(groups, n, V.VIT_EPS, m))
            assert not all(v <= 1.0 for v in rm.values()), (m, rm)
    for M, D in V.ROWSTAT_CASES:
        for f32 in (True, False):
            x = V.rowstat_case(M, D, dt, f32)
            st, x16 = V.row_stats_emulate(x, V.VIT_EPS, dtype)
            r = V.row_stats_check(x, V.VIT_EPS, st, x16 if f32 else None, dtype)
            print(f"row_stats M{M} D{D} {'f32' if f32 else dt} rows: {r}")
            assert all(v <= 1.0 for v in r.values()), r
            for m in V.ROWSTAT_MUTANTS[:1 if not f32 else 2]:
                st, x16 = V.row_stats_emulate(x, V.VIT_EPS, dtype, m)
                rm = V.row_stats_check(x, V.VIT_EPS, st, x16 if f32 else None, dtype)
                assert not all(v <= 1.0 for v in rm.values()), (m, D, rm)


# =========================================================================================================================================
# refusals: nothing may reach a launch
# =========================================================================================================================================
def _launched():
    return sum(L.gemm_launches(f, e) for f in range(L.GEMM_FAMILIES) for e in range(16))


def _refused(arr, epi, word, n=1, dt="f16"):
    """Refused by the plan entry and by the launch entry alike, before any launch, with ``word`` in the message."""
    out = (C.c_int32 * 7)()
    assert L.lib().mra_debug_gemm_plan(arr, n, epi, L.mra_dtype(V.DTYPES[dt]), V.CUS, out) == -1
    msg = L.lib().mra_last_error().decode()
    assert word in msg, msg
    before = _launched()
    assert L.lib().mra_debug_gemm(arr, n, epi, L.mra_dtype(V.DTYPES[dt]), None) == -1 and _launched() == before
    assert word in L.lib().mra_last_error().decode()


def _desc(name, dt="f16"):
    c = V.BY_NAME[name]
    return c, V.descriptor(c, dt, V.fake_addr(c, dt))


STAT32, RESOP, RESOP2, STAT16, LNF, GELU, F32M = ("mixed RES_F32_STAT M776 N1408 K1408", "mixed RES_OP M600 N640 K256 in place",
                                                   "mixed RES_OP M600 N640 K256 separate", "mixed RES_OP_STAT M520 N1408 K128 in place",
                                                   "p8_256 LNF_OP M300 N512 K1408 rows", "p8_256 LNF_GELU_OP M257 N256 K128", "mixed RES_F32 M600 N384 K128")


def _exactly(name, field, need):
    """The footprint itself passes; one element less is refused by both entries."""
    c, arr = _desc(name)
    setattr(arr[0], field, need)
    out = (C.c_int32 * 7)()
    assert L.lib().mra_debug_gemm_plan(arr, 1, c["epi"], L.MRA_F16, V.CUS, out) == 0, (name, field, L.lib().mra_last_error())
    setattr(arr[0], field, need - 2)
    _refused(arr, c["epi"], field.replace("_bytes", ""))


def _need(l, rows, cols, esz):
    return (int(V.index(l, rows, cols).max()) + 1 - l["off"]) * esz


def test_footprints_of_the_new_buffers_are_exact():
    c = V.BY_NAME[RESOP2]
    _exactly(RESOP2, "aux_bytes", _need(c["c"], 600, 640, 2))
    _exactly(RESOP, "aux_bytes", _need(c["c"], 600, 640, 2))
    _exactly(RESOP, "c_bytes", _need(c["c"], 600, 640, 2))
    c = V.BY_NAME[STAT32]
    _exactly(STAT32, "ln_y32_bytes", 776 * 11 * 2 * 4)
    _exactly(STAT32, "ln_y16_bytes", _need(c["y16"], 776, 1408, 2))
    _exactly(STAT32, "c_bytes", _need(c["c"], 776, 1408, 4))
    _exactly(STAT32, "r_bytes", 776 * 1408 * 4)
    _exactly(STAT32, "bias_bytes", 1408 * 4)
    _exactly(STAT16, "ln_y32_bytes", 520 * 22 * 2 * 4)
    _exactly(STAT16, "bias_bytes", 1408 * 4)
    _exactly(LNF, "ln_y32_bytes", 300 * 2 * 4)
    _exactly(LNF, "ln_gain_bytes", 512 * 4)
    _exactly(GELU, "ln_y32_bytes", 257 * 2 * 4)
    _exactly(GELU, "ln_gain_bytes", 256 * 4)


@pytest.mark.parametrize("name,change,word", [
    (RESOP, lambda d: setattr(d, "aux", 0), "aux"),
    (RESOP2, lambda d: setattr(d, "aux", d.aux + 8), "aux"),
    (RESOP2, lambda d: setattr(d, "aux", d.C + 16), "overlaps"),
    (RESOP2, lambda d: setattr(d, "aux", d.C - 16), "overlaps"),
    (STAT16, lambda d: setattr(d, "aux", d.C + 1408 * 2 + 16), "overlaps"),
    (STAT16, lambda d: setattr(d, "aux", 0), "aux"),
    (STAT16, lambda d: setattr(d, "ln_y32", 0), "ln_y32"),
    (STAT16, lambda d: setattr(d, "ln_y32", d.ln_y32 + 4), "ln_y32"),
    (STAT16, lambda d: setattr(d, "bias", 0), "bias"),
    (STAT32, lambda d: setattr(d, "bias", 0), "bias"),
    (STAT32, lambda d: setattr(d, "ln_y32", d.ln_y32 + 4), "ln_y32"),
    (STAT32, lambda d: setattr(d, "ln_y16", 0), "ln_y16"),
    (STAT32, lambda d: setattr(d, "ln_y16", d.ln_y16 + 8), "ln_y16"),
    (STAT32, lambda d: d.ln_y16_view.__setitem__(2, 1412), "ln_y16"),
    (STAT32, lambda d: d.ln_y16_view.__setitem__(2, 1400), "ln_y16"),
    (STAT32, lambda d: setattr(d, "R", 0), "residual"),
    (STAT32, lambda d: d.r_view.__setitem__(2, 1404), "R row stride"),
    (LNF, lambda d: setattr(d, "ln_y32", 0), "ln_y32"),
    (LNF, lambda d: setattr(d, "ln_y32", d.ln_y32 + 4), "ln_y32"),
    (LNF, lambda d: setattr(d, "ln_gain", 0), "ln_gain"),
    (LNF, lambda d: setattr(d, "ln_gain", d.ln_gain + 4), "ln_gain"),
    (GELU, lambda d: setattr(d, "ln_gain", 0), "ln_gain"),
    # what epilogue_rules and tile_rules refuse for these forms: MRA_EINVAL, never a launch
    (LNF, lambda d: setattr(d, "batch", 2), "one plain problem"),
    (LNF, lambda d: setattr(d, "n_ragged", 1), "one plain problem"),
    (STAT32, lambda d: setattr(d, "batch", 2), "one plain problem"),
    (RESOP, lambda d: setattr(d, "n_ragged", 1), "one plain problem"),
    (STAT16, lambda d: setattr(d, "batch", 3), "one plain problem"),
    (F32M, lambda d: setattr(d, "batch", 2), "gemm_plan"),
    (F32M, lambda d: setattr(d, "N", 512), "gemm_plan"),          # N % 256 == 128
    (F32M, lambda d: setattr(d, "N", 128), "gemm_plan"),          # N >= 384
    (F32M, lambda d: setattr(d, "K", 64), "gemm_plan"),           # K % 128
    (STAT32, lambda d: setattr(d, "K", 1344), "gemm_plan"),
    (LNF, lambda d: setattr(d, "N", 384), "gemm_plan"),           # N % 256 on the 256 x 256 tile
    (LNF, lambda d: d.c_view.__setitem__(2, 524), "gemm_plan"),   # 16-byte stores
    (F32M, lambda d: setattr(d, "tile_cfg", V.GT_P8_TAIL), "tile_cfg"),
    (LNF, lambda d: setattr(d, "tile_cfg", V.GT_128), "no such epilogue"),
    (STAT32, lambda d: setattr(d, "tile_cfg", V.GT_128), "no such epilogue"),
    (STAT16, lambda d: setattr(d, "tile_cfg", V.GT_AUTO), "no such epilogue"),
])
def test_refusals_of_the_vit_forms(name, change, word):
    c, arr = _desc(name)
    change(arr[0])
    _refused(arr, c["epi"], word)


def test_more_than_one_problem_is_refused():
    for name in (RESOP, STAT32, LNF, GELU, STAT16):
        c = V.BY_NAME[name]
        one = V.descriptor(c, "f16", V.fake_addr(c, "f16"))
        arr = (L.mra_gemm_desc * 2)(one[0], one[0])
        _refused(arr, c["epi"], "one problem", n=2)


def test_aux_equal_to_c_and_a_zero_item_stride_are_accepted():
    for name in (RESOP, STAT16, "patch RES_F32 2x16 N128 K640"):
        c, arr = _desc(name)
        assert (arr[0].aux == arr[0].C) == (c["aux"] == "inplace")
        assert _plan(c, "f16")[0] == 0, L.lib().mra_last_error()
    c, arr = _desc("patch RES_F32 2x16 N128 K640")
    assert arr[0].r_view[0] == 0 and arr[0].r_bytes == 16 * 128 * 4      # the broadcast rows' footprint is ONE set of rows
    arr[0].r_bytes -= 4
    _refused(arr, c["epi"], "r_bytes")


def _vit_refused(rc, word):
    msg = L.lib().mra_last_error().decode()
    assert rc == -1 and word in msg, (rc, msg)


def test_fold_weight_refusals():
    f = L.lib().mra_debug_vit_fold_weight
    P, N, K = 1 << 20, 6, 384
    ok = dict(W=P, w=N * K * 2, gain=2 * P, g=K * 4, beta=3 * P, b=K * 4, bias=4 * P, bb=N * 4, Wf=5 * P, wf=N * K * 2, cs=6 * P, c=N * 4, bf=7 * P, f=N * 4,
              N=N, K=K, dt=L.MRA_F16)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["W"], a["w"], a["gain"], a["g"], a["beta"], a["b"], a["bias"], a["bb"], a["Wf"], a["wf"], a["cs"], a["c"], a["bf"], a["f"], a["N"], a["K"],
                 a["dt"], None)
    assert call(N=0) == 0
    _vit_refused(call(dt=L.MRA_F32), "dtype")
    _vit_refused(call(N=-1), "negative")
    _vit_refused(call(K=0), "positive")
    for k in ("W", "gain", "beta", "Wf", "cs", "bf"):
        _vit_refused(call(**{k: 0}), "null")
    _vit_refused(call(W=P + 1), "aligned")
    _vit_refused(call(cs=6 * P + 2), "aligned")
    _vit_refused(call(bias=4 * P + 2), "aligned")
    _vit_refused(call(w=N * K * 2 - 2), "w_bytes")
    _vit_refused(call(wf=N * K * 2 - 2), "w_bytes")
    _vit_refused(call(g=K * 4 - 4), "gain")
    _vit_refused(call(b=K * 4 - 4), "gain")
    _vit_refused(call(bb=N * 4 - 4), "bias")
    _vit_refused(call(c=N * 4 - 4), "bias")
    _vit_refused(call(f=N * 4 - 4), "bias")
    _vit_refused(call(Wf=P + 64), "overlaps")


def test_group_stats_refusals():
    f = L.lib().mra_debug_vit_group_stats
    P, M, Gn = 1 << 20, 300, 22

    def call(groups=P, gb=M * Gn * 8, M=M, G=Gn, n=64, eps=1e-6, stats=2 * P, sb=M * 8):
        return f(groups, gb, M, G, n, eps, stats, sb, None)
    assert call(M=0) == 0
    _vit_refused(call(M=-1), "M must")
    _vit_refused(call(M=1 << 40), "M must")
    _vit_refused(call(G=0), "G must")
    _vit_refused(call(n=0), "group_cols")
    _vit_refused(call(eps=-1.0), "eps")
    _vit_refused(call(eps=float("nan")), "eps")
    _vit_refused(call(groups=0), "null")
    _vit_refused(call(stats=0), "null")
    _vit_refused(call(groups=P + 4), "float2")
    _vit_refused(call(stats=2 * P + 4), "float2")
    _vit_refused(call(gb=M * Gn * 8 - 4), "groups_bytes")
    _vit_refused(call(sb=M * 8 - 4), "stats_bytes")


def test_row_stats_refusals():
    f = L.lib().mra_debug_vit_row_stats
    P, M, D = 1 << 20, 5, 1408

    def call(x=P, xb=M * D * 4, xdt=L.MRA_F32, M=M, D=D, eps=1e-6, stats=2 * P, sb=M * 8, x16=3 * P, x16b=M * D * 2, dt=L.MRA_F16):
        return f(x, xb, xdt, M, D, eps, stats, sb, x16, x16b, dt, None)
    assert call(M=0) == 0
    _vit_refused(call(dt=L.MRA_F32), "dtype")
    _vit_refused(call(xdt=L.MRA_BF16), "x_dtype")
    _vit_refused(call(M=-1), "M must")
    for bad in (0, 64, 1400, 2176, -128):
        _vit_refused(call(D=bad), "multiple of 128")
    _vit_refused(call(eps=-1.0), "eps")
    _vit_refused(call(x16=0), "x16")
    _vit_refused(call(xdt=L.MRA_F16, xb=M * D * 2), "x16")            # rows in the operand dtype take no copy
    assert call(xdt=L.MRA_F16, xb=M * D * 2, x16=0, x16b=0, M=0) == 0
    _vit_refused(call(x=0), "null")
    _vit_refused(call(stats=0), "null")
    _vit_refused(call(x=P + 4), "aligned")
    _vit_refused(call(stats=2 * P + 4), "aligned")
    _vit_refused(call(x16=3 * P + 2), "aligned")
    _vit_refused(call(xdt=L.MRA_F16, x=P + 2, xb=M * D * 2, x16=0, x16b=0), "aligned")
    _vit_refused(call(xb=M * D * 4 - 4), "x_bytes")
    _vit_refused(call(xdt=L.MRA_F16, xb=M * D * 2 - 2, x16=0, x16b=0), "x_bytes")
    _vit_refused(call(sb=M * 8 - 4), "stats_bytes")
    _vit_refused(call(x16b=M * D * 2 - 2), "x16_bytes")
