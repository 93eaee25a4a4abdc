"""Without a GPU: the case table of tests/gemm_cases.py is what tests/test_gpu_gemm_forward.py will launch, so here it is held to account
first -- every case resolves (mra_debug_gemm_plan, host only) to the kernel family it names, the table covers every (family, epilogue) pair
the forwards reach, the fp32 emulation of every form sits inside its derived bound (the ratios are printed), every named mutant falls outside
on at least one case of its row, and every refusal of mra_debug_gemm refuses before anything is launched."""
import ctypes as C

import pytest
import torch

import gemm_cases as G
from mraudio_amd import _lib as L

DTS = ("f16", "bf16")
ROWS = sorted({c["row"] for c in G.CASES})


def test_the_codes_repeat_the_bindings():
    for n in ("EPI_OP", "EPI_GELU_OP", "EPI_RES_F32", "EPI_F32", "EPI_KV", "EPI_SOFTPART", "EPI_RES_LN", "GT_AUTO", "GT_64", "GT_128", "GT_256",
              "GT_WS_128x384", "GT_WS_176x384", "GT_K128_64x128", "GT_RING_144x128", "GT_RING_192x128", "GT_RING_96x64", "GF_V1_64", "GF_V1_128",
              "GF_WS_256", "GF_P8_256", "GF_WS_128x384", "GF_WS_176x384", "GF_K128_64x128", "GF_K128_64x64", "GF_RING_144x128", "GF_RING_192x128",
              "GF_RING_96x64"):
        assert getattr(G, n) == getattr(L, n), n
    assert abs(G.LOG2E - 1.4426950408889634) < 1e-15


def test_the_table_covers_every_pair_the_forwards_reach():
    have = {(c["family"], c["epi"]) for c in G.CASES}
    assert have == set(G.PAIRS), (sorted(set(G.PAIRS) - have), sorted(have - set(G.PAIRS)))
    assert ROWS == list(range(1, 16))
    assert all(G.ROW_MUTANTS[r] for r in ROWS)


def _plan(c, dt, cus=G.CUS):
    out = (C.c_int32 * 7)()
    arr = G.descriptors(c, dt, G.fake_addr(c, dt))
    rc = L.lib().mra_debug_gemm_plan(arr, len(c["probs"]), c["epi"], L.mra_dtype(G.DTYPES[dt]), cus, out)
    return rc, list(out)


@pytest.mark.parametrize("row", ROWS)
def test_every_case_resolves_to_the_family_it_names(row):
    """tile, family, threads, LDS bytes, grid, persistent, total tiles of every case at 256 CUs: the family is the table's, only the
    persistent case is persistent (its grid is the CU count, below its tile count), and the tile count is the one the shapes give."""
    for c in G.cases_of(row):
        for dt in DTS:
            rc, (tile, family, threads, lds, grid, persistent, tiles) = _plan(c, dt)
            assert rc == 0, (c["name"], L.lib().mra_last_error())
            assert family == c["family"], (c["name"], family)
            assert c["tile"] in (G.GT_AUTO, tile), (c["name"], tile)
            want_persistent = "persistent" in c["name"]
            assert persistent == int(want_persistent), c["name"]
            assert grid == (G.CUS if want_persistent else tiles), (c["name"], grid, tiles)
            assert threads in (256, 512, 768) and 0 < lds <= 160 * 1024
            if want_persistent:
                assert tiles == 17 * 36 and tiles > G.CUS


def _run_emulation(c, dt, mutant=None):
    """The emulated launch through ``check``; an EPI_RES_LN case launches twice on the same counters, as the GPU test does."""
    outs, cnt = G.emulate(c["name"], dt, mutant)
    ratios, fails = G.check(c["name"], dt, outs, cnt)
    if c["epi"] == G.EPI_RES_LN:
        outs2, cnt2 = G.emulate(c["name"], dt, mutant, counters=cnt)
        r2, f2 = G.check(c["name"], dt, outs2, cnt2)
        ratios = {k: max(v, r2.get(k, 0.0)) for k, v in ratios.items()}
        fails = fails + ["second launch: " + f for f in f2]
    return ratios, fails


@pytest.mark.parametrize("row", ROWS)
def test_faithful_emulations_are_inside_their_bounds(row):
    worst, failures = {}, []
    for c in G.cases_of(row):
        for dt in DTS:
            ratios, fails = _run_emulation(c, dt)
            for k, v in ratios.items():
                worst[(dt, k)] = max(worst.get((dt, k), (0.0, ""))[0:2], (v, c["name"]))
            failures += [(c["name"], dt, f) for f in fails]
    print(f"row {row}: worst emulated |d| / bound " + ", ".join(f"{dt} {k} {v:.3f} ({n})" for (dt, k), (v, n) in sorted(worst.items())))
    assert not failures, failures[:10]
    assert all(0.0 <= v <= 1.0 for v, _ in worst.values())


@pytest.mark.parametrize("row,mutant", [(r, m) for r in ROWS for m in G.ROW_MUTANTS[r]])
def test_every_mutant_is_outside_its_bound(row, mutant):
    """A mutant must fail ``check`` (a ratio above 1, an owned element unwritten, an element written outside) on at least one case of its
    row, in both operand types."""
    for dt in DTS:
        caught = None
        for c in G.cases_of(row):
            if c["heavy"]:
                continue
            ratios, fails = _run_emulation(c, dt, mutant)
            if fails:
                caught = (c["name"], fails[0])
                break
        assert caught, f"{mutant} ({dt}) passes every case of row {row}"
        print(f"{mutant} {dt}: caught by {caught[0]}: {caught[1]}")


# =========================================================================================================================================
# refusals: nothing may reach a launch
# =========================================================================================================================================
def _launched():
    return sum(L.gemm_launches(f, e) for f in range(L.GEMM_FAMILIES) for e in range(16))


def _refused(arr, n, epi, dt="f16", word=None):
    before = _launched()
    rc = L.lib().mra_debug_gemm(arr, n, epi, L.mra_dtype(G.DTYPES[dt]), None)
    msg = L.lib().mra_last_error().decode()
    assert rc == -1, (rc, msg)
    assert _launched() == before
    if word:
        assert word in msg, msg
    return msg


def _desc(name, dt="f16"):
    c = G.BY_NAME[name]
    return c, G.descriptors(c, dt, G.fake_addr(c, dt))


def _need(l, rows, cols, batch=1, esz=2):
    """Bytes from a layout's first element to the end of its last: the footprint mra_debug_gemm computes."""
    return (int(G.index(l, rows, cols, batch).max()) + 1 - l["off"]) * esz


def _exactly(name, field, need, n=None, word=None):
    """The footprint itself passes every host check (mra_debug_gemm_plan makes the same ones and launches nothing); one element less is refused
    by both entries."""
    c, arr = _desc(name)
    k = int(field.split(":")[0]) if ":" in field else 0
    f = field.split(":")[-1]
    n = n or len(c["probs"])
    setattr(arr[k], f, need)
    out = (C.c_int32 * 7)()
    assert L.lib().mra_debug_gemm_plan(arr, n, c["epi"], L.MRA_F16, G.CUS, out) == 0, (name, field, L.lib().mra_last_error())
    setattr(arr[k], f, need - 2)
    assert L.lib().mra_debug_gemm_plan(arr, n, c["epi"], L.MRA_F16, G.CUS, out) == -1
    return _refused(arr, n, c["epi"], word=word or f)


PLAIN = "v1_64 RES_F32 M70 K192 views"
GROUPS = "v1_64 OP groups 64/27/70/3 K768"
RAGGED = "scores F32 ragged M96 N300 K192 batch3"
SOFT = "scores SOFTPART M200 kv177 K192 batch2 peaked"
KWRAP = "scores SOFTPART M384 kv530 K384 batch2 mild kwrap"
PENC = "p.enc OP M200 E352 kv300 batch2 pscale"
KV = "kv GT_128 M514 tok257 K192"
LN2 = "ring96 RES_LN groups 203/70 K448 both"
CTX = "context GT_64 OP M96 E192"


def test_the_unchanged_descriptors_pass_the_host_checks():
    """The same descriptors the refusals below start from are accepted by the plan entry (what is refused is the change, not the base)."""
    for name in (PLAIN, GROUPS, RAGGED, SOFT, KWRAP, PENC, KV, LN2, CTX):
        rc, _ = _plan(G.BY_NAME[name], "f16")
        assert rc == 0, name


def test_launch_level_refusals():
    c, arr = _desc(PLAIN)
    _refused(arr, 0, c["epi"], word="1 .. 4")
    _refused(arr, 5, c["epi"], word="1 .. 4")
    _refused(None, 1, c["epi"], word="null")
    for epi in (6, 7, 14, 15, -1, 16):      # (8 and 10 .. 13 are the ViT's: tests/test_vit_gemm_cases_cpu.py)
        _refused(arr, 1, epi, word="epilogue")
    before = _launched()
    assert L.lib().mra_debug_gemm(arr, 1, c["epi"], L.MRA_F32, None) == -1 and _launched() == before
    arr[0].struct_bytes -= 8
    _refused(arr, 1, c["epi"], word="struct_bytes")


@pytest.mark.parametrize("field,change,word", [
    ("A", lambda d: 0, "null"), ("W", lambda d: 0, "null"), ("C", lambda d: 0, "null"), ("R", lambda d: 0, "residual"),
    ("A", lambda d: d.A + 2, "aligned"), ("W", lambda d: d.W + 8, "aligned"), ("C", lambda d: d.C + 4, "aligned"), ("R", lambda d: d.R + 4, "aligned"),
    ("bias", lambda d: d.bias + 4, "aligned"),
    ("M", lambda d: 0, "positive"), ("N", lambda d: -128, "positive"), ("K", lambda d: 96, "gemm_plan"), ("N", lambda d: 96, "gemm_plan"),
    ("tile_cfg", lambda d: 7, "tile_cfg"), ("tile_cfg", lambda d: 12, "tile_cfg"), ("batch", lambda d: -1, "batch"), ("n_ragged", lambda d: 2, "n_ragged"),
    ("w_bytes", lambda d: d.w_bytes - 2, "w_bytes"), ("bias_bytes", lambda d: d.bias_bytes - 4, "bias_bytes"), ("r_bytes", lambda d: d.r_bytes - 4, "r_bytes"),
    ("M", lambda d: d.M + 6, "leave"),
])
def test_one_problem_refusals(field, change, word):
    """RES_F32 through item views (rows [3, 8) of 9-row items): one field changed at a time."""
    c, arr = _desc(PLAIN)
    setattr(arr[0], field, change(arr[0]))
    _refused(arr, 1, c["epi"], word=word)


@pytest.mark.parametrize("view,idx,value,word", [
    ("a_view", 2, 196, "A view"), ("a_view", 0, 9 * 200 + 4, "A view"), ("a_view", 1, 0, "A view"), ("a_view", 2, 184, "below K"),
    ("c_view", 2, 134, "C view"), ("c_view", 2, 124, "C row stride"), ("c_view", 0, -1224, "C view"), ("r_view", 2, 124, "R row stride"),
    ("c_view", 0, 1 << 40, "c_bytes"), ("a_view", 0, 1 << 62, "a_bytes"),
])
def test_view_refusals(view, idx, value, word):
    c, arr = _desc(PLAIN)
    getattr(arr[0], view)[idx] = value
    _refused(arr, 1, c["epi"], word=word)


def test_footprints_are_exact():
    """Sizes cut to the last element a view addresses pass; one element less is refused (the buffers of the table have rows to spare)."""
    p = G.BY_NAME[PLAIN]["probs"][0]
    _exactly(PLAIN, "a_bytes", _need(p["a"], 70, 192))
    _exactly(PLAIN, "c_bytes", _need(p["c"], 70, 128, esz=4))
    _exactly(PLAIN, "r_bytes", _need(p["r"], 70, 128, esz=4))
    p = G.BY_NAME[RAGGED]["probs"][0]
    _exactly(RAGGED, "c_bytes", _need(p["c"], 96, 384, 3, esz=4))      # 384 = ceil(300 / 128) * 128 columns, the third batch entry's last row
    _exactly(RAGGED, "a_bytes", _need(p["a"], 96, 192, 3))
    p = G.BY_NAME[CTX]["probs"][0]
    _exactly(CTX, "a_bytes", _need(p["a"], 96, 192, 3))                 # items_view(R E, 32, E) + the head's 32 rows
    _exactly(CTX, "c_bytes", _need(p["c"], 96, 64, 3))
    p = G.BY_NAME[SOFT]["probs"][0]
    _exactly(SOFT, "c_bytes", _need(p["c"], 200, 352, 2))               # kv = 177: two tiles of 176 columns
    p = G.BY_NAME[LN2]["probs"]
    _exactly(LN2, "ln_y32_bytes", _need(p[0]["y32"], 203, 768, esz=4))
    _exactly(LN2, "1:ln_y16_bytes", _need(p[1]["y16"], 70, 768))
    _exactly(LN2, "1:ln_counter_bytes", 4 * 2, word="ln_counter")
    p = G.BY_NAME[GROUPS]["probs"]
    assert "problem 3" in _exactly(GROUPS, "3:c_bytes", _need(p[3]["c"], 3, 128))


def test_a_later_problem_of_a_group_is_checked_too():
    c, arr = _desc(GROUPS)
    arr[2].bias_bytes = 0
    assert "problem 2" in _refused(arr, 4, c["epi"], word="bias_bytes")


def test_batched_and_ragged_refusals():
    c, arr = _desc(RAGGED)
    arr[0].c_view[2] = 380                                    # N = 300 fits, the 384 columns a ragged launch writes do not
    _refused(arr, 1, c["epi"], word="C row stride")
    c, arr = _desc(RAGGED)
    arr[0].w_bytes -= 2
    _refused(arr, 1, c["epi"], word="w_bytes")
    c, arr = _desc(RAGGED)
    arr[0].a_bs = -8
    _refused(arr, 1, c["epi"], word="batch")
    for f, v in (("a_bs", 4), ("w_bs", 12), ("c_bs_bytes", 8)):
        c, arr = _desc(RAGGED)
        setattr(arr[0], f, getattr(arr[0], f) + v)
        _refused(arr, 1, c["epi"], word="batch strides")
    c, arr = _desc(CTX)
    arr[0].bias_bytes -= 4                                    # bias + (batch - 1) * bias_bs + N floats
    _refused(arr, 1, c["epi"], word="bias_bytes")
    c, arr = _desc(CTX)
    arr[0].bias_bs = 66
    _refused(arr, 1, c["epi"], word="batch strides")


def test_softpart_and_pscale_refusals():
    c, arr = _desc(SOFT)
    arr[0].stat_m_bytes = 4 * 2 * 200 * 2 - 4                 # batch * M * ntiles floats
    _refused(arr, 1, c["epi"], word="stat_m")
    c, arr = _desc(SOFT)
    arr[0].stat_l = 0
    _refused(arr, 1, c["epi"], word="stat_m and stat_l")
    c, arr = _desc(SOFT)
    arr[0].alpha = 0.0
    _refused(arr, 1, c["epi"], word="alpha")
    c, arr = _desc(SOFT)
    arr[0].c_view[2] = 348                                    # kv = 177 needs 2 tiles = 352 columns
    _refused(arr, 1, c["epi"], word="C row stride")
    c, arr = _desc(SOFT)
    arr[0].tile_cfg = G.GT_128
    _refused(arr, 1, c["epi"], word="no such epilogue")
    c, arr = _desc(KWRAP)
    assert arr[0].w_bytes == 2 * 2 * 530 * 192                # K / 2 columns per weight row: allocated exactly
    arr[0].w_bytes -= 2
    _refused(arr, 1, c["epi"], word="w_bytes")
    c, arr = _desc(PENC)
    arr[0].pscale_bytes = 4 * 2 * 2 * 512 - 4                 # batch * ps_ntiles * 512 floats
    _refused(arr, 1, c["epi"], word="pscale_bytes")
    c, arr = _desc(PENC)
    arr[0].M = 385
    _refused(arr, 1, c["epi"], word="M <= 384")
    c, arr = _desc(PENC)
    arr[0].w_bytes -= 2                                       # (k_rows - 1) * w_ld + N elements, + the batch stride
    _refused(arr, 1, c["epi"], word="w_bytes")
    c, arr = _desc(PENC)
    arr[0].w_ld = 344
    _refused(arr, 1, c["epi"], word="w_ld")
    c, arr = _desc(PENC)
    arr[0].pscale += 4
    _refused(arr, 1, c["epi"], word="pscale")


def test_kv_refusals():
    c, arr = _desc(KV)
    arr[0].c_bytes -= 2                                       # 4 x items x heads x tokens x 64 elements
    _refused(arr, 1, c["epi"], word="scatter")
    c, arr = _desc(KV)
    arr[0].kv_heads = 3
    _refused(arr, 1, c["epi"], word="multiple of kv_heads")
    c, arr = _desc(KV)
    arr[0].kv_items = 1
    _refused(arr, 1, c["epi"], word="exceeds kv_items")
    c, arr = _desc(KV)
    arr[0].kv_tokens = 0
    _refused(arr, 1, c["epi"], word="kv_tokens")
    c, arr = _desc(KV)
    arr[0].batch = 2
    _refused(arr, 1, c["epi"], word="no batch")


def test_layernorm_refusals():
    c, arr = _desc(LN2)
    arr[1].ln_counter = arr[0].ln_counter + 4 * 3             # problem 0 owns ceil(203 / 64) = 4 counters
    _refused(arr, 2, c["epi"], word="overlap")
    c, arr = _desc(LN2)
    arr[1].ln_counter_bytes = 4
    _refused(arr, 2, c["epi"], word="ln_counter")
    for f in ("ln_gain_bytes", "ln_bias_bytes"):
        c, arr = _desc(LN2)
        setattr(arr[0], f, 4 * 768 - 4)
        _refused(arr, 2, c["epi"], word="ln_gain")
    c, arr = _desc(LN2)
    arr[0].ln_y32, arr[0].ln_y16 = 0, 0
    _refused(arr, 2, c["epi"], word="output")
    c, arr = _desc(LN2)
    arr[0].ln_y32_view[2] = 764
    _refused(arr, 2, c["epi"], word="ln_y32")
    c, arr = _desc(LN2)
    arr[0].ln_counter = 0
    _refused(arr, 2, c["epi"], word="counters")
    c, arr = _desc(LN2)
    arr[0].tile_cfg = G.GT_64
    _refused(arr, 2, c["epi"], word="no such epilogue")


def test_the_plan_entry_refuses_without_a_gpu_too():
    c, arr = _desc(PLAIN)
    out = (C.c_int32 * 7)()
    assert L.lib().mra_debug_gemm_plan(arr, 1, c["epi"], L.MRA_F16, 256, None) == -1
    assert L.lib().mra_debug_gemm_plan(arr, 1, c["epi"], L.MRA_F16, -1, out) == -1
    arr[0].K = 100
    assert L.lib().mra_debug_gemm_plan(arr, 1, c["epi"], L.MRA_F16, 256, out) == -1


def test_constant_fold_kvp():
    assert [G.fold_kvp(k) for k in (150, 176, 177, 300, 530, 1000)] == [256, 256, 384, 384, 768, 1152]
    assert torch.tensor(G.ALPHA, dtype=torch.float32).item() == G.ALPHA
