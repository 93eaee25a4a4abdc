"""``-m gpu``: the GEMM launches only the ViT-g encoder issues (csrc/vit.hip: QKV, projection, fc1, fc2 and the patch embedding), one launch each
through ``mra_debug_gemm``, and the three small kernels of its folded LayerNorm through ``mra_debug_vit_*``, for every case of
``tests/vit_gemm_cases.py`` in f16 and bf16, against float64 references on the same rounded inputs under the DERIVED bounds of that file (nothing
there was fitted to this file's output; tests/test_vit_gemm_cases_cpu.py holds the fp32 emulations inside every bound and the named mutants
outside).  Every test asserts the family that ran (the launch counters) and max |d| / bound <= 1, and prints the ratio.

Canaries as tests/test_gpu_gemm_forward.py: every output buffer is all-ones bits between guards; after the launch exactly the owned elements
were rewritten, the guards are intact; inputs hold NaN wherever no view addresses them and come back bit for bit."""
import ctypes as C
import time

import pytest
import torch

import vit_gemm_cases as V
from mraudio_amd import _lib as L
from test_gpu_qformer_kernels import DEV, GUARD, Buf, _bits, _ok, _stream

pytestmark = pytest.mark.gpu
DTS = ["f16", "bf16"]


@pytest.fixture(scope="module", autouse=True)
def dev():
    assert torch.cuda.is_available()
    return torch.device(DEV)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _after(buf, what):
    """The inside of an output buffer on the CPU, after checking its guards."""
    bits = _bits(buf.buf).cpu()
    for sl in (slice(0, GUARD), slice(GUARD + buf.numel, None)):
        assert torch.equal(bits[sl], buf.before[sl]), f"{what}: a guard was written"
    return buf.inner.cpu()


def _nbytes(buf):
    return buf.numel * buf.inner.element_size()


def _launched():
    return [L.gemm_launches(f, e) for f in range(L.GEMM_FAMILIES) for e in range(16)]


def _buffers(c, dt):
    ins = {k: Buf(v.numel(), v.dtype, v) for k, v in V.inputs(c["name"], dt)["flat"].items()}
    outs = {k: Buf(v.numel(), v.dtype, v) for k, v in V.fresh_outputs(c, dt).items()}
    return ins, outs


def _addr(ins, outs):
    def addr(b):
        buf = ins.get(b) or outs.get(b)
        return None if buf is None else (buf.inner.data_ptr(), _nbytes(buf))
    return addr


def _launch(c, dt, persist=None):
    """One mra_debug_gemm call on fresh buffers.  Returns the outputs on the CPU."""
    ins, outs = _buffers(c, dt)
    arr = V.descriptor(c, dt, _addr(ins, outs), persist)
    fams = range(L.GEMM_FAMILIES)
    before = [L.gemm_launches(f, c["epi"]) for f in fams]
    _ok(L.lib().mra_debug_gemm(arr, 1, c["epi"], L.mra_dtype(V.DTYPES[dt]), _stream()), f"mra_debug_gemm {c['name']}")
    ran = [L.gemm_launches(f, c["epi"]) - b for f, b in zip(fams, before)]
    assert ran == [int(f == c["family"]) for f in fams], f"families launched {ran}, expected family {c['family']}"
    for k, buf in ins.items():
        buf.unchanged(k)
    return {k: _after(buf, k) for k, buf in outs.items()}


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", [c["name"] for c in V.CASES])
def test_vit_gemm_against_float64(name, dt):
    t0 = time.time()
    c = V.BY_NAME[name]
    if c["persist"]:      # the shape follows the device: strictly between one and two rounds of its compute units
        cus = _cus()
        c = next(p for p in V.persist_cases(cus) if p["epi"] == c["epi"])
        out = (C.c_int32 * 7)()
        arr = V.descriptor(c, dt, V.fake_addr(c, dt))
        assert L.lib().mra_debug_gemm_plan(arr, 1, c["epi"], L.mra_dtype(V.DTYPES[dt]), cus, out) == 0, L.lib().mra_last_error()
        assert out[1] == V.GF_P8_256 and out[5] == 1 and out[4] == cus & ~7 and cus < out[6] < 2 * cus, list(out)
    outs = _launch(c, dt)
    ratios, fails = V.check(c["name"], dt, outs)
    if c["persist"]:
        per_tile = _launch(c, dt, persist=0)
        same = torch.equal(_bits(outs["C"]), _bits(per_tile["C"]))
        ratios["persistent == per tile"] = 0.0 if same else float("inf")
        if not same:
            fails.append(f"{int((_bits(outs['C']) != _bits(per_tile['C'])).sum())} elements differ between the persistent and the per-tile launch")
    print(f"row {c['row']} {c['name']} {dt} (family {c['family']}): |d| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()) +
          f"  [{time.time() - t0:.1f} s]")
    assert not fails, fails[:8]
    assert all(v <= 1.0 for v in ratios.values()), ratios


# =========================================================================================================================================
# the companion kernels
# =========================================================================================================================================
def _fold_weight(f, dtype):
    N, K = f["w"].shape
    W, gain, beta = Buf(N * K, dtype, f["w"]), Buf(K, torch.float32, f["gain"]), Buf(K, torch.float32, f["beta"])
    bias = Buf(N, torch.float32, f["bias"]) if f["bias"] is not None else None
    Wf, cs, bf = Buf(N * K, dtype), Buf(N, torch.float32), Buf(N, torch.float32)
    _ok(L.lib().mra_debug_vit_fold_weight(W.ptr, _nbytes(W), gain.ptr, _nbytes(gain), beta.ptr, _nbytes(beta), bias.ptr if bias else None,
                                          _nbytes(bias) if bias else 0, Wf.ptr, _nbytes(Wf), cs.ptr, _nbytes(cs), bf.ptr, _nbytes(bf), N, K,
                                          L.mra_dtype(dtype), _stream()), "mra_debug_vit_fold_weight")
    for name, b in (("W", W), ("gain", gain), ("beta", beta), ("bias", bias)):
        if b:
            b.unchanged(name)
    return Wf.result(True, "Wf").view(N, K), cs.result(True, "cs"), bf.result(True, "bf")


def _group_stats(groups, n, eps, tail=0):
    M, Gn = groups.shape[:2]
    gb, st = Buf(M * Gn * 2, torch.float32, groups), Buf(M * 2 + tail, torch.float32)
    _ok(L.lib().mra_debug_vit_group_stats(gb.ptr, _nbytes(gb), M, Gn, n, eps, st.ptr, _nbytes(st), _stream()), "mra_debug_vit_group_stats")
    gb.unchanged("groups")
    w = torch.zeros(M * 2 + tail, dtype=torch.bool)
    w[:M * 2] = True
    return st.result(w, "stats")[:M * 2].view(M, 2)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("N,K,with_bias", V.FOLD_CASES)
def test_vit_fold_weight(N, K, with_bias, dt):
    dtype = V.DTYPES[dt]
    f = V.fold_case(N, K, with_bias, dt)
    r = V.fold_weight_check(f, *_fold_weight(f, dtype), dtype)
    print(f"row 11 vit_fold_weight N{N} K{K} bias {with_bias} {dt}: |d| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r


@pytest.mark.parametrize("M,Gn,n", V.GROUP_CASES)
def test_vit_group_stats(M, Gn, n):
    x, groups = V.group_case(M, Gn, n)
    st = _group_stats(groups, n, V.VIT_EPS, tail=V.STAT_GUARD)
    ra, _ = V.group_stats_check(groups, n, V.VIT_EPS, st)
    rb, _ = V.group_stats_check(groups, n, V.VIT_EPS, st, row=x)
    print(f"row 11 vit_group_stats M{M} G{Gn} n{n}: |d| / bound merge " + ", ".join(f"{k} {v:.3f}" for k, v in ra.items()) + "; rows " +
          ", ".join(f"{k} {v:.3f}" for k, v in rb.items()))
    assert all(v <= 1.0 for v in list(ra.values()) + list(rb.values())), (ra, rb)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("f32", [True, False])
@pytest.mark.parametrize("M,D", V.ROWSTAT_CASES)
def test_vit_row_stats(M, D, f32, dt):
    dtype = V.DTYPES[dt]
    x = V.rowstat_case(M, D, dt, f32)
    xb, st = Buf(M * D, x.dtype, x), Buf(M * 2, torch.float32)
    x16 = Buf(M * D, dtype) if f32 else None
    _ok(L.lib().mra_debug_vit_row_stats(xb.ptr, _nbytes(xb), L.mra_dtype(x.dtype), M, D, V.VIT_EPS, st.ptr, _nbytes(st), x16.ptr if f32 else None,
                                        _nbytes(x16) if f32 else 0, L.mra_dtype(dtype), _stream()), "mra_debug_vit_row_stats")
    xb.unchanged("x")
    r = V.row_stats_check(x, V.VIT_EPS, st.result(True, "stats").view(M, 2), x16.result(True, "x16").view(M, D) if f32 else None, dtype)
    print(f"row 11 vit_row_stats M{M} D{D} {'f32' if f32 else dt} rows ({dt}): |d| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r


# =========================================================================================================================================
# the chain of the three
# =========================================================================================================================================
@pytest.mark.parametrize("dt", DTS)
def test_vit_ln_fold_chain(dt):
    """EPI_RES_F32_STAT -> vit_group_stats -> EPI_LNF_OP on the first launch's ln_y16 and the merged statistics, weights from vit_fold_weight,
    against the float64 LayerNorm(C returned) w^T + b."""
    dtype = V.DTYPES[dt]
    M, D, Nq = V.CHAIN["M"], V.CHAIN["D"], V.CHAIN["Nq"]
    c1, c2 = V.BY_NAME["chain proj RES_F32_STAT M300 N384 K256"], V.BY_NAME["chain qkv LNF_OP M300 N256 K384"]
    o1 = _launch(c1, dt)
    r1, fails = V.check(c1["name"], dt, o1)
    assert not fails, fails[:8]
    Cret = o1["C"][V.index(c1["c"], M, D)[0]]
    x16 = o1["ln_y16"][V.index(c1["y16"], M, D)[0]]
    groups = o1["ln_y32"][:M * (D // 128) * 2].view(M, D // 128, 2)
    stat = _group_stats(groups, 128, V.VIT_EPS)
    f = V.chain_fold(dt)
    Wf, cs, bf = _fold_weight(f, dtype)
    ins = dict(A=Buf(M * D, dtype, x16), W=Buf(Nq * D, dtype, Wf), bias=Buf(Nq, torch.float32, bf), ln_y32=Buf(M * 2, torch.float32, stat),
               ln_gain=Buf(Nq, torch.float32, cs))
    outs = dict(C=Buf(c2["c"]["numel"], dtype))
    before = L.gemm_launches(V.GF_P8_256, V.EPI_LNF_OP)
    _ok(L.lib().mra_debug_gemm(V.descriptor(c2, dt, _addr(ins, outs)), 1, V.EPI_LNF_OP, L.mra_dtype(dtype), _stream()), "chain qkv gemm")
    assert L.gemm_launches(V.GF_P8_256, V.EPI_LNF_OP) == before + 1
    for k, b in ins.items():
        b.unchanged(k)
    must = torch.zeros(c2["c"]["numel"], dtype=torch.bool)
    idx = V.index(c2["c"], M, Nq)[0]
    must[idx.reshape(-1)] = True
    out = outs["C"].result(must, "chain C")[idx]
    r = V.chain_check(dt, Cret, x16, stat, Wf, cs, bf, out)
    print(f"row 10 chain {dt}: |d| / bound first launch " + ", ".join(f"{k} {v:.3f}" for k, v in r1.items()) + f"; LayerNorm(C) w^T + b {r:.3f}")
    assert r <= 1.0


# =========================================================================================================================================
# refusals with real buffers: nothing ran
# =========================================================================================================================================
@pytest.mark.parametrize("name,change,word", [
    ("mixed RES_OP M600 N640 K256 separate", lambda d: setattr(d, "aux", d.C + 16), "overlaps"),
    ("mixed RES_OP M600 N640 K256 separate", lambda d: setattr(d, "aux_bytes", d.aux_bytes - 4096), "aux_bytes"),
    ("mixed RES_OP_STAT M520 N1408 K128 in place", lambda d: setattr(d, "ln_y32_bytes", 520 * 22 * 8 - 4), "ln_y32"),
    ("mixed RES_F32_STAT M776 N1408 K1408", lambda d: setattr(d, "ln_y16_bytes", d.ln_y16_bytes // 2), "ln_y16"),
    ("mixed RES_F32_STAT M776 N1408 K1408", lambda d: setattr(d, "K", 1344), "gemm_plan"),
    ("mixed RES_F32 M600 N384 K128", lambda d: setattr(d, "tile_cfg", V.GT_P8_TAIL), "tile_cfg"),
    ("p8_256 LNF_OP M300 N512 K1408 rows", lambda d: setattr(d, "ln_gain_bytes", 511 * 4), "ln_gain"),
    ("p8_256 LNF_GELU_OP M257 N256 K128", lambda d: setattr(d, "batch", 2), "one plain problem"),
    ("p8_256 LNF_GELU_OP M257 N256 K128", lambda d: setattr(d, "struct_bytes", d.struct_bytes - 16), "struct_bytes"),
])
def test_refusals_launch_nothing(name, change, word):
    c = V.BY_NAME[name]
    ins, outs = _buffers(c, "f16")
    arr = V.descriptor(c, "f16", _addr(ins, outs))
    change(arr[0])
    before = _launched()
    rc = L.lib().mra_debug_gemm(arr, 1, c["epi"], L.MRA_F16, _stream())
    msg = L.lib().mra_last_error().decode()
    torch.cuda.synchronize()
    assert rc == -1 and word in msg, (rc, msg)
    assert _launched() == before
    for k, b in list(ins.items()) + list(outs.items()):
        b.unchanged(k)


def test_companion_refusals_launch_nothing():
    f = V.fold_case(6, 384, True, "f16")
    W, gain, beta, bias = Buf(6 * 384, torch.float16, f["w"]), Buf(384, torch.float32, f["gain"]), Buf(384, torch.float32, f["beta"]), Buf(6, torch.float32, f["bias"])
    Wf, cs, bf = Buf(6 * 384, torch.float16), Buf(6, torch.float32), Buf(6, torch.float32)
    rc = L.lib().mra_debug_vit_fold_weight(W.ptr, _nbytes(W), gain.ptr, _nbytes(gain), beta.ptr, _nbytes(beta), bias.ptr, _nbytes(bias), Wf.ptr, _nbytes(Wf) - 2,
                                          cs.ptr, _nbytes(cs), bf.ptr, _nbytes(bf), 6, 384, L.MRA_F16, _stream())
    assert rc == -1 and b"wf_bytes" in L.lib().mra_last_error()
    x, groups = V.group_case(300, 3, 128)
    gb, st = Buf(300 * 3 * 2, torch.float32, groups), Buf(300 * 2, torch.float32)
    assert L.lib().mra_debug_vit_group_stats(gb.ptr, _nbytes(gb), 301, 3, 128, V.VIT_EPS, st.ptr, _nbytes(st), _stream()) == -1
    xr = V.rowstat_case(5, 1408, "f16", True)
    xb, rs, x16 = Buf(5 * 1408, torch.float32, xr), Buf(10, torch.float32), Buf(5 * 1408, torch.float16)
    assert L.lib().mra_debug_vit_row_stats(xb.ptr, _nbytes(xb), L.MRA_F32, 5, 1408, V.VIT_EPS, rs.ptr, _nbytes(rs), x16.ptr, _nbytes(x16) - 2, L.MRA_F16,
                                          _stream()) == -1
    assert L.lib().mra_debug_vit_row_stats(xb.ptr, _nbytes(xb), L.MRA_F32, 5, 1400, V.VIT_EPS, rs.ptr, _nbytes(rs), x16.ptr, _nbytes(x16), L.MRA_F16,
                                          _stream()) == -1
    torch.cuda.synchronize()
    for k, b in (("W", W), ("Wf", Wf), ("cs", cs), ("bf", bf), ("groups", gb), ("stats", st), ("x", xb), ("row stats", rs), ("x16", x16)):
        b.unchanged(k)
