"""``-m gpu``: the folded cross-attention over RAW encoder features (no modality LayerNorm pass; csrc/gemm.hip CS = 1 / 2, csrc/mra_abi.hip
CrossPlan::raw, mra_qformer_forward_raw).

Launch level: the scores launch with column factors and in-kernel token statistics through ``mra_debug_gemm``, every case of
tests/raw_scores_cases.py against float64 of the rounded operands under that file's bounds (tests/test_raw_scores_cases_cpu.py holds the
fp32 emulation inside them); then the same launch again READING the factors the first one wrote (the form cross layers >= 1 run), which
must reproduce C and the statistics bit for bit.

Forward level: a small Q-Former that still runs the 176 x 384 tiles (12 heads x 32 queries, hidden 768, 4 layers = two cross layers, so the
second reads the stored factors) against the oracle, against LayerNorm + the folded path, after a reload of ln.weight, and through every
condition under which the raw form must not be taken.  The encoder width is 704: the smallest multiple of both 176 (the P . enc tile) and 64
(a K step; mra_qformer_create refuses any other width)."""
import ctypes
import time

import pytest
import torch

import raw_scores_cases as R
from mraudio_amd import _lib as L
from oracle import qformer_ref as O
from test_gpu_parity import Z_ATOL, build_qformer, oracle_cfg
from test_gpu_qformer_kernels import DEV, GUARD, Buf, _bits, _ok, _stream
from tools.make_golden import make_inputs

pytestmark = pytest.mark.gpu
GF_WS_176x384, EPI_SOFTPART, GT_WS_176x384 = 6, 5, 5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device(DEV)


# =========================================================================================================================================
# launch level
# =========================================================================================================================================
def _after(buf, what):
    bits = _bits(buf.buf).cpu()
    for sl in (slice(0, GUARD), slice(GUARD + buf.numel, None)):
        assert torch.equal(bits[sl], buf.before[sl]), f"{what}: a guard was written"
    return buf.inner.cpu()


def _launch(c, dt, ins, col_scale=None):
    """The scores launch of case c; col_scale None: col_stats = 1 (the launch computes and writes the factors), else they are read."""
    dtype = R.DTYPES[dt]
    outs = {k: Buf(v.numel(), v.dtype) for k, v in R.fresh_outputs(c, dt).items()}
    if col_scale is not None:
        outs["col_scale"] = col_scale
    B, M, N, K, ld = c["batch"], c["M"], c["N"], c["K"], R.fold_kvp(c["N"])
    d = L.mra_gemm_desc()
    d.struct_bytes = ctypes.sizeof(L.mra_gemm_desc)
    for name, buf in (("A", ins["A"]), ("W", ins["W"]), ("C", outs["C"]), ("stat_m", outs["stat_m"]), ("stat_l", outs["stat_l"]),
                      ("col_scale", outs["col_scale"])):
        setattr(d, name, buf.inner.data_ptr())
        setattr(d, {"A": "a_bytes", "W": "w_bytes", "C": "c_bytes"}.get(name, name + "_bytes"), buf.numel * buf.inner.element_size())
    d.a_view[:] = (0, M, K)
    d.c_view[:] = (0, M, ld)
    d.M, d.N, d.K = M, N, K
    d.batch, d.a_bs, d.w_bs, d.c_bs_bytes = B, M * K, N * K, M * ld * 2
    d.n_ragged = 1
    d.alpha = R.ALPHA
    d.tile_cfg = GT_WS_176x384
    d.cs_bs, d.col_stats, d.cs_eps = ld, int(col_scale is None), R.EPS
    before = L.gemm_launches(GF_WS_176x384, EPI_SOFTPART)
    _ok(L.lib().mra_debug_gemm(d, 1, EPI_SOFTPART, L.mra_dtype(dtype), _stream()), f"mra_debug_gemm {c['name']}")
    assert L.gemm_launches(GF_WS_176x384, EPI_SOFTPART) - before == 1
    for k, buf in ins.items():
        buf.unchanged(k)
    return outs, {k: _after(buf, k) for k, buf in outs.items()}


@pytest.mark.parametrize("name,dt", [(c["name"], "f16") for c in R.CASES] + [(R.CASES[5]["name"], "bf16"), (R.CASES[-1]["name"], "bf16")])
def test_scores_launch_with_in_kernel_token_statistics(name, dt, dev):
    t0 = time.time()
    c = R.BY_NAME[name]
    d = R.inputs(name, dt)
    ins = {"A": Buf(d["A"].numel(), d["A"].dtype, d["A"]), "W": Buf(d["W"].numel(), d["W"].dtype, d["W"])}
    bufs, outs = _launch(c, dt, ins)
    ratios, fails = R.check(name, dt, outs)
    ref = R.reference(name, dt)
    B, N, ld = c["batch"], c["N"], R.fold_kvp(c["N"])
    err = R.r_error(ref, outs["col_scale"][:B * ld].view(B, ld)[:, :N])
    print(f"{name} {dt}: r error {err / R.U32:.1f} u32 (bar {R.r_bar(dt) / R.U32:.1f} u32); |d| / bound " +
          ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()) + f"  [{time.time() - t0:.1f} s]")
    assert not fails, fails[:8]
    # the later cross layers' form: the same launch reading the factors just written gives the same bits
    again, outs2 = _launch(c, dt, ins, col_scale=bufs["col_scale"])
    for k in ("C", "stat_m", "stat_l", "col_scale"):
        assert torch.equal(_bits(outs2[k]), _bits(outs[k])), f"{k} differs when the factors are read instead of computed"


# =========================================================================================================================================
# forward level
# =========================================================================================================================================
E_SMALL = 704


@pytest.fixture(scope="module")
def small(dev):
    qf, cfg = build_qformer(dev, E_SMALL, seed=11, layers=4)
    assert (cfg.heads, cfg.n_query, cfg.hidden, cfg.cross_freq) == (12, 32, 768, 2)
    qf.set_cross_mode("fold")
    return qf, cfg, O.init_weights(oracle_cfg(cfg), seed=11, perturb=True)


def _features(ocfg, kv, seed):
    """N 3, L 5; encoder features with a token mean of the order of their spread, rounded to f16 (what an f16 encoder hands over)."""
    ids, tmask, att, feats = make_inputs(ocfg, 3, 5, kv, seed, True)
    g = torch.Generator().manual_seed(seed + 1)
    feats = feats * (0.5 + torch.rand(3, kv, 1, generator=g)) + (2.0 * torch.rand(3, kv, 1, generator=g) - 1.0)
    return ids, att, feats.half()


def _run(qf, dev, ids, att, x, item_index=None):
    """What XInstructBLIP.fuse_score does per modality: the raw form where the library allows it, LayerNorm + forward otherwise."""
    raw = qf.raw_features_ok(x, item_index=item_index)
    enc = x if raw else qf.modality_ln(x, item_index=item_index)
    out = qf.forward_fused(ids.to(dev), att.to(dev), enc, want_query=True, want_cls=True, raw=raw)
    return raw, out


@pytest.mark.parametrize("kv", [176, 300])
def test_raw_forward_matches_the_oracle_and_the_layernorm_path(kv, small, dev):
    qf, cfg, w = small
    ocfg = oracle_cfg(cfg)
    ids, att, x16 = _features(ocfg, kv, 40 + kv)
    x = x16.to(dev)
    raw, got = _run(qf, dev, ids, att, x)
    assert raw, "the folded form on the 176 x 384 tiles must take raw features"
    qf.set_option("raw_features", 0)
    try:
        raw0, ref = _run(qf, dev, ids, att, x)
    finally:
        qf.set_option("raw_features", 1)
    assert not raw0
    h = O.qformer_forward(w, ocfg, ids, att, w["query_tokens"].expand(3, -1, -1), O.modality_layernorm(x16.float(), w["ln.weight"], w["ln.bias"]))
    e_or = (got["query"].cpu() - h[:, :32]).abs().max().item()
    e_ln = max((got[k] - ref[k]).abs().max().item() for k in ("query", "cls"))
    e_ref = (ref["query"].cpu() - h[:, :32]).abs().max().item()
    print(f"kv {kv}: raw vs oracle {e_or:.3e} (LayerNorm path vs oracle {e_ref:.3e}), raw vs LayerNorm path {e_ln:.3e}")
    assert e_or < Z_ATOL
    assert e_ln < 5e-3


def test_outputs_follow_a_reloaded_ln_weight(small, dev):
    qf, cfg, w = small
    ocfg = oracle_cfg(cfg)
    ids, att, x16 = _features(ocfg, 300, 77)
    x = x16.to(dev)
    _, before = _run(qf, dev, ids, att, x)
    g0, b0 = w["ln.weight"].clone(), w["ln.bias"].clone()
    gen = torch.Generator().manual_seed(5)
    g1 = g0 * (1.0 + 0.5 * torch.rand(g0.shape, generator=gen))
    b1 = b0 + 0.3 * torch.randn(b0.shape, generator=gen)
    try:
        qf.push("ln.weight", g1)
        qf.push("ln.bias", b1)
        raw, got = _run(qf, dev, ids, att, x)
        assert raw
        h = O.qformer_forward(w, ocfg, ids, att, w["query_tokens"].expand(3, -1, -1), O.modality_layernorm(x16.float(), g1, b1))
        moved = (got["query"] - before["query"]).abs().max().item()
        err = (got["query"].cpu() - h[:, :32]).abs().max().item()
        print(f"reloaded ln: outputs moved by {moved:.3e}, error against the oracle with the new parameters {err:.3e}")
        assert err < Z_ATOL and moved > 10 * err
    finally:
        qf.push("ln.weight", g0)
        qf.push("ln.bias", b0)
        qf.sync_weights()


def test_forms_that_must_not_take_raw_features_are_unchanged(small, dev):
    qf, cfg, w = small
    ocfg = oracle_cfg(cfg)
    ids, att, x16 = _features(ocfg, 300, 91)
    x = x16.to(dev)
    idx = torch.tensor([2, 0, 1], device=dev)

    def both(x, item_index=None):
        """(raw taken with the option on, outputs with it on, outputs with it off)"""
        raw, on = _run(qf, dev, ids, att, x, item_index)
        qf.set_option("raw_features", 0)
        try:
            raw0, off = _run(qf, dev, ids, att, x, item_index)
        finally:
            qf.set_option("raw_features", 1)
        assert not raw0
        return raw, on, off

    def same(on, off):
        return all(torch.equal(_bits(on[k]), _bits(off[k])) for k in ("query", "cls"))

    assert qf.raw_features_ok(x)
    # an index gather; an fp32 input; a non-contiguous input
    for what, xx, ii in (("gather", x, idx), ("fp32", x.float(), None), ("strided", x.transpose(0, 1).contiguous().transpose(0, 1), None)):
        raw, on, off = both(xx, ii)
        assert not raw and same(on, off), what
    try:
        qf.set_cross_mode("kv_cache")
        raw, on, off = both(x)
        assert not raw and same(on, off), "kv_cache"
        for mode in ("fold_stream", "fold_rescale_pass"):   # the streaming kernels; the rescale pass over P instead of in-register factors
            qf.set_cross_mode(mode)
            assert not qf.raw_features_ok(x), mode
        qf.set_cross_mode("fold")
        qf.set_cross_precision("split")
        raw, on, off = both(x)
        assert not raw and same(on, off), "split precision"
        qf.set_cross_precision("auto")                     # a probe is pending
        assert not qf.raw_features_ok(x)
        assert not _run(qf, dev, ids, att, x)[0]
        rep = qf.cross_precision_report()
        assert rep["probes"] >= 1 and rep["resolved"] in ("op", "split")
        assert qf.raw_features_ok(x) == (rep["resolved"] == "op")   # resolved: the op chain may take raw features again
        qf.set_cross_precision("auto")                     # the probing forward itself, with the option on and off
        _, p_on = _run(qf, dev, ids, att, x)
        qf.set_cross_precision("auto")
        qf.set_option("raw_features", 0)
        _, p_off = _run(qf, dev, ids, att, x)
        assert same(p_on, p_off), "probe"
    finally:
        qf.set_option("raw_features", 1)
        qf.set_cross_precision("op")
        qf.set_cross_mode("fold")
    assert qf.raw_features_ok(x)
    # asking for the raw entry where it does not apply is an error, not a silent fall-back
    qf.set_cross_mode("kv_cache")
    try:
        with pytest.raises(Exception):
            qf.forward_fused(ids.to(dev), att.to(dev), x, want_query=True, raw=True)
    finally:
        qf.set_cross_mode("fold")
