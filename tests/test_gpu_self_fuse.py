"""``-m gpu``: the Q|K|V projection and the masked self-attention core of a layer in ONE launch (csrc/attention.hip qkv_attn_kernel;
mra_qformer_set_option "self_fuse").

Launch level: ``mra_debug_qkv_attention`` at H = 768, 12 heads, N in {1, 2, 3} (a single item, a full group, a ragged group), L in {1, 8, 32}
(S = 33, 40, 64: the partial second query block and the full one), f16 and bf16, masks with padded text tails and one item whose text is fully
padded, every buffer between sentinel guards -- against the two launches it replaces (``mra_debug_gemm`` on the ring tile the forward runs at
the headline shape, then ``mra_debug_self_attention``) and against a float64 reference that rounds Q, K and V to the operand dtype where the
kernels do.  The fused launch issues the ring kernel's MFMA chains (even K tiles, odd K tiles, their sum, the bias) and the attention core's own
tile step, so ctx is asserted BIT-IDENTICAL to the two launches on every case; the bound of 1.5 x the two launches' error against float64 that
the parent kernels would otherwise set is therefore met with ratio 1.  Measured maximum |ctx - float64| per case (fused = two launches):

    dtype  N  S=33      S=40      S=64
    f16    1  5.469e-04 7.814e-04 9.555e-04
    f16    2  8.322e-04 1.010e-03 1.004e-03
    f16    3  8.790e-04 1.285e-03 9.068e-04
    bf16   1  4.860e-03 9.328e-03 4.850e-03
    bf16   2  6.717e-03 4.744e-03 7.105e-03
    bf16   3  7.688e-03 7.897e-03 7.232e-03

Forward level: ``forward_fused`` with the option 1 and 0, folded and K/V-cache cross form, Kv 300.  At N = 32, L = 32 (2048 rows) and N = 27,
L = 8 (1080 rows, a ragged last group) the QKV GEMM of the two-launch path runs its ring tile: query and cls are identical bit for bit, and the
launch counters show no masked attention launch and no QKV ring launch in the fused forward.  At N = 3, L = 8 the two-launch path runs the QKV
GEMM on a two-buffer tile (ONE accumulator chain over K, where the ring tiles and the fused launch add an even and an odd chain); the plan
leaves such forwards on the two launches, so the outputs are identical there too (and inside the oracle bar of tests/test_gpu_parity.py).
S = 65, the pair forward and a forward that returns the full sequence keep the two launches."""
import time

import pytest
import torch

from mraudio_amd import _lib as L
from oracle import qformer_ref as O
from test_gpu_cross_fuse import _desc
from test_gpu_parity import Z_ATOL, build_qformer, oracle_cfg
from test_gpu_qformer_kernels import DEV, DT, Buf, _bits, _ok, _stream
from test_gpu_raw_features import _run
from tools.make_golden import make_inputs

pytestmark = pytest.mark.gpu
H, HEADS = 768, 12


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device(DEV)


# =========================================================================================================================================
# launch level
# =========================================================================================================================================
_CASE = {}


def _case(N, Lt, dt):
    """Seeded inputs rounded to the operand dtype and the float64 ctx, computed once per case."""
    key = (N, Lt, dt)
    if key not in _CASE:
        dtype = DT[dt][0]
        S = 32 + Lt
        g = torch.Generator().manual_seed(1000 * N + 10 * Lt + (dt == "bf16"))
        x = torch.randn(N * S, H, generator=g).to(dtype)                     # LayerNorm outputs: unit scale
        w = (0.04 * torch.randn(3 * H, H, generator=g)).to(dtype)
        b = 0.1 * torch.randn(3 * H, generator=g)
        mask = torch.ones(N, S, dtype=torch.int64)
        for n in range(N):
            mask[n, 32 + max(1, Lt - 3 * n - 1):] = 0                         # padded text tails (none where the text is one token)
        mask[N // 2, 32:] = 0                                                 # one item whose text is fully padded
        qkv = (x.double() @ w.double().T + b.double()).to(dtype).double().view(N, S, 3, HEADS, 64)   # rounded where the kernels round
        q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))        # [N, heads, S, 64]
        s = q @ k.transpose(-1, -2) / 8.0 + ((1 - mask.double()) * -10000.0)[:, None, None, :]
        ref = (torch.softmax(s, dim=-1) @ v).permute(0, 2, 1, 3).reshape(N, S, H)
        _CASE[key] = (x, w, b, mask, ref)
    return _CASE[key]


def _two_launches(x, w, b, mask, N, S, dtype, op):
    """Steps 1 and 2 as run_lanes issues them at the headline shape: the QKV GEMM on the 144 x 128 ring tile, then the attention core."""
    M = N * S
    qkv = Buf(M * 3 * H, dtype)
    ctx = Buf(M * H, dtype)
    nb = lambda t: t.numel * t.inner.element_size()
    d = _desc(A=x.inner.data_ptr(), a_bytes=nb(x), W=w.inner.data_ptr(), w_bytes=nb(w), bias=b.inner.data_ptr(), bias_bytes=nb(b),
              C=qkv.inner.data_ptr(), c_bytes=nb(qkv), a_view=(0, M, H), c_view=(0, M, 3 * H), M=M, N=3 * H, K=H, tile_cfg=L.GT_RING_144x128)
    before = L.gemm_launches(L.GF_RING_144x128, L.EPI_OP)
    _ok(L.lib().mra_debug_gemm(d, 1, L.EPI_OP, op, _stream()), "qkv gemm")
    assert L.gemm_launches(L.GF_RING_144x128, L.EPI_OP) - before == 1
    _ok(L.lib().mra_debug_self_attention(qkv.ptr, mask.ptr, op, N, S, HEADS, ctx.ptr, None, _stream()), "self attention")
    return ctx.result(True, "ctx of the two launches")


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("Lt", [1, 8, 32])
@pytest.mark.parametrize("N", [1, 2, 3])
def test_fused_launch_against_float64_and_the_two_launches(N, Lt, dt, dev):
    t0 = time.time()
    dtype, op = DT[dt]
    S = 32 + Lt
    x_, w_, b_, mask_, ref = _case(N, Lt, dt)
    x, w, b, mask = (Buf(t.numel(), t.dtype, t) for t in (x_, w_, b_, mask_))
    ctx = Buf(N * S * H, dtype)
    before = L.lib().mra_debug_qkv_attention_launches()
    _ok(L.lib().mra_debug_qkv_attention(x.ptr, w.ptr, b.ptr, mask.ptr, op, N, S, HEADS, ctx.ptr, _stream()), "mra_debug_qkv_attention")
    assert L.lib().mra_debug_qkv_attention_launches() - before == 1
    for name, t in (("rows", x), ("wqkv", w), ("bqkv", b), ("mask", mask)):
        t.unchanged(name)
    got = ctx.result(True, "ctx")
    two = _two_launches(x, w, b, mask, N, S, dtype, op)
    e_fused = (got.double().view(N, S, H) - ref).abs().max().item()
    e_two = (two.double().view(N, S, H) - ref).abs().max().item()
    same = torch.equal(_bits(got), _bits(two))
    print(f"fused qkv+attention N {N} S {S} {dt}: max |d| against float64 fused {e_fused:.3e}, two launches {e_two:.3e}, "
          f"bit-identical: {same}  [{time.time() - t0:.1f} s]")
    assert torch.isfinite(got.float()).all()
    assert e_fused <= 1.5 * e_two
    assert same, f"{int((_bits(got) != _bits(two)).sum())} elements differ from the two-launch path"


def test_null_mask_and_null_bias(dev):
    """NULL mask = all ones (the two-launch path then runs the unmasked core), NULL bias = no bias: same bits as the two launches."""
    dtype, op = DT["f16"]
    N, S = 3, 40
    x_, w_, _, _, _ = _case(N, 8, "f16")
    x, w = Buf(x_.numel(), dtype, x_), Buf(w_.numel(), dtype, w_)
    ctx, qkv, ctx2 = Buf(N * S * H, dtype), Buf(N * S * 3 * H, dtype), Buf(N * S * H, dtype)
    _ok(L.lib().mra_debug_qkv_attention(x.ptr, w.ptr, None, None, op, N, S, HEADS, ctx.ptr, _stream()), "mra_debug_qkv_attention")
    nb = lambda t: t.numel * t.inner.element_size()
    d = _desc(A=x.inner.data_ptr(), a_bytes=nb(x), W=w.inner.data_ptr(), w_bytes=nb(w), C=qkv.inner.data_ptr(), c_bytes=nb(qkv),
              a_view=(0, N * S, H), c_view=(0, N * S, 3 * H), M=N * S, N=3 * H, K=H, tile_cfg=L.GT_RING_144x128)
    _ok(L.lib().mra_debug_gemm(d, 1, L.EPI_OP, op, _stream()), "qkv gemm")
    _ok(L.lib().mra_debug_self_attention(qkv.ptr, None, op, N, S, HEADS, ctx2.ptr, None, _stream()), "self attention")
    assert torch.equal(_bits(ctx.result(True, "ctx")), _bits(ctx2.result(True, "ctx of the two launches")))


# =========================================================================================================================================
# forward level
# =========================================================================================================================================
E_SMALL = 704
LAYERS = 4


@pytest.fixture(scope="module")
def small(dev):
    qf, cfg = build_qformer(dev, E_SMALL, seed=11, layers=LAYERS)
    assert (cfg.heads, cfg.n_query, cfg.hidden, cfg.cross_freq) == (12, 32, 768, 2)
    return qf, cfg, O.init_weights(oracle_cfg(cfg), seed=11, perturb=True)


def _counts():
    return (int(L.lib().mra_debug_qkv_attention_launches()), int(L.lib().mra_debug_attention_launches(1)),
            L.gemm_launches(L.GF_RING_144x128, L.EPI_OP))


def _forward(qf, dev, ids, att, x, option):
    qf.set_option("self_fuse", option)
    c0 = _counts()
    _, out = _run(qf, dev, ids, att, x)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items() if v is not None}, [b - a for a, b in zip(c0, _counts())]


@pytest.fixture(scope="module")
def default_option(small):
    """The option value a new handle starts with is restored after every forward test."""
    return 1 if _default_is_on(small[0]) else 0


def _default_is_on(qf):
    ids = torch.randint(1000, 30000, (32, 1))
    att = torch.ones(32, 33, dtype=torch.long)
    c0 = _counts()
    qf.forward_fused(ids.to(DEV), att.to(DEV), torch.zeros(32, 8, E_SMALL, dtype=torch.float16, device=DEV), want_query=True)
    torch.cuda.synchronize()
    return _counts()[0] - c0[0] > 0


@pytest.mark.parametrize("mode", ["fold", "kv_cache"])
@pytest.mark.parametrize("N,Lt", [(32, 32), (27, 8)])
def test_forward_is_identical_and_issues_neither_old_launch(N, Lt, mode, small, default_option, dev):
    """2048 rows of S = 64 (the headline chain) and 1080 rows of S = 40 with a ragged last group."""
    qf, cfg, _ = small
    ids, _, att, feats = make_inputs(oracle_cfg(cfg), N, Lt, 300, 91, True)
    x = feats.half().to(dev)
    qf.set_cross_mode(mode)
    try:
        on, n_on = _forward(qf, dev, ids, att, x, 1)
        off, n_off = _forward(qf, dev, ids, att, x, 0)
    finally:
        qf.set_option("self_fuse", default_option)
        qf.set_cross_mode("auto")
    print(f"{mode} N {N} L {Lt}: launches (fused, masked attention core, QKV ring 144 x 128) on {n_on} off {n_off}")
    assert n_on == [LAYERS, 0, 0] and n_off == [0, LAYERS, LAYERS]
    assert set(on) == {"query", "cls"}
    for k in off:
        assert torch.isfinite(on[k]).all()
        assert torch.equal(_bits(on[k]), _bits(off[k])), f"{k}: the fused launch changed the forward's output"


@pytest.mark.parametrize("mode", ["fold", "kv_cache"])
def test_small_forward_keeps_the_two_launches_and_its_bits(mode, small, default_option, dev):
    """N = 3, L = 8: 120 rows, the QKV GEMM on a two-buffer tile (one accumulator chain over K) -- the plan leaves such a forward alone, so
    the option cannot move it off the pair forward's bits; both runs are held to the oracle bar as well."""
    qf, cfg, w = small
    ocfg = oracle_cfg(cfg)
    ids, _, att, feats = make_inputs(ocfg, 3, 8, 300, 92, True)
    x16 = feats.half()
    qf.set_cross_mode(mode)
    try:
        on, n_on = _forward(qf, dev, ids, att, x16.to(dev), 1)
        off, n_off = _forward(qf, dev, ids, att, x16.to(dev), 0)
    finally:
        qf.set_option("self_fuse", default_option)
        qf.set_cross_mode("auto")
    assert n_on[:2] == [0, LAYERS] and n_off[:2] == [0, LAYERS]
    h = O.qformer_forward(w, ocfg, ids, att, w["query_tokens"].expand(3, -1, -1), O.modality_layernorm(x16.float(), w["ln.weight"], w["ln.bias"]))
    for k in off:
        assert torch.equal(_bits(on[k]), _bits(off[k]))
    e_q = (on["query"] - h[:, :32]).abs().max().item()
    e_c = (on["cls"] - h[:, 32]).abs().max().item()
    print(f"{mode}: query vs oracle {e_q:.3e}, cls vs oracle {e_c:.3e}")
    assert e_q < Z_ATOL and e_c < Z_ATOL


def test_long_prompts_and_the_pair_forward_keep_the_two_launches(small, default_option, dev):
    qf, cfg, _ = small
    qf1, _ = build_qformer(dev, E_SMALL, seed=12, layers=LAYERS)          # the second lane of the pair forward
    ocfg = oracle_cfg(cfg)
    try:
        ids, _, att, feats = make_inputs(ocfg, 16, 33, 40, 93, True)     # S = 65, 1040 rows
        x = feats.half().to(dev)
        on, n_on = _forward(qf, dev, ids, att, x, 1)
        off, n_off = _forward(qf, dev, ids, att, x, 0)
        assert n_on == [0, LAYERS, LAYERS] and n_off == [0, LAYERS, LAYERS]
        for k in off:
            assert torch.equal(_bits(on[k]), _bits(off[k]))
        ids, _, att, feats = make_inputs(ocfg, 16, 32, 40, 94, True)     # two lanes of 1024 rows
        enc = qf.modality_ln(feats.half().to(dev))
        qf.set_option("self_fuse", 1)
        c0 = _counts()
        full = qf.forward_fused(ids.to(dev), att.to(dev), enc, want_query=True, want_full=True)   # the full sequence: the two launches
        torch.cuda.synchronize()
        assert [b - a for a, b in zip(c0, _counts())] == [0, LAYERS, LAYERS]
        c0 = _counts()
        only_q = qf.forward_fused(ids.to(dev), att.to(dev), enc, want_query=True)["query"]
        torch.cuda.synchronize()
        assert [b - a for a, b in zip(c0, _counts())] == [LAYERS, 0, 0]
        assert torch.equal(_bits(only_q.cpu()), _bits(full["query"].cpu()))
        res = {}
        for option in (1, 0):
            qf.set_option("self_fuse", option)
            qf1.set_option("self_fuse", option)
            c0 = _counts()
            pair = type(qf).forward_pair(qf, qf1, ids.to(dev), att.to(dev), enc, enc, want_cls=True)
            torch.cuda.synchronize()
            n = [b - a for a, b in zip(c0, _counts())]
            assert n[:2] == [0, LAYERS], f"the pair forward with the option {option} ran {n}"
            res[option] = [t.cpu() for lane in pair for t in lane]
        for a, b in zip(res[1], res[0]):
            assert torch.equal(_bits(a), _bits(b))
        with pytest.raises(L.MraError):
            qf.set_option("self_fuse", 2)
    finally:
        qf.set_option("self_fuse", default_option)
