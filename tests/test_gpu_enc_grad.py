"""Encoder side of the training step on the GPU (``-m gpu``): the data-gradient GEMM over the head-major dK / dV cache alone
(``mra_debug_kvgrad_gemm``) and the modality LayerNorm backward alone (``mra_modality_ln_backward``) against the float64 references and
derived bounds of tests/enc_grad_cases.py; ``mra_qformer_backward_enc`` + the LayerNorm backward behind autograd against torch.autograd over
the CPU oracle (single and multi-query); that nothing else moved; and the model-level switch ``enable_qformer_training(train_ln=True)``.

Bars of the end-to-end checks: those of tests/test_gpu_backward.py for a gradient tensor (relative Frobenius 2e-2, peak 5e-2 in f16, 8 x in
bf16).  The refusals of the three entries that need a handle are here too (tests/test_enc_grad_cases_cpu.py has the ones that do not)."""
import ctypes as C
import functools

import pytest
import torch

import enc_grad_cases as EG
from oracle import qformer_ref as O
from test_gpu_backward import DTYPES
from test_gpu_multi_query import make_rows

pytestmark = pytest.mark.gpu

GUARD = 4096
MRA_ESTATE, MRA_ENOMEM = -2, -4      # include/mra.h
SENTINEL = -7.25


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _id(v):
    return str(v).replace("torch.", "")


def _bars(op_dtype):
    return next(d[2:] for d in DTYPES if d[0] == op_dtype)


def _handle(dev, E, layers, op_dtype):
    from mraudio_amd.qformer import QFormer, QFormerConfig

    return QFormer(QFormerConfig(enc_width=E, layers=layers, op_dtype=op_dtype), device=dev)


def _loaded(dev, E, layers, op_dtype, seed=0):
    """A Q-Former of ``layers`` layers holding the oracle's seeded weights: (qf, oracle cfg, weights)."""
    qf = _handle(dev, E, layers, op_dtype)
    ocfg = O.QFormerCfg(enc_width=E, layers=layers)
    w = O.init_weights(ocfg, seed=seed, perturb=True)
    qf.load_state_dict({k: v for k, v in w.items() if k.startswith("bert.")})
    for k in ("query_tokens", "ln.weight", "ln.bias"):
        qf.push(k, w[k])
    return qf, ocfg, w


def _stream():
    from mraudio_amd import _lib
    return _lib.current_stream()


def _lib_():
    from mraudio_amd import _lib
    return _lib


# ---- 1. the GEMM alone --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kg_case(layers, Ne, kv, E, dtype):
    dkv, W = EG.make_kvgrad(EG.ncross_of(layers), Ne, kv, E, dtype)
    ref, bound = EG.kvgrad_ref(dkv, W)
    return dkv, W, ref, bound


def _push_kv_weights(qf, W, layers):
    H = EG.HIDDEN
    for cl in range(EG.ncross_of(layers)):
        for sel, name in enumerate(("key", "value")):
            r0 = (cl * 2 + sel) * H
            qf.push(f"bert.encoder.layer.{cl * 2}.crossattention.self.{name}.weight", W[r0: r0 + H])


def run_kvgrad(qf, dkv, Ne, kv, E, dev, dkv_short=0, out_short=0, expect=0):
    """One mra_debug_kvgrad_gemm call: the cache sits between NaN guards (whatever the contraction must not read is NaN), the output
    between sentinel guards.  Returns d_enc [Ne * kv, E] on the CPU."""
    _lib = _lib_()
    n = dkv.numel()
    g16 = GUARD // 2
    cache = torch.full((g16 + n + g16,), float("nan"), dtype=dkv.dtype, device=dev)
    cache[g16: g16 + n] = dkv.reshape(-1).to(dev)
    rows = Ne * kv
    g32 = GUARD // 4
    buf = torch.full((g32 + rows * E + g32,), SENTINEL, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().mra_debug_kvgrad_gemm(qf._handle, C.c_void_p(cache.data_ptr() + GUARD), n * 2 - dkv_short, Ne, kv,
                                              C.c_void_p(buf.data_ptr() + GUARD), rows * E * 4 - out_short, _stream())
    torch.cuda.synchronize(dev)
    assert rc == expect, (rc, _lib.lib().mra_last_error())
    out = buf.cpu()
    assert (out[:g32] == SENTINEL).all() and (out[-g32:] == SENTINEL).all()
    body = out[g32: g32 + rows * E].view(rows, E)
    if rc != 0:
        assert (body == SENTINEL).all()           # refused: nothing written
    return body


@pytest.mark.parametrize("layers", EG.KG_LAYERS)
@pytest.mark.parametrize("E", EG.ENC_WIDTHS)
@pytest.mark.parametrize("dtype", EG.DTYPES, ids=_id)
def test_kvgrad_gemm_against_float64(dtype, E, layers, dev):
    qf = _handle(dev, E, layers, dtype)
    shapes = [(ne, kv) for (lay, ne, kv) in EG.kg_cases() if lay == layers]
    pushed = None
    for Ne, kv in shapes:
        dkv, W, ref, bound = kg_case(layers, Ne, kv, E, dtype)
        if pushed is None or not torch.equal(pushed, W):
            _push_kv_weights(qf, W, layers)
            pushed = W
        got = run_kvgrad(qf, dkv, Ne, kv, E, dev)
        assert (got != SENTINEL).all() and torch.isfinite(got).all()
        r = EG.ratio(got, ref, bound)
        print(f"kvgrad layers {layers} ({Ne}, {kv}) E {E} {_id(dtype)}: ratio {r:.3g}")
        assert r <= 1.0, (layers, Ne, kv, E, dtype, r)


def test_kvgrad_gemm_refusals_that_need_a_handle(dev):
    _lib = _lib_()
    qf = _handle(dev, 768, 2, torch.float16)
    dkv, W, _, _ = kg_case(2, 3, 40, 768, torch.float16)
    _push_kv_weights(qf, W, 2)
    run_kvgrad(qf, dkv, 3, 40, 768, dev, dkv_short=1, expect=-1)
    assert b"dkv_bytes" in _lib.lib().mra_last_error()
    run_kvgrad(qf, dkv, 3, 40, 768, dev, out_short=1, expect=-1)
    assert b"d_enc_bytes" in _lib.lib().mra_last_error()
    with torch.cuda.device(dev):
        assert _lib.lib().mra_debug_kvgrad_gemm(qf._handle, None, 0, 0, 40, None, 0, _stream()) == 0      # enc_items == 0: a no-op
        # mra_qformer_backward_enc: training not enabled, then a workspace one byte too small
        ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
        out = torch.zeros(3 * 40 * 768, dtype=torch.float32, device=dev)
        L = _lib.lib()
        assert L.mra_qformer_backward_enc(qf._handle, 3, 1, 5, 40, _lib.ptr(ws), ws.numel(), _lib.ptr(out), _stream()) == MRA_ESTATE
        assert b"enable_training" in L.mra_last_error()
        assert L.mra_qformer_backward_enc(qf._handle, 0, 1, 5, 40, None, 0, None, _stream()) == 0             # enc_items == 0: a no-op
    qf2, _, _ = _loaded(dev, 768, 2, torch.float16)
    qf2.enable_training()
    with torch.cuda.device(dev):
        need = int(L.mra_qformer_multi_train_workspace_bytes(qf2._handle, 3, 2, 5, 40))
        assert need > 0
        big = torch.zeros(need, dtype=torch.uint8, device=dev)
        rc = L.mra_qformer_backward_enc(qf2._handle, 3, 2, 5, 40, _lib.ptr(big), need - 1, _lib.ptr(out), _stream())
        assert rc == MRA_ENOMEM and b"workspace too small" in L.mra_last_error()
        # mra_modality_ln_backward on a handle whose ln.* was never loaded
        x = torch.zeros(2, 3, 768, dtype=torch.float32, device=dev)
        rc = L.mra_modality_ln_backward(qf._handle, _lib.ptr(x), _lib.MRA_F32, 2, 3, _lib.ptr(x), None, None, None, _stream())
        assert rc == MRA_ESTATE and b"not loaded" in L.mra_last_error()
    torch.cuda.synchronize(dev)
    assert float(out.abs().max()) == 0.0


# ---- 2. the LayerNorm backward alone -------------------------------------------------------------------------------------------------------
X_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


@functools.lru_cache(maxsize=None)
def mln_case(rows, E, x_dtype):
    c = EG.make_mln(rows, E, x_dtype)
    return c, EG.mln_ref(c["x"], c["d_out"], c["gain"], c["dgain0"], c["dbias0"]), EG.mln_ref(c["x"], c["d_out"], c["gain"])


@functools.lru_cache(maxsize=None)
def ln_handle(E):
    return _handle(torch.device("cuda:0"), E, 2, torch.float16)


def run_mln(qf, c, dev, want_x, want_g, want_b, inplace, prefill, items=None):
    """One mra_modality_ln_backward call; outputs between sentinel guards.  Returns (d_x, d_gain, d_bias, d_out after) on the CPU, None
    for what was not asked for."""
    _lib = _lib_()
    rows, E = c["x"].shape
    items = items or 1
    g32 = GUARD // 4
    x = c["x"].to(dev).contiguous()
    dout_buf = torch.full((g32 + rows * E + g32,), SENTINEL, dtype=torch.float32, device=dev)
    dout_buf[g32: g32 + rows * E] = c["d_out"].reshape(-1).to(dev)
    dx_buf = torch.full((g32 + rows * E + g32,), SENTINEL, dtype=torch.float32, device=dev)
    vec = lambda t0: torch.cat([torch.full((g32,), SENTINEL), t0 if prefill else torch.zeros(E), torch.full((g32,), SENTINEL)]).to(dev)   # noqa: E731
    dg_buf, db_buf = vec(c["dgain0"]), vec(c["dbias0"])
    p = lambda b: C.c_void_p(b.data_ptr() + GUARD)   # noqa: E731
    dx_ptr = None if not want_x else (p(dout_buf) if inplace else p(dx_buf))
    with torch.cuda.device(dev):
        rc = _lib.lib().mra_modality_ln_backward(qf._handle, _lib.ptr(x), _lib.mra_dtype(x.dtype), items, rows // items, p(dout_buf), dx_ptr,
                                                 p(dg_buf) if want_g else None, p(db_buf) if want_b else None, _stream())
    torch.cuda.synchronize(dev)
    assert rc == 0, _lib.lib().mra_last_error()
    outs = []
    for b in (dout_buf, dx_buf, dg_buf, db_buf):
        h = b.cpu()
        assert (h[:g32] == SENTINEL).all() and (h[-g32:] == SENTINEL).all()
        outs.append(h[g32:-g32])
    dout_after, dx_sep, dg, db = outs
    if not (want_x and not inplace):
        assert (dx_sep == SENTINEL).all()
    if not (want_x and inplace):
        assert torch.equal(dout_after.view(rows, E), c["d_out"])           # d_out is only read
    if not want_g:
        assert torch.equal(dg, c["dgain0"] if prefill else torch.zeros(E))
    if not want_b:
        assert torch.equal(db, c["dbias0"] if prefill else torch.zeros(E))
    dx = None if not want_x else (dout_after if inplace else dx_sep).view(rows, E)
    return dx, (dg if want_g else None), (db if want_b else None)


@pytest.mark.parametrize("x_dtype", X_DTYPES, ids=_id)
@pytest.mark.parametrize("E", EG.ENC_WIDTHS)
def test_modality_ln_backward_against_float64(E, x_dtype, dev):
    qf = ln_handle(E)
    for rows in EG.LN_ROWS:
        c, ref_pre, ref_zero = mln_case(rows, E, x_dtype)
        qf.push("ln.weight", c["gain"])
        qf.push("ln.bias", torch.zeros(E))
        combos = [(wx, wg, wb) for wx in (True, False) for wg in (True, False) for wb in (True, False)]
        for wx, wg, wb in combos:
            for inplace in ((False, True) if wx else (False,)):
                for prefill in ((True, False) if (wx and wg and wb) else (True,)):
                    dx_ref, dx_b, dg_ref, dg_b, db_ref, db_b = ref_pre if prefill else ref_zero
                    items = 4 if rows == 64 else 1
                    dx, dg, db = run_mln(qf, c, dev, wx, wg, wb, inplace, prefill, items)
                    rs = (EG.ratio(dx, dx_ref, dx_b) if wx else 0.0, EG.ratio(dg, dg_ref, dg_b) if wg else 0.0, EG.ratio(db, db_ref, db_b) if wb else 0.0)
                    if wx and wg and wb:
                        print(f"mln rows {rows} E {E} {_id(x_dtype)} inplace {inplace} prefill {prefill}: d_x {rs[0]:.3f} d_gain {rs[1]:.3f} d_bias {rs[2]:.3f}")
                    assert max(rs) <= 1.0, (rows, E, x_dtype, (wx, wg, wb), inplace, prefill, rs)


# ---- 3. end to end against torch.autograd over the oracle -----------------------------------------------------------------------------------
def _errors(got, ref):
    return ((got - ref).norm() / ref.norm()).item(), ((got - ref).abs().max() / ref.abs().max()).item()


@functools.lru_cache(maxsize=None)
def oracle_e2e(E, op_dtype, P):
    """Oracle autograd of the loss of test_forward_backward_matches_oracle_autograd through LayerNorm -> cast -> Q-Former (4 layers, 3
    items, L = 5, kv = 40; chain row i * P + p reads item i): inputs and the gradients of feats, ln.weight, ln.bias, computed once."""
    n, L, kv = 3, 5, 40
    ocfg = O.QFormerCfg(enc_width=E, layers=4)
    w = O.init_weights(ocfg, seed=0, perturb=True)
    N = n * P
    ids, att = make_rows(ocfg, N, L, 77)
    feats = torch.randn(n, kv, E, generator=torch.Generator().manual_seed(78)).requires_grad_(True)
    g, b = w["ln.weight"].clone().requires_grad_(True), w["ln.bias"].clone().requires_grad_(True)
    gen = torch.Generator().manual_seed(5)
    rq, rc = torch.randn(N, 32, 768, generator=gen), torch.randn(N, 768, generator=gen)
    enc = O.modality_layernorm(feats, g, b).to(op_dtype).float()
    h = O.qformer_forward(w, ocfg, ids, att, w["query_tokens"].expand(N, -1, -1), enc.repeat_interleave(P, 0) if P > 1 else enc)
    ((h[:, :32] * rq).sum() + (h[:, 32] * rc).sum()).backward()
    return dict(ids=ids, att=att, feats=feats.detach(), rq=rq, rc=rc, d_feats=feats.grad, d_g=g.grad, d_b=b.grad, q=h[:, :32].detach())


def gpu_e2e(qf, w, case, P, dev, want_x=True):
    """The HIP path of the same graph: returns (d_feats or None, d ln.weight, d ln.bias, q)."""
    x = case["feats"].to(dev).requires_grad_(want_x)
    g, b = w["ln.weight"].to(dev).requires_grad_(True), w["ln.bias"].to(dev).requires_grad_(True)
    qf.push("ln.weight", g)
    qf.push("ln.bias", b)
    enc = qf.modality_ln_train(x, g, b)
    ids, att = case["ids"].to(dev), case["att"].to(dev)
    q, c = qf.forward_multi_train(ids, att, enc, P) if P > 1 else qf.forward_train(ids, att, enc)
    ((q * case["rq"].to(dev)).sum() + (c * case["rc"].to(dev)).sum()).backward()
    torch.cuda.synchronize(dev)
    return (x.grad.cpu() if want_x else None), g.grad.cpu(), b.grad.cpu(), q.detach().cpu()


@pytest.mark.parametrize("P", (1, 3), ids=("single", "multi3"))
@pytest.mark.parametrize("E", EG.ENC_WIDTHS)
@pytest.mark.parametrize("op_dtype", EG.DTYPES, ids=_id)
def test_encoder_side_gradients_match_oracle_autograd(op_dtype, E, P, dev):
    rel_tol, peak_tol = _bars(op_dtype)
    case = oracle_e2e(E, op_dtype, P)
    qf, ocfg, w = _loaded(dev, E, 4, op_dtype)
    d_x, d_g, d_b, q = gpu_e2e(qf, w, case, P, dev)
    assert (q - case["q"]).abs().max().item() < (1e-2 if op_dtype == torch.float16 else 8e-2)
    for name, got, ref in (("d_feats", d_x, case["d_feats"]), ("d ln.weight", d_g, case["d_g"]), ("d ln.bias", d_b, case["d_b"])):
        assert ref.abs().max().item() > 0 and torch.isfinite(got).all()
        rel, peak = _errors(got.float(), ref)
        print(f"{name} E {E} {_id(op_dtype)} P {P}: relative Frobenius {rel:.3e} peak {peak:.3e}")
        assert rel < rel_tol and peak < peak_tol, (name, rel, peak)
    # the LayerNorm-only case: no d_x asked for, the same parameter gradients
    qf._grad_flat.zero_()
    _, d_g2, d_b2, _ = gpu_e2e(qf, w, case, P, dev, want_x=False)
    assert _errors(d_g2, d_g)[0] < 1e-5 and _errors(d_b2, d_b)[0] < 1e-5


def test_modality_ln_train_refuses_tensors_that_were_not_pushed(dev):
    from mraudio_amd._lib import MraError

    qf, ocfg, w = _loaded(dev, 768, 2, torch.float16)
    x = torch.randn(2, 8, 768, device=dev)
    g, b = w["ln.weight"].to(dev).requires_grad_(True), w["ln.bias"].to(dev).requires_grad_(True)
    with pytest.raises(MraError, match="not the tensor last pushed"):
        qf.modality_ln_train(x, g, b)
    qf.push("ln.weight", g)
    qf.push("ln.bias", b)
    assert torch.equal(qf.modality_ln_train(x, g, b), qf.modality_ln(x))          # the same bits as the inference entry
    with torch.no_grad():
        g.mul_(1.5)
    with pytest.raises(MraError, match="changed since it was pushed"):
        qf.modality_ln_train(x, g, b)


# ---- 4. nothing else moved ---------------------------------------------------------------------------------------------------------------
# Two runs of the SAME step do not give the same bits everywhere, with or without this feature: the LayerNorm, embedding and query-token
# gradients are summed by float atomics from several workgroups, in an order that is not fixed (measured on the parent's code path itself:
# two default steps differ by a few ulp there; tests/test_gpu_multi_train.py compares such buffers with allclose for the same reason).  So:
#   * inside ONE backward, the new launch must leave the flat gradient buffer, the outputs and the tape bit for bit as they were;
#   * across runs, the outputs and every gradient with a fixed summation order -- the dense / query / key / value weights and biases, written
#     by one workgroup each while the weight-gradient GEMM does not split its contraction (under 256 contraction rows: the shapes below) --
#     are bit-identical, and the atomically summed rest agrees to the project's bar for two runs of one step (rtol 1e-3, atol 1e-5).
def _fixed_order(name):
    return name != "query_tokens" and "LayerNorm" not in name and "embeddings" not in name


def _assert_same_step(qf, a, b, what):
    names = [k for k in qf.bert.state_dict(prefix="bert.")] + ["query_tokens"]
    rest = torch.ones(a.numel(), dtype=torch.bool, device=a.device)       # the slots no backward writes (ln.*, llm_proj.*)
    for k in names:
        off, numel = qf._slice_of(k)
        x, y = a[off: off + numel], b[off: off + numel]
        rest[off: off + numel] = False
        if _fixed_order(k):
            assert torch.equal(x, y), (what, k, (x - y).abs().max().item())
        else:
            assert torch.allclose(x, y, rtol=1e-3, atol=1e-5), (what, k, (x - y).abs().max().item())
    assert torch.equal(a[rest], b[rest]) and float(a[rest].abs().max()) == 0.0


@pytest.mark.parametrize("P", (0, 3), ids=("single", "multi3"))
def test_requesting_the_encoder_gradient_changes_nothing_else(P, dev):
    qf, ocfg, w = _loaded(dev, 1408, 4, torch.float16)
    n, L, kv = (2 if P else 3), 5, 40                   # at most 222 chain rows: no weight gradient splits its contraction
    N = n * max(P, 1)
    ids, att = make_rows(ocfg, N, L, 77)
    ids, att = ids.to(dev), att.to(dev)
    enc0 = O.modality_layernorm(torch.randn(n, kv, 1408, generator=torch.Generator().manual_seed(78)), w["ln.weight"], w["ln.bias"]).half().to(dev)
    gen = torch.Generator().manual_seed(5)
    rq, rc = torch.randn(N, 32, 768, generator=gen).to(dev), torch.randn(N, 768, generator=gen).to(dev)
    qf.enable_training()

    def step(want):
        qf._grad_flat.zero_()
        enc = enc0.clone().requires_grad_(want)
        q, c = qf.forward_multi_train(ids, att, enc, P) if P else qf.forward_train(ids, att, enc)
        node = q.grad_fn
        ((q * rq).sum() + (c * rc).sum()).backward()
        torch.cuda.synchronize(dev)
        assert (enc.grad is not None) == want
        return q.detach().clone(), c.detach().clone(), qf._grad_flat.clone(), enc.grad, node

    q0, c0, g0, _, _ = step(False)
    q1, c1, g1, d_enc, _ = step(True)
    assert d_enc.dtype == enc0.dtype and torch.isfinite(d_enc).all() and d_enc.abs().max().item() > 0
    assert g0.abs().max().item() > 0
    assert torch.equal(q0, q1) and torch.equal(c0, c1)
    _assert_same_step(qf, g0, g1, "with against without the encoder gradient")
    # inside one backward: the tape of a step WITHOUT the request, then the new launch alone on it
    q2, c2, g2, _, node = step(False)
    assert node.ws is None
    ws = qf._train_ws                                   # the node hands its tape back to the owner after its backward
    tape = ws.clone()
    again = qf._enc_grad(enc0, n, L, kv, max(P, 1), ws)
    torch.cuda.synchronize(dev)
    assert torch.equal(qf._grad_flat, g2) and torch.equal(ws, tape)
    assert torch.equal(again, d_enc)                    # the data-gradient chain has a fixed order: the same bits as the autograd run


def _small_batch(T=3, kv_v=40, kv_a=24, seed=2):
    g = torch.Generator().manual_seed(seed)
    return {"video_embeds": torch.randn(1, T, kv_v, 1408, generator=g), "audio_embeds": torch.randn(1, T, kv_a, 768, generator=g),
            "text_input": ["Query: a person opens the door.\nRelevant windows: "], "text_output": ["[[2, 4]]"],
            "timestamps": [list(range(0, 2 * T, 2))], "duration": [2 * T]}


def test_train_ln_false_is_the_default_step(dev):
    """``enable_qformer_training()`` and ``enable_qformer_training(train_ln=False)``: the same loss bit for bit, the same gradient buffers
    (bit for bit where two runs of one step can be, see above), no LayerNorm gradient and no further optimizer parameter."""
    from mraudio_amd.models.xinstructblip import XInstructBLIP

    res = []
    for kw in ({}, {"train_ln": False}):
        model = XInstructBLIP(seed=3, perturb=True, device=dev)
        model.enable_qformer_training(**kw)
        loss = model(_small_batch())["loss"]
        loss.backward()
        torch.cuda.synchronize(dev)
        for m in model.modalities:
            assert getattr(model, f"{m}_ln").weight.grad is None and getattr(model, f"{m}_ln").bias.grad is None
            assert not getattr(model, f"{m}_ln").weight.requires_grad
        assert len(model.flat_optimizer_params()) == len(model.modalities)
        res.append((loss.detach().clone(), model))
    assert torch.equal(res[0][0], res[1][0])
    for m in res[0][1].modalities:
        qa, qb = getattr(res[0][1], f"{m}_Qformer"), getattr(res[1][1], f"{m}_Qformer")
        assert qa._grad_flat.abs().max().item() > 0
        _assert_same_step(qa, qa._grad_flat, qb._grad_flat, f"{m}: default against train_ln=False")


# ---- 5. consistency inside one backward ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op_dtype", EG.DTYPES, ids=_id)
def test_ln_bias_gradient_is_the_kv_bias_gradients_through_the_weights(op_dtype, dev):
    """sum_rows d_enc = sum_k W_kv[k][.] db_kv[k]: both sides come out of the same dK / dV cache of one backward."""
    rel_tol, peak_tol = _bars(op_dtype)
    E = 1408
    case = oracle_e2e(E, op_dtype, 1)
    qf, ocfg, w = _loaded(dev, E, 4, op_dtype)
    qf.enable_training()
    qf._grad_flat.zero_()
    _, _, d_b, _ = gpu_e2e(qf, w, case, 1, dev, want_x=False)
    want = torch.zeros(E, dtype=torch.float64)
    for layer in (0, 2):
        for name in ("key", "value"):
            p = f"bert.encoder.layer.{layer}.crossattention.self.{name}."
            want += qf.grad_of(p + "bias").cpu().double() @ w[p + "weight"].to(op_dtype).double()
    rel, peak = _errors(d_b.double(), want)
    print(f"d ln.bias against W_kv^T db_kv, {_id(op_dtype)}: relative Frobenius {rel:.3e} peak {peak:.3e}")
    assert want.abs().max().item() > 0 and rel < rel_tol and peak < peak_tol, (rel, peak)


# ---- 6. no stale weight copy ---------------------------------------------------------------------------------------------------------------
def test_d_enc_follows_every_route_that_changes_weights(dev):
    E, layers = 768, 4
    n, L, kv = 3, 5, 40
    qf, ocfg, w = _loaded(dev, E, layers, torch.float16)
    ids, att = make_rows(ocfg, n, L, 77)
    enc0 = O.modality_layernorm(torch.randn(n, kv, E, generator=torch.Generator().manual_seed(78)), w["ln.weight"], w["ln.bias"]).half().to(dev)
    gen = torch.Generator().manual_seed(5)
    rq, rc = torch.randn(n, 32, 768, generator=gen).to(dev), torch.randn(n, 768, generator=gen).to(dev)

    def d_enc_of(q_former):
        enc = enc0.clone().requires_grad_(True)
        q, c = q_former.forward_train(ids.to(dev), att.to(dev), enc)
        ((q * rq).sum() + (c * rc).sum()).backward()
        torch.cuda.synchronize(dev)
        return enc.grad.clone()

    def fresh_like(q_former, extra=None):
        """A new handle loaded with the CURRENT master values of ``q_former`` (and ``extra`` pushes on top)."""
        other = _handle(dev, E, layers, torch.float16)
        other.load_state_dict({k: v.detach().clone() for k, v in q_former.state_dict().items()})
        off, numel = q_former._slice_of("query_tokens")
        other.push("query_tokens", q_former._master_flat[off: off + numel].view(1, 32, 768).clone())
        for k in ("ln.weight", "ln.bias"):
            other.push(k, w[k])
        for k, v in (extra or {}).items():
            other.sync_weights()
            other.push(k, v)
        return other

    qf.enable_training()
    off, numel = qf._slice_of("query_tokens")
    with torch.no_grad():
        qf._master_flat[off: off + numel].copy_(w["query_tokens"].reshape(-1).to(dev))
    qf._dirty = True
    first = d_enc_of(qf)
    assert first.abs().max().item() > 0
    # (a) the fused optimizer pass
    qf.adam_step(1e-3, zero_grad=True)
    after_adam = d_enc_of(qf)
    assert not torch.equal(after_adam, first)
    assert torch.equal(after_adam, d_enc_of(fresh_like(qf)))
    # (b) load_flat: the master buffer edited in place, uploaded by sync_weights
    key = "bert.encoder.layer.2.crossattention.self.value.weight"
    with torch.no_grad():
        dict(qf.named_parameters())[key].mul_(1.25)
    qf._dirty = True
    after_flat = d_enc_of(qf)
    assert not torch.equal(after_flat, after_adam)
    assert torch.equal(after_flat, d_enc_of(fresh_like(qf)))
    # (c) a push of one cross key weight past the master buffer
    kname = "bert.encoder.layer.0.crossattention.self.key.weight"
    new_k = (w[kname] * 0.5).to(dev)
    qf.sync_weights()
    qf.push(kname, new_k)
    after_push = d_enc_of(qf)
    assert not torch.equal(after_push, after_flat)
    assert torch.equal(after_push, d_enc_of(fresh_like(qf, {kname: new_k})))


# ---- 7. model level ------------------------------------------------------------------------------------------------------------------------
def _finetune_batch():
    g = torch.Generator().manual_seed(2)
    return {"video_embeds": torch.randn(1, 20, 257, 1408, generator=g), "audio_embeds": torch.randn(1, 20, 256, 768, generator=g),
            "text_input": ["Query: a person opens the door.\nGiven the video and the query, find the relevant windows.\nRelevant windows: "],
            "text_output": ["[[6, 12]]"], "timestamps": [list(range(0, 40, 2))], "duration": [40]}


# The BCE loss of this batch gives the 16-bit tensors of the backward tape (dK / dV among them) gradients of order 1e-6 (oracle autograd:
# |d_enc| <= 7.6e-6, median 9.6e-7 on the audio side): below f16's smallest normal 6.1e-5, where the format keeps 3 - 7 bits instead of 11
# and the f16 bars above do not describe it -- measured unscaled on an MI355X: {m}_ln.weight off by 4.4e-2 (audio), the same chain.  f16
# training scales its loss for this reason (the reference steps through a GradScaler): the f16 case backs 2^12 x loss and unscales, bf16
# (the trainer's operand dtype, with fp32's exponent range) runs unscaled.
MODEL_CASES = [(torch.float16, 4096.0), (torch.bfloat16, 1.0)]


def text_ids(model, samples):
    text = model.tokenizer(samples["text_input"], padding="longest", truncation=True, max_length=128, return_tensors="pt")
    return tuple(text.input_ids[0].tolist()), tuple(text.attention_mask[0].tolist())


@functools.lru_cache(maxsize=None)
def _oracle_ln_grads(text_input, ids_mask):
    """Oracle autograd of the BCE loss of ``_finetune_batch`` with respect to the LayerNorm parameters of both modalities, computed once:
    (loss, {modality: {"ln.weight": grad, "ln.bias": grad}})."""
    import os

    from mraudio_amd.models.xinstructblip import ENC_WIDTH

    samples, T = _finetune_batch(), 20
    ids, tm = torch.tensor(ids_mask[0]).repeat(T, 1), torch.tensor(ids_mask[1]).repeat(T, 1)
    cfgs = {m: O.QFormerCfg(enc_width=ENC_WIDTH[m]) for m in ("video", "audio")}
    ws = {"video": O.init_weights(cfgs["video"], seed=3, perturb=True), "audio": O.init_weights(cfgs["audio"], seed=4, perturb=True)}
    for m in ws:
        for k in ("ln.weight", "ln.bias"):
            ws[m][k] = ws[m][k].clone().requires_grad_(True)
    torch.set_num_threads(max(1, min(32, len(os.sched_getaffinity(0)))))
    ref = O.encode_fuse_score(ws, cfgs, {m: samples[f"{m}_embeds"][0] for m in ("audio", "video")}, ids, tm, 1, T)
    ts = torch.tensor(samples["timestamps"][0], dtype=torch.float32)
    want = torch.nn.functional.binary_cross_entropy_with_logits(ref["fused"] * 20.0, ((ts >= 6) & (ts <= 12)).float())
    want.backward()
    return want.detach(), {m: {k: ws[m][k].grad for k in ("ln.weight", "ln.bias")} for m in ws}


@pytest.mark.parametrize("op_dtype,loss_scale", MODEL_CASES, ids=("f16-scaled", "bf16"))
def test_model_level_layernorm_training(op_dtype, loss_scale, dev):
    from mraudio_amd.models.xinstructblip import XInstructBLIP

    rel_tol, peak_tol = _bars(op_dtype)
    samples = _finetune_batch()
    T = 20
    model = XInstructBLIP(seed=3, perturb=True, device=dev, op_dtype=op_dtype)
    model.enable_qformer_training(train_ln=True)
    lns = {m: getattr(model, f"{m}_ln") for m in model.modalities}
    params = model.flat_optimizer_params()
    assert len(params) == len(model.modalities) + 2 * len(model.modalities)
    assert {id(p) for p in params[len(model.modalities):]} == {id(p) for ln in lns.values() for p in ln.parameters()}
    loss = model(samples)["loss"]
    (loss * loss_scale).backward()
    torch.cuda.synchronize(dev)
    want, ref_grads = _oracle_ln_grads(tuple(samples["text_input"]), tuple(text_ids(model, samples)))
    assert abs(loss.item() - want.item()) <= (1e-3 if op_dtype == torch.float16 else 8e-3) * max(1.0, abs(want.item()))
    for m, ln in lns.items():
        for k, p in (("ln.weight", ln.weight), ("ln.bias", ln.bias)):
            assert p.grad is not None and p.grad.abs().max().item() > 0
            rel, peak = _errors(p.grad.cpu().float() / loss_scale, ref_grads[m][k])
            print(f"{m}_{k} {_id(op_dtype)}: relative Frobenius {rel:.3e} peak {peak:.3e}")
            assert rel < rel_tol and peak < peak_tol, (m, k, rel, peak)
    # one optimizer step: the next forward runs on the updated LayerNorm
    old_ln = {k: v.detach().clone() for k, v in model.state_dict().items() if "_ln." in k}
    for p in params:
        p.grad.div_(loss_scale)
    opt = torch.optim.Adam(params, lr=1e-3, fused=True)
    opt.step()
    opt.zero_grad(set_to_none=True)
    with torch.no_grad():
        after = model(samples)["loss"].item()
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert any((sd[k] - old_ln[k]).abs().max().item() > 0 for k in old_ln)

    other = XInstructBLIP(seed=3, perturb=True, device=dev, op_dtype=op_dtype)
    other.enable_qformer_training(train_ln=True)

    def loss_of(state):
        other.load_state_dict(state)
        with torch.no_grad():
            return other(samples)["loss"].item()

    fresh = loss_of(sd)
    assert abs(after - fresh) < 1e-6, (after, fresh)
    stale = loss_of({**sd, **old_ln})                          # the same Q-Formers behind the LayerNorm of before the step
    assert abs(after - stale) > 1e-6, (after, stale)


@pytest.mark.parametrize("train_ln", (True, False))
def test_trainer_checkpoints_carry_the_layernorm_only_when_it_trains(train_ln, dev, tmp_path):
    from mraudio_amd.models.xinstructblip import XInstructBLIP
    from mraudio_amd.utils.mr_dataset import SyntheticMRDataset
    from mraudio_amd.utils.trainer import Trainer, default_args

    args = default_args(output_dir=str(tmp_path), gpu=0, max_epoch=1, warmup_steps=2, lr=1e-5)
    data = SyntheticMRDataset(2, T=4, seed=0, signal=1.0)
    kw = {"train_ln": True} if train_ln else {}
    tr = Trainer(args, model=XInstructBLIP(seed=3, perturb=True, device=dev), train_dataset=data, val_dataset=data, **kw)
    if train_ln:
        before = tr.model.video_ln.weight.detach().clone()
        tr.train_epoch(0)
        assert not torch.equal(before, tr.model.video_ln.weight.detach())
    path = tr._save_checkpoint(0)
    state = torch.load(path, map_location="cpu", weights_only=True)["model"]
    for m in tr.model.modalities:
        for k in ("weight", "bias"):
            assert (f"{m}_ln.{k}" in state) == train_ln
    assert any(k.startswith("video_Qformer.bert.") for k in state)
