"""The backward of the LM's causal grouped-query attention on the GPU (``-m gpu``): ``mra_prefill_attention_backward`` on every element of
dQ, dK and dV against float64 under the DERIVED bounds of tests/prefill_bwd_cases.py -- q / dq as transposed views, K / V as views of a longer,
poisoned buffer, the dO / out rows of query rows that attend nothing poisoned, padded output strides with sentinels between rows and heads,
guards around the three outputs and the workspace, two runs bit for bit -- the forward entry chained into it, every attention backward of a
real training step of the tiny Llamas of tests/test_gpu_lm_step.py, and ``XInstructBLIP(lm_attention="hip")`` against ``"stock"``."""
import pytest
import torch

import prefill_attn_cases as PC
import prefill_bwd_cases as BC
from mraudio_amd import _lib
from mraudio_amd.models import lm_attention as LA
from mraudio_amd.models import lm_decode as LD

pytestmark = pytest.mark.gpu

GUARD = 64                       # elements on either side of every output (a multiple of 8: the views stay 16-byte aligned)
SENT = float("nan")               # NaN sentinels: an element the entry leaves unwritten also fails the comparison against float64
CASES = BC.cases()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _id(dt):
    return "f16" if dt == torch.float16 else "bf16"


def _guarded(dev, dtype, B, H, S, D, s_pad, transposed):
    """A [B, H, S, D] output view inside a sentinel-filled buffer with padded strides: ``transposed`` = the transposed view of a
    [B, S, H, D + pad] tensor (position stride H (D + pad) + s_pad), else [B, H, S, D + pad] rows with s_pad spare rows per head.
    (buffer, view)."""
    pad = 8 * (1 + H % 3)
    if transposed:
        ss = H * (D + pad) + 8 * s_pad
        buf = torch.full((2 * GUARD + B * S * ss,), SENT, dtype=dtype, device=dev)
        body = buf[GUARD: GUARD + B * S * ss].view(B, S, ss)
        view = body[:, :, :H * (D + pad)].view(B, S, H, D + pad)[..., :D].transpose(1, 2)
    else:
        rows = S + s_pad
        buf = torch.full((2 * GUARD + B * H * rows * (D + pad),), SENT, dtype=dtype, device=dev)
        view = buf[GUARD: GUARD + B * H * rows * (D + pad)].view(B, H, rows, D + pad)[:, :, :S, :D]
    return buf, view


def _sentinels_kept(buf, view) -> bool:
    """Everything of ``buf`` outside ``view`` still holds the sentinel."""
    keep = view.clone()
    view.fill_(SENT)
    ok = bool(torch.isnan(buf).all())
    view.copy_(keep)
    return ok


def _operands(dev, case, dtype):
    """The forward test's operands (q transposed, K / V in a longer poisoned buffer, mask bytes) plus dout / out as padded [B, Sq, Hq, D]
    views with the rows of query rows that attend nothing poisoned, and lse."""
    B, Hq, Hkv, Sq, Skv, off, D, _ = case
    c, lay = BC.make_case(*case, dtype), PC.layout(Hq, Sq, Skv, D)
    q = c["q"].to(dev).transpose(1, 2).contiguous().transpose(1, 2)
    kbuf = torch.full((B, Hkv, lay["Smax"], lay["k_ss"]), float("nan"), dtype=dtype, device=dev)
    vbuf = torch.full((B, Hkv, lay["Smax"], lay["v_ss"]), float("-inf"), dtype=dtype, device=dev)
    k, v = kbuf[:, :, :Skv, :D], vbuf[:, :, :Skv, :D]
    k.copy_(c["k"])
    v.copy_(c["v"])
    mask, m_sb = None, 0
    if c["mask"] is not None:
        m_sb = Skv + 3
        mask = torch.ones(B, m_sb, dtype=torch.uint8, device=dev)
        mask[:, :Skv] = c["mask"].to(dev).to(torch.uint8) * (1 + 6 * (Skv % 2))
    dead = ~(c["lse"] > float("-inf")).transpose(1, 2)[..., None].expand(B, Sq, Hq, D)      # [B, Sq, Hq, D]
    dout_c, out_c = c["dout"].clone(), c["out"].clone()
    PC._poison(dout_c, dead)
    PC._poison(out_c, dead)
    o_sh = lay["o_sh"]
    dout = torch.zeros(B, Sq, Hq, o_sh + 8, dtype=dtype, device=dev)[..., :D]
    out = torch.zeros(B, Sq, Hq, o_sh, dtype=dtype, device=dev)[..., :D]
    dout.copy_(dout_c)
    out.copy_(out_c)
    return c, q, k, v, mask, m_sb, dout, out, c["lse"].to(dev)


def _call(case, dtype, c, q, k, v, mask, m_sb, dout, out, lse, dq, dk, dv, ws, ws_bytes):
    B, Hq, Hkv, Sq, Skv, off, D, _ = case
    return _lib.lib().mra_prefill_attention_backward(
        _lib.ptr(q), q.stride(0), q.stride(1), q.stride(2), _lib.ptr(k), k.stride(0), k.stride(1), k.stride(2), _lib.ptr(v), v.stride(0), v.stride(1),
        v.stride(2), None if mask is None else _lib.ptr(mask), m_sb, _lib.ptr(out), out.stride(0), out.stride(1), out.stride(2), _lib.ptr(dout),
        dout.stride(0), dout.stride(1), dout.stride(2), _lib.ptr(lse), B, Hq, Hkv, Sq, Skv, off, D, _lib.mra_dtype(dtype), c["scale"], _lib.ptr(dq),
        dq.stride(0), dq.stride(1), dq.stride(2), _lib.ptr(dk), dk.stride(0), dk.stride(1), dk.stride(2), _lib.ptr(dv), dv.stride(0), dv.stride(1),
        dv.stride(2), _lib.ptr(ws), ws_bytes, _lib.current_stream())


def _run(dev, case, dtype, ops=None):
    """One call of the entry on guarded, strided buffers: (dq [B, Hq, Sq, D], dk, dv [B, Hkv, Skv, D]) after the guard checks."""
    B, Hq, Hkv, Sq, Skv, off, D, _ = case
    c, q, k, v, mask, m_sb, dout, out, lse = ops if ops is not None else _operands(dev, case, dtype)
    qbuf, dq = _guarded(dev, dtype, B, Hq, Sq, D, Sq % 2, True)
    kbuf, dk = _guarded(dev, dtype, B, Hkv, Skv, D, 1 + Skv % 3, False)
    vbuf, dv = _guarded(dev, dtype, B, Hkv, Skv, D, Skv % 2, True)
    ws_bytes = int(_lib.lib().mra_prefill_attention_backward_workspace_bytes(B, Hq, Sq))
    assert ws_bytes == BC.workspace_bytes(B, Hq, Sq)
    wbuf = torch.full((2 * GUARD + ws_bytes // 4,), SENT, dtype=torch.float32, device=dev)
    ws = wbuf[GUARD: GUARD + ws_bytes // 4]
    for t in (q, k, v, dout, out, dq, dk, dv, ws):
        assert t.data_ptr() % 16 == 0
    _lib.check(_call(case, dtype, c, q, k, v, mask, m_sb, dout, out, lse, dq, dk, dv, ws, ws_bytes), "prefill_attention_backward")
    assert _sentinels_kept(qbuf, dq) and _sentinels_kept(kbuf, dk) and _sentinels_kept(vbuf, dv), case
    assert bool(torch.isnan(wbuf[:GUARD]).all() and torch.isnan(wbuf[GUARD + ws_bytes // 4:]).all()), case
    assert torch.equal(q.cpu().view(torch.int16), c["q"].view(torch.int16)) and torch.equal(k.cpu().view(torch.int16), c["k"].view(torch.int16))
    return dq.clone(), dk.clone(), dv.clone()


def _bits(ts):
    return [t.contiguous().view(torch.int16) for t in ts]


@pytest.mark.parametrize("dtype", BC.DTYPES, ids=_id)
def test_entry_against_float64(dev, dtype):
    worst = [0.0, 0.0, 0.0]
    for case in CASES:
        got = _run(dev, case, dtype)
        r = BC.ratios(*case, dtype, *got)
        print(f"prefill_attention_backward {_id(dtype)} {case}: |d| / bound dq {r[0]:.3g} dk {r[1]:.3g} dv {r[2]:.3g}")
        assert max(r) <= 1.0, (case, r)
        worst = [max(a, b) for a, b in zip(worst, r)]
        again = _run(dev, case, dtype)                                               # two runs, the same bits
        assert all(torch.equal(a, b) for a, b in zip(_bits(got), _bits(again))), case
    print(f"prefill_attention_backward {_id(dtype)}: worst |d| / bound dq {worst[0]:.3g} dk {worst[1]:.3g} dv {worst[2]:.3g}")
    assert all(w > 0.0 for w in worst)


@pytest.mark.parametrize("dtype", BC.DTYPES, ids=_id)
def test_forward_entry_chained_into_the_backward(dev, dtype):
    """``mra_prefill_attention``'s own out and lse into the backward: inside the backward's bound around float64 of the values it was given,
    and around the float64 backward of the float64 forward inside the sum of the two bounds (the forward's lse_b and out_b carried, first
    order, through the backward's sums: ``reference_tensors(lse_err=, out_err=)``)."""
    case = (3, 8, 2, 2 * BC.KB + 3, 2 * BC.KB + 3, 0, 128, "holes") if dtype == torch.bfloat16 else (3, 4, 2, BC.KB + 1, 3 * BC.KB, BC.KB - 1, 64, "left_pad")
    B, Hq, Hkv, Sq, Skv, off, D, _ = case
    c, q, k, v, mask, m_sb, dout, _, _ = _operands(dev, case, dtype)
    km = None if c["mask"] is None else c["mask"].to(dev)[:, None, None, :]
    out, lse = LD.prefill_attention(q, k, v, km, c["scale"], q_offset=off, hip=True, want_lse=True)
    fwd = PC.reference(*case, dtype)
    assert max(PC.ratios_against(fwd, out, lse)) <= 1.0
    got = _run(dev, case, dtype, ops=(c, q, k, v, mask, m_sb, dout, out, lse))
    given = BC.reference_tensors(c["q"], c["k"], c["v"], c["mask"], c["dout"], out.cpu(), lse.cpu(), c["scale"], off, dtype)
    r_given = BC.ratios_against(given, *got)
    f = BC._forward64(c["q"], c["k"], c["v"], c["mask"], c["scale"], off)                # the exact forward: unrounded lse and out
    exact = BC.reference_tensors(c["q"], c["k"], c["v"], c["mask"], c["dout"], f["out"].transpose(1, 2), f["lse"], c["scale"], off, dtype,
                                 lse_err=fwd["lse_b"], out_err=fwd["out_b"])
    r = BC.ratios_against(exact, *got)
    print(f"chained {_id(dtype)} {case}: |d| / bound around the values given dq {r_given[0]:.3g} dk {r_given[1]:.3g} dv {r_given[2]:.3g}; "
          f"around the exact backward, inside the sum of the two bounds dq {r[0]:.3g} dk {r[1]:.3g} dv {r[2]:.3g}")
    assert max(r_given) <= 1.0 and max(r) <= 1.0


def test_zero_batch_and_refusals_touch_nothing(dev):
    case = (1, 4, 2, 33, 33, 0, 64, "holes")
    dtype = torch.bfloat16
    B, Hq, Hkv, Sq, Skv, off, D, _ = case
    ops = _operands(dev, case, dtype)
    outs = [torch.full((B, H, S, D), SENT, dtype=dtype, device=dev) for H, S in ((Hq, Sq), (Hkv, Skv), (Hkv, Skv))]
    n = int(_lib.lib().mra_prefill_attention_backward_workspace_bytes(B, Hq, Sq))
    ws = torch.full((n // 4,), SENT, dtype=torch.float32, device=dev)
    assert _call((0,) + case[1:], dtype, *ops, *outs, ws, n) == 0
    assert _call(case, dtype, *ops, *outs, ws, n - 1) == -1 and b"workspace too small" in _lib.lib().mra_last_error()
    assert _call(case[:5] + (1,) + case[6:], dtype, *ops, *outs, ws, n) == -1 and b"q_offset" in _lib.lib().mra_last_error()
    torch.cuda.synchronize(dev)
    assert all(bool(torch.isnan(t).all()) for t in outs + [ws])


def test_python_node_takes_the_entries_and_the_torch_ops_otherwise(dev):
    dtype = torch.bfloat16
    case = (3, 8, 2, BC.KB + 1, BC.KB + 1, 0, 128, "left_pad")
    B, Hq, Hkv, Sq, Skv, off, D, _ = case
    c = BC.make_case(*case, dtype)
    ref = BC.reference(*case, dtype)
    km = c["mask"].to(dev)[:, None, None, :]
    leaves = lambda: [t.to(dev).nan_to_num(0, 0, 0).requires_grad_(True) for t in (c["q"], c["k"], c["v"])]      # noqa: E731
    q, k, v = leaves()
    qt = q.transpose(1, 2).contiguous().transpose(1, 2)                                # as transformers hands it over
    out = LA.causal_attention(qt, k, v, km, c["scale"], hip=True)
    assert out.grad_fn is not None and type(out.grad_fn).__name__ == "_CausalAttentionBackward" and out.shape == (B, Sq, Hq, D)
    assert torch.equal(out, LD.prefill_attention(qt.detach(), k.detach(), v.detach(), km, c["scale"], hip=True))
    dout = c["dout"].to(dev)
    out.backward(dout)
    # out and lse are the forward entry's own: the chained test's bound around the exact backward
    fwd = PC.reference(*case, dtype)
    f = BC._forward64(c["q"], c["k"], c["v"], c["mask"], c["scale"], off)
    exact = BC.reference_tensors(c["q"], c["k"], c["v"], c["mask"], c["dout"], f["out"].transpose(1, 2), f["lse"], c["scale"], off, dtype,
                                 lse_err=fwd["lse_b"], out_err=fwd["out_b"])
    assert q.grad.shape == q.shape and k.grad.shape == k.shape and v.grad.shape == v.shape and q.grad.dtype == dtype
    assert max(BC.ratios_against(exact, q.grad, k.grad, v.grad)) <= 1.0
    q2, k2, v2 = leaves()
    LA.causal_attention(q2, k2, v2, km, c["scale"], hip=False).backward(dout)          # the torch ops under autograd: the oracle's route
    for a, b in ((q.grad, q2.grad), (k.grad, k2.grad), (v.grad, v2.grad)):
        assert a.shape == b.shape and b.dtype == dtype and bool(torch.isfinite(b).all())
        assert ((a.double() - b.double()).norm() / b.double().norm()).item() <= 8 * BC.U[dtype]      # two roundings of every tensor apart
    with torch.no_grad():
        assert torch.equal(LA.causal_attention(qt, k, v, km, c["scale"]), out.detach())
    with pytest.raises(_lib.MraError, match="16-bit"):
        LA.causal_attention(q.float(), k.float(), v.float(), km, c["scale"], hip=True)


# ---- the model ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kv_heads", [4, 2])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_every_attention_backward_of_a_real_training_step_is_inside_the_bound(dev, dtype, kv_heads, monkeypatch):
    from mraudio_amd.models.lora import lora_modules
    from test_gpu_lm_step import PREFIX, _llama, _prefix

    llm, _ = _llama(dev, kv_heads, dtype, True)
    for m in lora_modules(llm).values():
        for p in list(m.lora_A.parameters()) + list(m.lora_B.parameters()):
            p.requires_grad_(True)
    llm.train()
    embeds, mask = _prefix(dev, dtype)
    labels = torch.randint(3, llm.config.vocab_size, mask.shape, generator=torch.Generator().manual_seed(4)).to(dev)
    labels[:, :PREFIX - 40] = -100
    labels = labels.masked_fill(mask == 0, -100)
    seen = []
    real = LA._backward_entry

    def spy(q, k, v, key_mask, out, dout, lse, scale, q_offset):
        got = real(q, k, v, key_mask, out, dout, lse, scale, q_offset)
        assert key_mask.dtype == torch.bool and tuple(key_mask.shape) == (3, 1, 1, k.shape[2]) and k.shape[1] == kv_heads and q_offset == 0
        assert got[0].shape == q.shape and got[1].shape == k.shape and got[2].shape == v.shape
        ref = BC.reference_tensors(q.cpu(), k.cpu(), v.cpu(), key_mask[:, 0, 0].cpu(), dout.cpu(), out.cpu(), lse.cpu(), scale, 0, dtype)
        seen.append((BC.ratios_against(ref, *got), q.shape[2], k.shape[2], got[0].stride()))
        return got

    monkeypatch.setattr(LA, "_backward_entry", spy)
    before = llm.config._attn_implementation
    x = embeds.clone().requires_grad_(True)
    with LA.hip_train(llm):
        loss = llm(inputs_embeds=x, attention_mask=mask, labels=labels, return_dict=True).loss * 64.0      # f16 cotangents above the subnormals
    loss.backward()
    assert llm.config._attn_implementation == before and bool(torch.isfinite(x.grad).all())
    assert len(seen) == llm.config.num_hidden_layers and all(s[1] == s[2] == PREFIX for s in seen)
    worst = [max(s[0][i] for s in seen) for i in range(3)]
    print(f"{_id(dtype)} kv heads {kv_heads}: {len(seen)} attention backward calls of {PREFIX} rows, dq strides {seen[0][3]}; worst |d| / bound "
          f"dq {worst[0]:.3g} dk {worst[1]:.3g} dv {worst[2]:.3g}")
    assert all(0.0 < w <= 1.0 for w in worst)


def _train_model(dev, dropout):
    from test_gpu_llm_objective import _batch, _model, _tiny_llama
    from test_gpu_lora import _randomise_B

    llm, tok = _tiny_llama(dev)
    model = _model(dev, llm, tok)
    model.objective = "llm"
    model.enable_lora(r=8, alpha=8, dropout=dropout)
    return llm, model, _batch(dev), _randomise_B


def test_lm_attention_hip_against_stock_on_the_tiny_llama(dev, monkeypatch):
    """Loss: the stock-vs-fused bar of tests/test_gpu_lm_head.py, 2 * 2^-8 * max|z| over the fp32 logits of the labelled rows (either route
    rounds its attention output once to bf16; what that moves in a logit is far inside one rounding of the logit itself).  Gradients: the
    bars of tests/test_gpu_backward.py for a gradient tensor."""
    from test_gpu_backward import DTYPES
    from test_gpu_lm_head import _labelled_logit_peak
    from test_gpu_lora import _adapter_grads

    rel_tol, peak_tol = next((d[2], d[3]) for d in DTYPES if d[0] == torch.bfloat16)
    llm, model, batch, randomise = _train_model(dev, 0.05)
    model.enable_qformer_training(train_proj=True)
    randomise(model)
    model.train()
    routed = []
    real = LA.causal_attention
    monkeypatch.setattr(LA, "causal_attention", lambda *a, **kw: routed.append(a[0].is_cuda) or real(*a, **kw))
    zmax, n = _labelled_logit_peak(model, batch)
    bar = 2 * 2.0 ** -8 * zmax
    impl, state = llm.config._attn_implementation, {k: v.clone() for k, v in llm.state_dict().items()}
    runs = {}
    for mode in ("before", "stock", "hip", "again"):
        model.lm_attention = "hip" if mode == "hip" else "stock"
        for p in model.lora_parameters() + list(model.video_llm_proj.parameters()) + list(model.audio_llm_proj.parameters()):
            p.grad = None
        for m in model.modalities:
            getattr(model, f"{m}_Qformer")._grad_flat.zero_()
        torch.manual_seed(21)                                                        # the same seeds, hence the same dropout masks
        count = len(routed)
        loss = model(batch)["loss"]
        loss.backward()
        torch.cuda.synchronize(dev)
        assert len(routed) - count == (llm.config.num_hidden_layers if mode == "hip" else 0) and all(routed)
        assert llm.config._attn_implementation == impl and all(torch.equal(v, llm.state_dict()[k]) for k, v in state.items())
        runs[mode] = (loss.detach().clone(), _adapter_grads(model) + [model.video_llm_proj.weight.grad.clone(), model.audio_llm_proj.weight.grad.clone(),
                                                                     model.video_Qformer._grad_flat.clone(), model.audio_Qformer._grad_flat.clone()])
    d = abs(runs["hip"][0].item() - runs["stock"][0].item())
    print(f"LM loss on {n} labelled rows: stock {runs['stock'][0].item():.6f} hip {runs['hip'][0].item():.6f}, |d| {d:.3g}, bar 2 * 2^-8 * max|z| = {bar:.3g}")
    assert n > 0 and d <= bar
    worst = (0.0, 0.0)
    for got, ref in zip(runs["hip"][1], runs["stock"][1]):
        assert torch.isfinite(got).all() and ref.abs().max().item() > 0
        rel = ((got - ref).norm() / ref.norm()).item()
        peak = (got - ref).abs().max().item() / ref.abs().max().item()
        worst = (max(worst[0], rel), max(worst[1], peak))
        assert rel < rel_tol and peak < peak_tol, (rel, peak)
    print(f"hip against stock, gradients of adapters / llm_proj / Q-Formers: worst rel {worst[0]:.3g} (bar {rel_tol}), worst peak {worst[1]:.3g} "
          f"(bar {peak_tol})")
    # a following stock call: the bits of the one made before -- the loss always, a gradient wherever two stock calls in a row give the same
    # bits themselves (the stock backward has atomics of its own)
    assert torch.equal(runs["again"][0], runs["stock"][0]) and torch.equal(runs["before"][0], runs["stock"][0])
    same = [torch.equal(a, b) for a, b in zip(runs["before"][1], runs["stock"][1])]
    assert sum(same) >= len(same) // 2, same                                          # else the check below would say nothing
    print(f"{sum(same)} of {len(same)} gradient tensors are the same bits over two stock calls in a row; those are checked behind the hip call")
    assert all(torch.equal(a, b) for a, b, s in zip(runs["again"][1], runs["stock"][1], same) if s)


def test_three_adam_steps_under_lm_attention_hip_lower_the_loss(dev):
    llm, model, batch, _ = _train_model(dev, 0.0)
    model.lm_attention = "hip"
    model.train()
    opt = torch.optim.Adam(model.lora_parameters(), lr=1e-3, fused=True)
    losses = []
    for it in range(4):
        opt.zero_grad(set_to_none=False)
        loss = model(batch)["loss"]
        assert torch.isfinite(loss) and loss.requires_grad
        losses.append(loss.item())
        if it == 3:
            break
        loss.backward()
        opt.step()
    print("LM loss over three fused-Adam steps on the adapters, lm_attention = hip:", losses)
    assert losses[3] < losses[0], losses


def _lm_run(llm, params, embeds, mask, labels, hip):
    """One forward + backward of the bare LM (loss x 64: f16 cotangents above the subnormals): (loss, adapter gradients)."""
    import contextlib

    for p in params:
        p.grad = None
    torch.manual_seed(21)                                                            # the same seeds, hence the same dropout masks
    with (LA.hip_train(llm) if hip else contextlib.nullcontext()):
        loss = llm(inputs_embeds=embeds, attention_mask=mask, labels=labels, return_dict=True).loss
    (loss * 64.0).backward()
    return loss.detach().clone(), [p.grad.clone() for p in params]


@pytest.mark.parametrize("kv_heads", [4, 2])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_hip_train_against_stock_on_the_bare_llamas(dev, dtype, kv_heads, monkeypatch):
    """The model-level checks on the LMs of the per-call test (4 and 2 K/V heads, B = 3, a prefix of 300 with left padding and holes,
    adapters on): the loss inside 2 U[T] max|z| of stock (z: the fp32 logits of the labelled rows), every adapter gradient inside the bars of
    tests/test_gpu_backward.py, a following stock call, three fused-Adam steps."""
    from mraudio_amd.models.lora import lora_modules
    from test_gpu_backward import DTYPES
    from test_gpu_lm_step import PREFIX, _llama, _prefix

    rel_tol, peak_tol = next((d[2], d[3]) for d in DTYPES if d[0] == dtype)
    llm, _ = _llama(dev, kv_heads, dtype, True)
    params = [p for m in lora_modules(llm).values() for p in list(m.lora_A.parameters()) + list(m.lora_B.parameters())]
    for p in params:
        p.requires_grad_(True)
    llm.train()
    embeds, mask = _prefix(dev, dtype)
    labels = torch.randint(3, llm.config.vocab_size, mask.shape, generator=torch.Generator().manual_seed(4)).to(dev)
    labels[:, :PREFIX - 40] = -100
    labels = labels.masked_fill(mask == 0, -100)
    routed = []
    real = LA.causal_attention
    monkeypatch.setattr(LA, "causal_attention", lambda *a, **kw: routed.append(a[0].is_cuda) or real(*a, **kw))
    with torch.no_grad():
        hidden = llm.eval().get_decoder()(inputs_embeds=embeds, attention_mask=mask, return_dict=True).last_hidden_state
        llm.train()
        rows = hidden[:, :-1][labels[:, 1:] != -100]                                 # position t predicts label t + 1
        zmax = (rows.float() @ llm.lm_head.weight.float().t()).abs().max().item()
    bar = 2 * BC.U[dtype] * zmax
    impl, state = llm.config._attn_implementation, {k: v.clone() for k, v in llm.state_dict().items()}
    runs = {}
    for mode in ("before", "stock", "hip", "again"):
        count = len(routed)
        runs[mode] = _lm_run(llm, params, embeds, mask, labels, mode == "hip")
        torch.cuda.synchronize(dev)
        assert len(routed) - count == (llm.config.num_hidden_layers if mode == "hip" else 0) and all(routed)
        assert llm.config._attn_implementation == impl and all(torch.equal(v, llm.state_dict()[k]) for k, v in state.items())
    d = abs(runs["hip"][0].item() - runs["stock"][0].item())
    print(f"{_id(dtype)} kv heads {kv_heads}: LM loss on {rows.shape[0]} labelled rows: stock {runs['stock'][0].item():.6f} hip {runs['hip'][0].item():.6f}, "
          f"|d| {d:.3g}, bar 2 U[T] max|z| = {bar:.3g}")
    assert rows.shape[0] > 0 and d <= bar
    worst = (0.0, 0.0)
    for got, ref in zip(runs["hip"][1], runs["stock"][1]):
        assert torch.isfinite(got).all() and ref.abs().max().item() > 0
        rel = ((got - ref).norm() / ref.norm()).item()
        peak = (got - ref).abs().max().item() / ref.abs().max().item()
        worst = (max(worst[0], rel), max(worst[1], peak))
        assert rel < rel_tol and peak < peak_tol, (rel, peak)
    print(f"{_id(dtype)} kv heads {kv_heads}: hip against stock, {len(params)} adapter gradients: worst rel {worst[0]:.3g} (bar {rel_tol}), worst peak "
          f"{worst[1]:.3g} (bar {peak_tol})")
    assert torch.equal(runs["again"][0], runs["stock"][0]) and torch.equal(runs["before"][0], runs["stock"][0])
    same = [torch.equal(a, b) for a, b in zip(runs["before"][1], runs["stock"][1])]
    assert sum(same) >= len(same) // 2, same
    print(f"{_id(dtype)} kv heads {kv_heads}: {sum(same)} of {len(same)} adapter gradients are the same bits over two stock calls in a row")
    assert all(torch.equal(a, b) for a, b, s in zip(runs["again"][1], runs["stock"][1], same) if s)
    opt = torch.optim.Adam(params, lr=1e-3, fused=True)
    losses = []
    for it in range(4):
        losses.append(_lm_run(llm, params, embeds, mask, labels, True)[0].item())
        if it < 3:
            opt.step()
    print(f"{_id(dtype)} kv heads {kv_heads}: LM loss over three fused-Adam steps on the adapters under hip_train:", losses)
    assert losses[3] < losses[0], losses


@pytest.mark.parametrize("reentrant", [True, False], ids=["reentrant", "non_reentrant"])
def test_activation_checkpointing_gives_the_bits_of_the_plain_hip_step(dev, reentrant, monkeypatch):
    """The node is deterministic and ``hold_for_backward`` keeps the training attention in force for the recomputation: a checkpointed
    ``_lm_ce`` under ``lm_attention="hip"`` gives the loss and the adapter gradients of the un-checkpointed one, bit for bit."""
    from mraudio_amd.models.lora import lora_modules
    from mraudio_amd.models.xinstructblip import XInstructBLIP
    from test_gpu_lm_step import PREFIX, _llama, _prefix

    class Ce:
        lm_loss, lm_attention, _lm_ce = "stock", "hip", XInstructBLIP._lm_ce

    dtype = torch.bfloat16
    llm, _ = _llama(dev, 2, dtype, True)
    params = [p for m in lora_modules(llm).values() for p in list(m.lora_A.parameters()) + list(m.lora_B.parameters())]
    for p in params:
        p.requires_grad_(True)
    llm.train()
    model = Ce()
    model.llm_model = llm
    embeds, mask = _prefix(dev, dtype)
    labels = torch.randint(3, llm.config.vocab_size, mask.shape, generator=torch.Generator().manual_seed(4)).to(dev)
    labels[:, :PREFIX - 40] = -100
    labels = labels.masked_fill(mask == 0, -100)
    calls = []
    real = LA._backward_entry
    monkeypatch.setattr(LA, "_backward_entry", lambda *a: calls.append(1) or real(*a))
    impl = llm.config._attn_implementation

    def step():
        for p in params:
            p.grad = None
        torch.manual_seed(21)
        x = embeds.clone().requires_grad_(True)
        loss = model._lm_ce(x, mask, labels)
        assert llm.config._attn_implementation == impl
        loss.backward()
        torch.cuda.synchronize(dev)
        assert llm.config._attn_implementation == impl
        return loss.detach().clone(), [p.grad.clone() for p in params] + [x.grad.clone()]

    plain = step()
    llm.gradient_checkpointing_enable(gradient_checkpointing_kwargs={"use_reentrant": reentrant})
    n = len(calls)
    ckpt = step()
    assert len(calls) - n == llm.config.num_hidden_layers == n                       # every backward went through the entry, none through SDPA
    assert torch.equal(plain[0], ckpt[0]) and all(torch.equal(a, b) for a, b in zip(plain[1], ckpt[1]))
