"""The LM head + cross-entropy on the labelled rows on the GPU (``-m gpu``): ``mra_lm_head_ce_forward`` / ``mra_lm_head_ce_backward`` on every
element of nll, lse and dh against float64 under the DERIVED bounds of tests/lm_head_cases.py, with sentinel-filled outputs between guards,
pitched h / W / dh, a workspace guarded at ``workspace_bytes``, two runs bit for bit, want_grad 0 against 1, R = 0; and the model's
``lm_loss = "fused"`` on the tiny bf16 Llama of tests/test_gpu_llm_objective.py (V = 260, K = 256).

Bars of the model level.  Loss, "fused" against "stock": 2 * 2^-8 * max|z| over the fp32 logits z of the labelled rows, computed here -- the
stock route rounds its logits to bf16 (half an ulp: 2^-9 |z| each) before the upcast and this one does not; lse and the target logit each move
by at most that, and the factor 2 on top covers the two together twice over.  Gradients, "fused" against "rows": the bars of
tests/test_gpu_backward.py for a gradient tensor (``DTYPES``, imported)."""
import pytest
import torch

import lm_head_cases as HC
from mraudio_amd import _lib
from mraudio_amd.models import lm_head as H
from test_gpu_backward import DTYPES
from test_gpu_llm_objective import _batch, _model, _tiny_llama
from test_gpu_lora import _adapter_grads, _randomise_B

pytestmark = pytest.mark.gpu

GUARD = 64                       # elements on either side of every output (a multiple of 8: the views stay 16-byte aligned)
SENT = 77.0                      # exact in f16, bf16 and fp32
WS_GUARD, WS_SENT = 256, 0xA5    # bytes behind the workspace


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _id(dt):
    return "f16" if dt == torch.float16 else "bf16"


def _guarded(t: torch.Tensor, ld: int, dev):
    rows, width = t.shape
    buf = torch.full((2 * GUARD + rows * ld,), SENT, dtype=t.dtype, device=dev)
    view = buf[GUARD: GUARD + rows * ld].view(rows, ld)[:, :width]
    view.copy_(t)
    assert view.data_ptr() % 16 == 0
    return buf, view


def _guards_intact(buf: torch.Tensor, rows: int, width: int, ld: int) -> bool:
    body = buf[GUARD: GUARD + rows * ld].view(rows, ld)
    return bool((buf[:GUARD] == SENT).all() and (buf[GUARD + rows * ld:] == SENT).all() and (body[:, width:] == SENT).all())


def _run(dev, R, V, K, dtype, want_grad=True, backward=True):
    """One forward (+ backward) through the entries on guarded, pitched buffers: (nll, lse, dh or None) on the device, after the guard checks."""
    lib, stream = _lib.lib(), _lib.current_stream()
    c = HC.make_case(R, V, K, dtype)
    ldh, ldw, lddh = HC.pitches(R, V, K)
    dt = _lib.mra_dtype(dtype)
    hbuf, h = _guarded(c["h"], ldh, dev)
    wbuf, W = _guarded(c["W"], ldw, dev)
    labels, g = c["labels"].to(dev), c["g"].to(dev)
    nbuf, nll = _guarded(torch.full((1, R), SENT), R, dev)
    lbuf, lse = _guarded(torch.full((1, R), SENT), R, dev)
    nbytes = int(lib.mra_lm_head_ce_workspace_bytes(R, V, K, dt, int(want_grad)))
    assert nbytes == HC.workspace_bytes(R, V, K, want_grad)
    ws = torch.full((nbytes + WS_GUARD,), WS_SENT, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 16 == 0
    _lib.check(lib.mra_lm_head_ce_forward(_lib.ptr(h), ldh, R, K, _lib.ptr(W), ldw, V, dt, _lib.ptr(labels), _lib.ptr(nll), _lib.ptr(lse), _lib.ptr(ws),
                                          nbytes, int(want_grad), stream), "forward")
    dh = None
    if backward:
        dbuf, dh = _guarded(torch.full((R, K), SENT, dtype=dtype), lddh, dev)
        _lib.check(lib.mra_lm_head_ce_backward(_lib.ptr(g), _lib.ptr(W), ldw, V, K, dt, _lib.ptr(labels), _lib.ptr(lse), _lib.ptr(ws), nbytes, _lib.ptr(dh),
                                               lddh, R, stream), "backward")
        assert _guards_intact(dbuf, R, K, lddh), (R, V, K)
    assert bool((ws[nbytes:] == WS_SENT).all()), (R, V, K)
    assert _guards_intact(nbuf, 1, R, R) and _guards_intact(lbuf, 1, R, R) and _guards_intact(hbuf, R, K, ldh) and _guards_intact(wbuf, V, K, ldw)
    assert torch.equal(W.cpu(), c["W"]) and torch.equal(h.cpu(), c["h"])
    return nll[0], lse[0], dh


@pytest.mark.parametrize("dtype", HC.DTYPES, ids=_id)
def test_entries_against_float64(dev, dtype):
    worst = [0.0, 0.0, 0.0]
    for R, V, K in HC.cases():
        nll, lse, dh = _run(dev, R, V, K, dtype)
        r = HC.ratios(R, V, K, dtype, nll, lse, dh)
        print(f"lm_head_ce {_id(dtype)} R {R} V {V} K {K}: |d| / bound nll {r[0]:.3g} lse {r[1]:.3g} dh {r[2]:.3g}")
        assert max(r) <= 1.0, ((R, V, K), r)
        worst = [max(a, b) for a, b in zip(worst, r)]
        nll2, lse2, dh2 = _run(dev, R, V, K, dtype)                                  # two runs, the same bits (NaN rows compared as bits)
        assert torch.equal(nll.view(torch.int32), nll2.view(torch.int32)) and torch.equal(lse, lse2) and torch.equal(dh, dh2), (R, V, K)
        nll0, lse0, _ = _run(dev, R, V, K, dtype, want_grad=False, backward=False)
        assert torch.equal(nll.view(torch.int32), nll0.view(torch.int32)) and torch.equal(lse, lse0), (R, V, K)
    print(f"lm_head_ce {_id(dtype)}: worst |d| / bound nll {worst[0]:.3g} lse {worst[1]:.3g} dh {worst[2]:.3g}")
    assert all(w > 0.0 for w in worst)


def test_zero_rows_touch_nothing(dev):
    lib, stream = _lib.lib(), _lib.current_stream()
    out = torch.full((64,), SENT, device=dev)
    W = torch.full((16, 8), SENT, dtype=torch.bfloat16, device=dev)
    assert lib.mra_lm_head_ce_workspace_bytes(0, 16, 8, _lib.MRA_BF16, 1) == 0
    assert lib.mra_lm_head_ce_forward(_lib.ptr(out), 8, 0, 8, _lib.ptr(W), 8, 16, _lib.MRA_BF16, _lib.ptr(out), _lib.ptr(out), _lib.ptr(out), _lib.ptr(out),
                                      0, 1, stream) == 0
    assert lib.mra_lm_head_ce_backward(_lib.ptr(out), _lib.ptr(W), 8, 16, 8, _lib.MRA_BF16, _lib.ptr(out), _lib.ptr(out), _lib.ptr(out), 0, _lib.ptr(out),
                                       8, 0, stream) == 0
    torch.cuda.synchronize(dev)
    assert bool((out == SENT).all()) and bool((W == SENT).all())
    # the Python entry with no labelled row: cross_entropy's own answer, through the torch route
    hidden = torch.randn(2, 5, 8, device=dev, dtype=torch.bfloat16, requires_grad=True)
    loss = H.lm_head_ce(hidden, W, torch.full((2, 5), -100, device=dev))
    assert torch.isnan(loss) and loss.requires_grad


@pytest.mark.parametrize("dtype", HC.DTYPES, ids=_id)
def test_python_entry_is_one_node_and_scatters_back(dev, dtype):
    R, V, K = 17, 513, 200
    c, ref = HC.make_case(R, V, K, dtype), HC.reference(R, V, K, dtype)
    ok = ref["valid"]
    B, S = 2, 40
    pos = torch.randperm(B * (S - 1), generator=torch.Generator().manual_seed(1))[:int(ok.sum())].sort().values      # flat (b, t) with t < S - 1
    b, t = pos // (S - 1), pos % (S - 1)
    hidden = torch.randn(B, S, K, generator=torch.Generator().manual_seed(2)).to(dtype)
    hidden[b, t] = c["h"][ok]
    labels = torch.full((B, S), -100)
    labels[b, t + 1] = c["labels"][ok].long()
    hd = hidden.to(dev).requires_grad_(True)
    W = c["W"].to(dev)
    none = H.lm_head_ce(hd, W, labels.to(dev), hip=True, reduction="none")
    assert none.grad_fn is not None and type(none.grad_fn).__name__ == "_LmHeadCEBackward"
    assert HC.ratio(none.detach().cpu(), ref["nll"][ok], ref["nll_b"][ok]) <= 1.0
    (none * c["g"][ok].to(dev)).sum().backward()
    grad = hd.grad.cpu()
    assert HC.ratio(grad[b, t], ref["dh"][ok], ref["dh_b"][ok]) <= 1.0
    keep = torch.ones(B, S, dtype=torch.bool)
    keep[b, t] = False
    assert bool((grad[keep] == 0).all())
    hd.grad = None
    mean = H.lm_head_ce(hd, W, labels.to(dev))
    assert abs(mean.item() - ref["nll"][ok].mean().item()) <= ref["nll_b"][ok].max().item() + 1e-6 * abs(mean.item())
    (mean * 3.0).backward()                                                          # g_r = grad_output / n on the device
    n = int(ok.sum())
    want = ref["dh"][ok] / c["g"][ok].double()[:, None] * 3.0 / n
    bound = ref["dh_b"][ok] / c["g"][ok].double().abs()[:, None] * 3.0 / n
    rows = c["g"][ok] != 0
    assert HC.ratio(hd.grad.cpu()[b, t][rows], want[rows], bound[rows] * 1.01 + 2.0 ** -24 * (1.0 + want[rows].abs())) <= 1.0
    with pytest.raises(_lib.MraError, match="gradient"):
        H.lm_head_ce(hd, W.clone().requires_grad_(True), labels.to(dev), hip=True)
    with pytest.raises(_lib.MraError, match="dtype"):
        H.lm_head_ce(hd.float(), W, labels.to(dev), hip=True)


# ---- the model ----------------------------------------------------------------------------------------------------------------------------------
def _labelled_logit_peak(model, batch):
    """max |z| over the fp32 logits of the labelled rows, from the LM's own hidden states."""
    with torch.no_grad():
        inputs_llm, atts = model._llm_inputs(batch)
        embeds, mask, targets = model.prompt_assembler.assemble_forward(batch, inputs_llm, atts)
        hidden = model.llm_model.get_decoder()(inputs_embeds=embeds, attention_mask=mask, return_dict=True).last_hidden_state
        index, _ = H.labelled_rows(targets)
        rows = hidden.reshape(-1, hidden.shape[-1]).index_select(0, index)
        return (rows.float() @ model.llm_model.lm_head.weight.float().t()).abs().max().item(), int(index.numel())


def test_fused_loss_and_gradients_on_the_tiny_llama(dev):
    rel_tol, peak_tol = next((d[2], d[3]) for d in DTYPES if d[0] == torch.bfloat16)
    llm, tok = _tiny_llama(dev)
    model = _model(dev, llm, tok)
    batch = _batch(dev)
    fired = []
    llm.lm_head.register_forward_hook(lambda *a: fired.append(1))
    with torch.no_grad():
        stock = model.forward_llm(batch, train=False)["loss"].item()
        assert fired == [1]
        model.lm_loss = "fused"
        fused = model.forward_llm(batch, train=False)["loss"].item()
        assert fired == [1]
    zmax, n = _labelled_logit_peak(model, batch)
    bar = 2 * 2.0 ** -8 * zmax
    print(f"LM loss on {n} labelled rows: stock {stock:.6f} fused {fused:.6f}, |d| {abs(stock - fused):.3g}, bar 2 * 2^-8 * max|z| = {bar:.3g}")
    assert n > 0 and abs(stock - fused) <= bar
    del fired[:]
    model.objective = "llm"
    model.enable_lora(r=8, alpha=8, dropout=0.05)
    model.enable_qformer_training(train_proj=True)
    _randomise_B(model)
    model.train()
    runs = {}
    for mode in ("fused", "rows"):
        model.lm_loss = mode
        for p in model.lora_parameters() + list(model.video_llm_proj.parameters()) + list(model.audio_llm_proj.parameters()):
            p.grad = None
        for m in model.modalities:
            getattr(model, f"{m}_Qformer")._grad_flat.zero_()
        torch.manual_seed(21)                                                        # the same seeds, hence the same dropout masks
        loss = model(batch)["loss"]
        loss.backward()
        torch.cuda.synchronize(dev)
        runs[mode] = (loss.item(), _adapter_grads(model) + [model.video_llm_proj.weight.grad.clone(), model.audio_llm_proj.weight.grad.clone(),
                                                           model.video_Qformer._grad_flat.clone(), model.audio_Qformer._grad_flat.clone()])
    assert fired == []
    assert abs(runs["fused"][0] - runs["rows"][0]) <= bar
    worst = (0.0, 0.0)
    for got, ref in zip(runs["fused"][1], runs["rows"][1]):
        assert torch.isfinite(got).all() and ref.abs().max().item() > 0
        rel = ((got - ref).norm() / ref.norm()).item()
        peak = (got - ref).abs().max().item() / ref.abs().max().item()
        worst = (max(worst[0], rel), max(worst[1], peak))
        assert rel < rel_tol and peak < peak_tol, (rel, peak)
    print(f"fused against rows, gradients of adapters / llm_proj / Q-Formers: worst rel {worst[0]:.3g} (bar {rel_tol}), worst peak {worst[1]:.3g} "
          f"(bar {peak_tol})")


def test_three_adam_steps_under_fused_lower_the_loss(dev):
    llm, tok = _tiny_llama(dev)
    model = _model(dev, llm, tok)
    batch = _batch(dev)
    model.objective, model.lm_loss = "llm", "fused"
    model.enable_lora(r=8, alpha=8, dropout=0.0)
    model.train()
    fired = []
    llm.lm_head.register_forward_hook(lambda *a: fired.append(1))
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
    print("LM loss over three fused-Adam steps on the adapters, lm_loss = fused:", losses)
    assert losses[3] < losses[0], losses
    assert fired == [] and llm.lm_head.weight.grad is None


def test_trainer_takes_lm_loss_and_trains_the_adapters(dev, tmp_path):
    from mraudio_amd.utils.trainer import Trainer, default_args

    llm, tok = _tiny_llama(dev)
    model = _model(dev, llm, tok)
    fired = []
    llm.lm_head.register_forward_hook(lambda *a: fired.append(1))
    kw = dict(output_dir=str(tmp_path), gpu=0, synthetic=4, dataset="Charades_STA", lr=1e-3, warmup_steps=1, objective="llm", lora=True,
              train_qformers=False, val_freq=2)
    with pytest.raises(ValueError, match="lm_loss"):
        Trainer(default_args(max_epoch=1, **dict(kw, lm_loss="fast")), model=model)
    with pytest.raises(ValueError, match="objective"):
        Trainer(default_args(max_epoch=1, **dict(kw, objective="score", lora=False, lm_loss="fused")), model=model)
    assert model.lm_loss == "stock"
    tr = Trainer(default_args(max_epoch=2, lm_loss="fused", **kw), model=model)
    assert model.lm_loss == "fused" and model.lora
    tr.train()
    assert len(tr.history) == 2 and tr.history[1]["loss_value"] < tr.history[0]["loss_value"], tr.history
    assert fired == []                                                               # training never ran lm_head; validation is the scorer's
