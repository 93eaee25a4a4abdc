"""The LoRA branch on the GPU (``-m gpu``): ``mra_lora_down`` / ``mra_lora_up_add`` / ``mra_lora_wgrad`` on every element against float64
under the DERIVED bounds of tests/lora_cases.py, with guards around every output, pitched views, prefilled gradients and rows = 0; the mask
the kernels apply against Python's ``keep_mask``, bit for bit; and the model / trainer plumbing on a tiny Llama in bf16.

Bars of the model-level comparison with ``LoraLinear(hip=False)``: those of tests/test_gpu_backward.py for a gradient tensor (``DTYPES``,
imported)."""
import os

import pytest
import torch

import lora_cases as LC
from mraudio_amd.models import lora as L
from test_gpu_backward import DTYPES
from test_gpu_llm_objective import LH, _batch, _model, _tiny_llama

pytestmark = pytest.mark.gpu

GUARD = 64                       # elements on either side of every output (a multiple of 8: the views stay 16-byte aligned)
SENT = 77.0                      # exact in f16, bf16 and fp32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _id(dt):
    return "f16" if dt == torch.float16 else "bf16"


def _guarded(t: torch.Tensor, ld: int, dev):
    """(buffer, view): ``t`` [rows, width] copied into a sentinel-filled buffer with pitch ``ld`` and GUARD elements on either side."""
    rows, width = t.shape
    buf = torch.full((2 * GUARD + rows * ld,), SENT, dtype=t.dtype, device=dev)
    view = buf[GUARD: GUARD + rows * ld].view(rows, ld)[:, :width]
    view.copy_(t)
    assert view.data_ptr() % 16 == 0
    return buf, view


def _guards_intact(buf: torch.Tensor, rows: int, width: int, ld: int) -> bool:
    body = buf[GUARD: GUARD + rows * ld].view(rows, ld)
    return bool((buf[:GUARD] == SENT).all() and (buf[GUARD + rows * ld:] == SENT).all() and (body[:, width:] == SENT).all())


@pytest.fixture(scope="module")
def refs():
    """The float64 references and bounds of every case, computed once per (dtype, case) and shared by the three entry tests."""
    cache = {}

    def get(dtype, case):
        key = (dtype, case)
        if key not in cache:
            rows, width, R, p = case
            c = LC.make_case(rows, width, R, dtype)
            keep, iq = LC.mask(rows, width, p), LC.inv_q(p)
            cache[key] = (c, iq, LC.down_ref(c["x"], c["W"], iq, keep), LC.up_ref(c["y0"], c["u"], c["W"], iq, keep),
                          LC.wgrad_ref(c["x"], c["u"], c["dW0"], iq, keep))
        return cache[key]

    return get


# ---- per entry: every element against float64 under the derived bound ---------------------------------------------------------------------
@pytest.mark.parametrize("layout", (LC.NR, LC.RN), ids=("NR", "RN"))
@pytest.mark.parametrize("dtype", LC.DTYPES, ids=_id)
def test_down_against_float64(dev, refs, dtype, layout):
    worst = 0.0
    for case in LC.cases():
        rows, width, R, p = case
        c, iq, (ref, bound), _, _ = refs(dtype, case)
        ld = LC.pitch(rows, width, R)
        xbuf, x = _guarded(c["x"], ld, dev)
        obuf, out = _guarded(torch.full((rows, R), SENT), R, dev)
        w = LC.as_memory(c["W"], layout).to(dev)
        L.lora_down(x, w, layout, iq, p, LC.SEED, out=out)
        again = torch.full_like(out, SENT)
        L.lora_down(x, w, layout, iq, p, LC.SEED, out=again)
        r = LC.ratio(out.cpu(), ref, bound)
        worst = max(worst, r)
        assert r <= 1.0, (case, r)
        assert torch.equal(out, again), case                                   # two runs, the same bits
        assert _guards_intact(obuf, rows, R, R) and _guards_intact(xbuf, rows, width, ld), case
    print(f"lora down {_id(dtype)} layout {layout}: worst ratio to bound {worst:.3g}")
    assert worst > 0.0


@pytest.mark.parametrize("layout", (LC.NR, LC.RN), ids=("NR", "RN"))
@pytest.mark.parametrize("dtype", LC.DTYPES, ids=_id)
def test_up_add_against_float64(dev, refs, dtype, layout):
    worst = 0.0
    for case in LC.cases():
        rows, width, R, p = case
        c, iq, _, (ref, bound), _ = refs(dtype, case)
        ld = LC.pitch(rows, width, R)
        ybuf, y = _guarded(c["y0"], ld, dev)
        ubuf, u = _guarded(c["u"], R, dev)
        w = LC.as_memory(c["W"], layout).to(dev)
        L.lora_up_add(y, u, w, layout, iq, p, LC.SEED)
        r = LC.ratio(y.cpu().float(), ref, bound)
        worst = max(worst, r)
        assert r <= 1.0, (case, r)
        assert _guards_intact(ybuf, rows, width, ld) and _guards_intact(ubuf, rows, R, R), case
    print(f"lora up_add {_id(dtype)} layout {layout}: worst ratio to bound {worst:.3g}")
    assert worst > 0.0


@pytest.mark.parametrize("layout", (LC.NR, LC.RN), ids=("NR", "RN"))
@pytest.mark.parametrize("dtype", LC.DTYPES, ids=_id)
def test_wgrad_against_float64(dev, refs, dtype, layout):
    worst = 0.0
    for case in LC.cases():
        rows, width, R, p = case
        c, iq, _, _, (ref, bound) = refs(dtype, case)
        ld = LC.pitch(rows, width, R)
        xbuf, x = _guarded(c["x"], ld, dev)
        u = c["u"].to(dev)
        mem = LC.as_memory(c["dW0"], layout)                                   # the prefill, in the layout under test
        dbuf, dw = _guarded(mem, mem.shape[1], dev)
        L.lora_wgrad(x, u, dw, layout, iq, p, LC.SEED)
        _, dw2 = _guarded(mem, mem.shape[1], dev)
        L.lora_wgrad(x, u, dw2, layout, iq, p, LC.SEED)
        got = LC.from_memory(dw.cpu().contiguous(), layout, R, width)
        r = LC.ratio(got, ref, bound)
        worst = max(worst, r)
        assert r <= 1.0, (case, r)
        assert torch.equal(dw, dw2), case                                      # no atomics: two runs, the same bits
        assert _guards_intact(dbuf, mem.shape[0], mem.shape[1], mem.shape[1]) and _guards_intact(xbuf, rows, width, ld), case
    print(f"lora wgrad {_id(dtype)} layout {layout}: worst ratio to bound {worst:.3g}")
    assert worst > 0.0


def test_zero_rows_touch_nothing(dev):
    x = torch.full((4, 32), SENT, dtype=torch.bfloat16, device=dev)
    f = torch.full((32, 8), SENT, device=dev)
    u = torch.full((4, 8), SENT, device=dev)
    L.lora_down(x[:0], f, LC.NR, 1.0, 0.5, 1, out=u[:0])
    L.lora_up_add(x[:0], u[:0], f, LC.NR, 1.0, 0.5, 1)
    L.lora_wgrad(x[:0], u[:0], f, LC.NR, 1.0, 0.5, 1)
    torch.cuda.synchronize(dev)
    assert all(bool((t == SENT).all()) for t in (x, f, u))


# ---- the mask the kernels apply is Python's, bit for bit -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", LC.DTYPES, ids=_id)
@pytest.mark.parametrize("p", (0.05, 0.5))
def test_kernel_mask_is_pythons_keep(dev, dtype, p):
    for rows, width in ((67, 264), (17, 40), (1, 8)):
        ld = width + 8
        _, y = _guarded(torch.zeros(rows, width, dtype=dtype), ld, dev)
        one = torch.ones(rows, 1, device=dev)
        L.lora_up_add(y, one, torch.ones(width, 1, device=dev), LC.NR, 1.0, p, LC.SEED)          # y = keep
        keep = L.keep_mask(LC.SEED, rows, width, p)
        assert torch.equal(y.cpu() != 0, keep), (rows, width)
        # down with W = 1 counts the kept elements of a row of ones, wgrad with u = 1 those of a column: exact small integers
        x = torch.ones(rows, width, dtype=dtype, device=dev)
        cnt = L.lora_down(x, torch.ones(1, width, device=dev), LC.RN, 1.0, p, LC.SEED)
        assert torch.equal(cnt.cpu()[:, 0], keep.sum(1).float())
        col = L.lora_wgrad(x, one, torch.zeros(1, width, device=dev), LC.RN, 1.0, p, LC.SEED)
        assert torch.equal(col.cpu()[0], keep.sum(0).float())


def test_dropped_elements_keep_their_bits_and_odd_shapes_fall_back(dev):
    """A dropped element of up_add is not touched, even when the chain it would have received is not finite; and the automatic route
    (``hip=None``) runs what the entries do not take -- here a width that is no multiple of 8 -- as torch ops instead of raising."""
    rows, width, p = 17, 40, 0.5
    y0 = torch.randn(rows, width, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)
    y = y0.to(dev)
    u = torch.full((rows, 1), float("inf"), device=dev)
    L.lora_up_add(y, u, torch.ones(width, 1, device=dev), LC.NR, 1.0, p, LC.SEED)
    keep = L.keep_mask(LC.SEED, rows, width, p)
    assert torch.equal(y.cpu()[~keep], y0[~keep]) and torch.isinf(y.cpu()[keep].float()).all()
    from torch import nn
    mod = L.LoraLinear(nn.Linear(20, 24, device=dev, dtype=torch.bfloat16), r=4, dropout=0.0)
    x = torch.randn(3, 20, device=dev, dtype=torch.bfloat16)
    assert mod._use_hip(x) is False and mod(x).shape == (3, 24)
    mod.hip = True
    with pytest.raises(L.MraError, match="multiples of 8"):
        mod(x)


# ---- the model on a tiny Llama, bf16 -----------------------------------------------------------------------------------------------------------
def _randomise_B(model, seed=3):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model._lora_mods:
            B = m.lora_B["default"].weight
            B.copy_((torch.randn(B.shape, generator=g) * 0.05).to(B.device))


def _adapter_grads(model):
    return [p.grad.clone() for p in model.lora_parameters()]


def test_fresh_adapters_leave_the_loss_bit_for_bit(dev):
    llm, tok = _tiny_llama(dev)
    model = _model(dev, llm, tok)
    batch = _batch(dev)
    before = model.forward_llm(batch)["loss"]
    model.enable_lora()
    assert model.lora and len(model._lora_mods) == 14 and len(model.lora_parameters()) == 28
    for m in model._lora_mods:
        m.train()                                                              # dropout on: u changes, B = 0 adds exactly nothing
    after = model.forward_llm(batch)["loss"]
    assert torch.equal(before, after) and after.requires_grad
    assert not any(k.startswith("llm_model") for k in model.state_dict())


def test_loss_and_gradients_match_the_torch_path(dev):
    rel_tol, peak_tol = next((d[2], d[3]) for d in DTYPES if d[0] == torch.bfloat16)
    llm, tok = _tiny_llama(dev)
    model = _model(dev, llm, tok)
    batch = _batch(dev)
    model.objective = "llm"
    model.enable_lora(r=8, alpha=8, dropout=0.05)
    model.enable_qformer_training(train_proj=True)                             # dx reaches llm_proj and the Q-Formers
    _randomise_B(model)
    model.train()
    runs = {}
    for hip in (True, False):
        for m in model._lora_mods:
            m.hip = hip
        for p in model.lora_parameters() + list(model.video_llm_proj.parameters()) + list(model.audio_llm_proj.parameters()):
            p.grad = None
        for m in model.modalities:
            getattr(model, f"{m}_Qformer")._grad_flat.zero_()
        torch.manual_seed(21)                                                  # the same seeds, hence the same masks
        loss = model(batch)["loss"]
        loss.backward()
        torch.cuda.synchronize(dev)
        seeds = [m.last_seed for m in model._lora_mods]
        runs[hip] = (loss.item(), seeds, _adapter_grads(model), [model.video_llm_proj.weight.grad.clone(), model.audio_llm_proj.weight.grad.clone(),
                                                                  model.video_Qformer._grad_flat.clone(), model.audio_Qformer._grad_flat.clone()])
    assert runs[True][1] == runs[False][1] and len(set(runs[True][1])) == 14 and all(s > 0 for s in runs[True][1])
    assert abs(runs[True][0] - runs[False][0]) <= 2e-2 * abs(runs[False][0]), (runs[True][0], runs[False][0])
    worst = (0.0, 0.0)
    for got, ref in zip(runs[True][2] + runs[True][3], runs[False][2] + runs[False][3]):
        assert torch.isfinite(got).all() and ref.abs().max().item() > 0
        rel = ((got - ref).norm() / ref.norm()).item()
        peak = (got - ref).abs().max().item() / ref.abs().max().item()
        worst = (max(worst[0], rel), max(worst[1], peak))
        assert rel < rel_tol and peak < peak_tol, (rel, peak)
    print(f"lora model gradients, HIP against torch ops: worst rel {worst[0]:.3g} (bar {rel_tol}), worst peak {worst[1]:.3g} (bar {peak_tol})")


def test_frozen_qformers_three_adam_steps_lower_the_loss(dev):
    llm, tok = _tiny_llama(dev)
    model = _model(dev, llm, tok)
    batch = _batch(dev)
    model.objective = "llm"
    model.enable_lora(r=8, alpha=8, dropout=0.0)
    model.train()
    model._sync()
    frozen = {m: (None if getattr(getattr(model, f"{m}_Qformer"), "_master_flat", None) is None else getattr(model, f"{m}_Qformer")._master_flat.clone(),
                  {k: v.clone() for k, v in getattr(model, f"{m}_Qformer").state_dict().items()},
                  getattr(model, f"{m}_llm_proj").weight.detach().clone(), getattr(model, f"{m}_llm_proj").bias.detach().clone())
              for m in model.modalities}
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
    print("LM loss over three fused-Adam steps on the adapters:", losses)
    assert losses[3] < losses[0], losses
    for m in model.modalities:
        qf, (flat, sd, W, b) = getattr(model, f"{m}_Qformer"), frozen[m]
        assert (flat is None and getattr(qf, "_master_flat", None) is None) or torch.equal(qf._master_flat, flat)
        assert all(torch.equal(v, sd[k]) for k, v in qf.state_dict().items())
        assert torch.equal(getattr(model, f"{m}_llm_proj").weight, W) and torch.equal(getattr(model, f"{m}_llm_proj").bias, b)
        assert all(p.grad is None for p in getattr(model, f"{m}_llm_proj").parameters())


def test_loss_scale_is_divided_out_of_the_adapter_gradients(dev):
    llm, tok = _tiny_llama(dev)
    model = _model(dev, llm, tok)
    batch = _batch(dev)
    model.objective = "llm"
    model.enable_lora(r=8, alpha=8, dropout=0.05)
    _randomise_B(model)
    model.train()
    runs = {}
    for s in (1.0, 1024.0):
        model.loss_scale = s
        for p in model.lora_parameters():
            p.grad = None
        torch.manual_seed(5)
        loss = model(batch)["loss"]
        loss.backward()
        torch.cuda.synchronize(dev)
        runs[s] = (loss.item(), _adapter_grads(model))
    assert runs[1.0][0] == runs[1024.0][0]
    for a, b in zip(runs[1.0][1], runs[1024.0][1]):
        assert torch.isfinite(b).all() and a.norm().item() > 0 and ((a - b).norm() / a.norm()).item() < 1e-2


def test_both_objective_with_frozen_qformers(dev):
    """objective "both", LoRA on, Q-Formers frozen: the loss is bce + lm_weight * lm with the two terms reported, the scorer term carries no
    gradient, and the adapter gradients are lm_weight times those of the "llm" run under the same seeds."""
    llm, tok = _tiny_llama(dev)
    model = _model(dev, llm, tok)
    batch = _batch(dev)
    model.enable_lora(r=8, alpha=8, dropout=0.05)
    _randomise_B(model)
    model.train()
    model.lm_weight = 0.5
    runs = {}
    for obj in ("llm", "both"):
        model.objective = obj
        for p in model.lora_parameters():
            p.grad = None
        torch.manual_seed(9)
        out = model(batch)
        out["loss"].backward()
        torch.cuda.synchronize(dev)
        runs[obj] = (out, _adapter_grads(model))
    both, lm = runs["both"][0], runs["llm"][0]["loss"]
    assert set(both) == {"loss", "loss_score", "loss_lm"} and not both["loss_score"].requires_grad and not both["loss_lm"].requires_grad
    assert torch.equal(both["loss_lm"], lm.detach())
    model.objective = "score"
    with torch.no_grad():
        bce = model(batch)["loss"]
    assert torch.equal(both["loss_score"], bce)
    want = bce.item() + 0.5 * lm.item()
    assert abs(both["loss"].item() - want) <= 1e-6 * abs(want)
    for a, b in zip(runs["llm"][1], runs["both"][1]):          # the 16-bit activation gradients are halved exactly (a power of two)
        assert a.norm().item() > 0 and ((0.5 * a - b).norm() / (0.5 * a).norm()).item() < 1e-3
    assert all(p.grad is None for m in model.modalities for p in getattr(model, f"{m}_llm_proj").parameters())


def test_trainer_saves_resumes_and_generates_with_adapters(dev, tmp_path):
    from mraudio_amd.utils.trainer import Trainer, default_args

    llm, tok = _tiny_llama(dev)
    model = _model(dev, llm, tok)
    kw = dict(output_dir=str(tmp_path), gpu=0, synthetic=4, dataset="Charades_STA", lr=1e-3, warmup_steps=1, objective="llm", lora=True,
              train_qformers=False, val_freq=2)
    tr = Trainer(default_args(max_epoch=2, **kw), model=model)
    assert model.lora and not getattr(model, "train_qformers", False)
    tr.train()
    assert len(tr.history) == 2 and tr.history[1]["loss_value"] < tr.history[0]["loss_value"], tr.history
    path = os.path.join(tmp_path, "checkpoint_1.pth")
    ck = torch.load(path, weights_only=True)["model"]
    key = "llm_model.base_model.model.model.layers.0.self_attn.q_proj.lora_B.default.weight"
    assert key in ck and ck[key].abs().sum() > 0
    named = {k for k, _ in model.named_parameters()}
    assert len([k for k in ck if k.startswith("llm_model.")]) == 28 and not any(k in named for k in ck)      # nothing else trainable
    saved = {k: v.clone() for k, v in ck.items() if k.startswith("llm_model.")}
    with torch.no_grad():
        for p in model.lora_parameters():
            p.zero_()
    tr2 = Trainer(default_args(max_epoch=3, resume_ckpt_path=path, **kw), model=model)
    tr2._load_checkpoint(path)
    assert tr2.start_epoch == 2
    now = {f"llm_model.{k}": v for k, v in L.lora_state_dict(model.llm_model).items()}
    assert all(torch.equal(now[k].cpu(), v) for k, v in saved.items())
    # the same file through the model's own loader with its default (strict) flags, as evaluate --lora --checkpoint F calls it
    assert all(k.startswith("llm_model.") for k in ck)
    with torch.no_grad():
        for p in model.lora_parameters():
            p.zero_()
    msg = model.load_checkpoint(path)
    assert msg.missing_keys == [] and msg.unexpected_keys == [] and "LoRA adapters of" in model.weights_source
    now = {f"llm_model.{k}": v for k, v in L.lora_state_dict(model.llm_model).items()}
    assert all(torch.equal(now[k].cpu(), v) for k, v in saved.items())
    model.eval()
    assert not any(m.training for m in model._lora_mods)
    texts = model.generate_llm(_batch(dev), max_new_tokens=4)
    assert len(texts) == 2 and all(isinstance(t, str) for t in texts)
