"""The LM objective on the GPU (``-m gpu``): ``QFormer.llm_proj_train`` (``mra_llm_proj_backward`` behind autograd) against torch.autograd
over the CPU oracle, and the model / trainer plumbing that carries the gradient of a frozen causal LM's loss through ``{m}_llm_proj`` into
the Q-Formers: ``XInstructBLIP.objective`` "llm" / "both", ``enable_qformer_training(train_proj=True)``, ``Trainer``.

Bars of the oracle check: those of tests/test_gpu_backward.py for a gradient tensor (``DTYPES``, imported).  Two runs of one step: the rule
of tests/test_gpu_enc_grad.py (``_assert_same_step``, imported)."""
import os

import pytest
import torch

from oracle import qformer_ref as O
from test_gpu_backward import DTYPES
from test_gpu_enc_grad import _assert_same_step
from tools.make_golden import make_inputs

pytestmark = pytest.mark.gpu

LH = 256


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _tiny_llama(dev, dtype=torch.bfloat16):
    tf = pytest.importorskip("transformers")
    from mraudio_amd.models.llm_prompt import SimpleLlmTokenizer

    torch.manual_seed(0)
    tok = SimpleLlmTokenizer()
    cfg = tf.LlamaConfig(vocab_size=len(tok), hidden_size=LH, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                         num_key_value_heads=4, max_position_embeddings=4096, pad_token_id=tok.pad_token_id, bos_token_id=2, eos_token_id=2)
    llm = tf.LlamaForCausalLM(cfg).to(dev).to(dtype).eval().requires_grad_(False)
    return llm, tok


def _model(dev, llm, tok, seed=0):
    from mraudio_amd.models.xinstructblip import XInstructBLIP

    model = XInstructBLIP(seed=seed, perturb=True, device=dev, llm_hidden_size=LH, op_dtype=torch.bfloat16)
    model.attach_llm(llm, tok)
    return model


def _batch(dev, n=2, T=6):
    from mraudio_amd.utils.mr_dataset import SyntheticMRDataset, collate_fn

    ds = SyntheticMRDataset(n, T=T, seed=5, duration=2 * T)
    batch = collate_fn([ds[i] for i in range(n)])
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}


# ---- 1. the node ---------------------------------------------------------------------------------------------------------------------------
def test_llm_proj_train_is_llm_proj_and_wants_the_pushed_tensors(dev):
    from mraudio_amd._lib import MraError
    from mraudio_amd.qformer import QFormer, QFormerConfig

    qf = QFormer(QFormerConfig(enc_width=64, hidden=256, heads=4, inter=256, layers=2, vocab=16, max_pos=8, llm_hidden=LH), device=dev)
    g = torch.Generator().manual_seed(3)
    W = (torch.randn(LH, 256, generator=g) * 0.05).to(dev).requires_grad_(True)
    b = (torch.randn(LH, generator=g) * 0.1).to(dev).requires_grad_(True)
    z = torch.randn(3, 32, 256, generator=g).to(dev)
    with pytest.raises(MraError, match="not the tensor last pushed"):
        qf.llm_proj_train(z, W, b)
    qf.push("llm_proj.weight", W)
    qf.push("llm_proj.bias", b)
    for dt in (torch.float32, torch.float16):
        assert torch.equal(qf.llm_proj_train(z, W, b, dt), qf.llm_proj(z, dt))        # the same bits as the inference entry
    with torch.no_grad():
        W.mul_(1.5)
    with pytest.raises(MraError, match="changed since it was pushed"):
        qf.llm_proj_train(z, W, b)


# ---- 2. against the oracle; 3. with the projection frozen ----------------------------------------------------------------------------------
@pytest.mark.parametrize("op_dtype,fwd_tol,rel_tol,peak_tol", DTYPES, ids=["f16", "bf16"])
def test_projection_and_qformer_gradients_match_oracle_autograd(dev, op_dtype, fwd_tol, rel_tol, peak_tol):
    from mraudio_amd.qformer import QFormer, QFormerConfig

    ocfg = O.QFormerCfg(enc_width=1408, llm_hidden=LH)
    w = O.init_weights(ocfg, seed=0, perturb=True)
    qf = QFormer(QFormerConfig(enc_width=1408, llm_hidden=LH, op_dtype=op_dtype), device=dev)
    qf.load_state_dict({k: v for k, v in w.items() if k.startswith("bert.")})
    for k in ("query_tokens", "ln.weight", "ln.bias"):
        qf.push(k, w[k])
    n, L, kv = 4, 9, 40                                  # 164 chain rows: no weight gradient splits its contraction
    ids, tmask, att, feats = make_inputs(ocfg, n, L, kv, 77, True)
    enc = O.modality_layernorm(feats, w["ln.weight"], w["ln.bias"]).to(op_dtype)
    g = torch.Generator().manual_seed(5)
    G, rq = torch.randn(n, 32, LH, generator=g), torch.randn(n, 32, 768, generator=g)

    train = lambda k: k.startswith("bert.") or k in ("query_tokens", "llm_proj.weight", "llm_proj.bias")    # noqa: E731
    wl = {k: (v.clone().requires_grad_(True) if train(k) else v) for k, v in w.items()}
    h = O.qformer_forward(wl, ocfg, ids, att, wl["query_tokens"].expand(n, -1, -1), enc.float())
    ((O.llm_project(h, wl, n, 1) * G).sum() + (h[:, :32] * rq).sum()).backward()

    def step(train_proj):
        qf.enable_training()
        qf._grad_flat.zero_()
        Wp = w["llm_proj.weight"].to(dev).requires_grad_(train_proj)
        bp = w["llm_proj.bias"].to(dev).requires_grad_(train_proj)
        qf.push("llm_proj.weight", Wp)
        qf.push("llm_proj.bias", bp)
        q, _ = qf.forward_train(ids.to(dev), att.to(dev), enc.to(dev), want_cls=False)
        y = qf.llm_proj_train(q, Wp, bp)
        ((y * G.to(dev)).sum() + (q * rq.to(dev)).sum()).backward()
        torch.cuda.synchronize(dev)
        return y.detach().cpu(), Wp.grad, bp.grad, qf._grad_flat.clone()

    y, dW, db, flat = step(True)
    named = {"llm_proj.weight": dW.cpu(), "llm_proj.bias": db.cpu()}
    for k, ref in wl.items():
        if not train(k):
            continue
        got = named[k] if k in named else qf.grad_of(k).view_as(ref.grad).cpu()
        gref = ref.grad
        if k.endswith("key.bias"):          # the true gradient is 0 (softmax shift invariance): noise against the query-bias one
            scale = wl[k.replace(".key.", ".query.")].grad.norm().item()
            assert got.norm().item() < rel_tol * scale + 1e-4, (k, got.norm().item(), scale)
            continue
        if gref.abs().max().item() == 0.0:  # the text rows' feed-forward of the last layer: the loss reads query rows only
            assert "layer.11." in k and got.abs().max().item() == 0.0, k
            continue
        rel = ((got - gref).norm() / gref.norm()).item()
        peak = (got - gref).abs().max().item() / gref.abs().max().item()
        assert rel < rel_tol and peak < peak_tol, (k, rel, peak)
    # the projection frozen: no gradient for it, the Q-Former's unchanged (the rule for two runs of one step)
    _, dW0, db0, flat0 = step(False)
    assert dW0 is None and db0 is None
    _assert_same_step(qf, flat, flat0, "train_proj off")


# ---- 4. a frozen causal LM trains the Q-Formers and the projections ------------------------------------------------------------------------
def test_llm_objective_trains_through_a_frozen_llama(dev):
    llm, tok = _tiny_llama(dev)
    model = _model(dev, llm, tok)
    batch = _batch(dev)
    model.objective = "llm"
    model.enable_qformer_training(train_proj=True)
    W0 = model.video_llm_proj.weight.detach().clone()
    opt = torch.optim.Adam(model.flat_optimizer_params(), lr=1e-4, fused=True)
    losses = []
    for it in range(4):
        opt.zero_grad(set_to_none=False)
        loss = model(batch)["loss"]
        assert torch.isfinite(loss)
        losses.append(loss.item())
        if it == 3:
            break
        loss.backward()
        if it == 0:
            for m in ("video", "audio"):
                gw = getattr(model, f"{m}_llm_proj").weight.grad
                flat = getattr(model, f"{m}_Qformer")._grad_flat
                for t in (gw, getattr(model, f"{m}_llm_proj").bias.grad, flat):
                    assert t is not None and torch.isfinite(t).all() and t.abs().sum().item() > 0, m
            assert all(p.grad is None for p in llm.parameters())
        opt.step()
    print("LM loss over three fused-Adam steps:", losses)
    assert losses[3] < losses[0], losses
    # the stale-copy hook: the handle's projection is the UPDATED parameter (a fused step bumps no version counter)
    model._sync()
    W, b = model.video_llm_proj.weight.detach(), model.video_llm_proj.bias.detach()
    assert not torch.equal(W, W0)
    z = torch.randn(3, 32, 768, generator=torch.Generator().manual_seed(1)).to(dev)
    ref = torch.nn.functional.linear(z.bfloat16().float(), W.bfloat16().float(), b)
    fwd_tol = next(d[1] for d in DTYPES if d[0] == torch.bfloat16)
    assert (model.video_Qformer.llm_proj(z) - ref).abs().max().item() < fwd_tol
    stale = torch.nn.functional.linear(z.bfloat16().float(), W0.bfloat16().float(), b)
    assert (model.video_Qformer.llm_proj(z) - ref).abs().max() < (model.video_Qformer.llm_proj(z) - stale).abs().max()


# ---- 5. both objectives over one Q-Former pass; 6. the defaults are the parent's ------------------------------------------------------------
def test_both_is_the_weighted_sum_over_one_qformer_backward(dev):
    from mraudio_amd._lib import MraError

    llm, tok = _tiny_llama(dev)
    model = _model(dev, llm, tok)
    batch = _batch(dev)
    model.enable_qformer_training(train_proj=True)
    model.lm_weight = 0.5
    single = {}
    for obj in ("score", "llm"):
        model.objective = obj
        single[obj] = model(batch)["loss"].item()
    model.objective = "both"
    calls = {}
    for m in ("video", "audio"):
        qf = getattr(model, f"{m}_Qformer")
        inner = qf._run_backward

        def counted(*a, _m=m, _inner=inner, **kw):
            calls[_m] = calls.get(_m, 0) + 1
            return _inner(*a, **kw)

        qf._run_backward = counted
    out = model(batch)
    want = single["score"] + 0.5 * single["llm"]
    assert abs(out["loss"].item() - want) <= 1e-6 * abs(want), (out["loss"].item(), single)
    out["loss"].backward()
    torch.cuda.synchronize(dev)
    assert calls == {"video": 1, "audio": 1}
    grouped = dict(batch, text_input=[[t] for t in batch["text_input"]], text_output=[[t] for t in batch["text_output"]])
    with pytest.raises(MraError, match="multi-query"):
        model(grouped)
    # loss_scale: a power of two scales every gradient inside the LM exactly (no overflow at 2^10 here) and is divided out in fp32 in the
    # projection's backward -- the loss value is the same number, the gradients differ only where the unscaled run lost subnormal bits
    model.objective = "llm"
    runs = {}
    for s in (1.0, 1024.0):
        model.loss_scale = s
        model.video_llm_proj.weight.grad = None
        model.video_Qformer._grad_flat.zero_()
        loss = model(batch)["loss"]
        loss.backward()
        torch.cuda.synchronize(dev)
        runs[s] = (loss.item(), model.video_llm_proj.weight.grad.clone(), model.video_Qformer._grad_flat.clone())
    assert runs[1.0][0] == runs[1024.0][0]
    for a, b in zip(runs[1.0][1:], runs[1024.0][1:]):
        assert torch.isfinite(b).all() and ((a - b).norm() / a.norm()).item() < 1e-2

def test_defaults_give_the_parents_values(dev):
    """``objective="score"`` and ``forward_llm(samples)`` with default arguments, on a model that went through the new switches and back,
    against a model of the same seed that never saw them: the same bits."""
    llm, tok = _tiny_llama(dev)
    plain, touched = _model(dev, llm, tok), _model(dev, llm, tok)
    batch = _batch(dev)
    plain.enable_qformer_training()
    touched.enable_qformer_training(train_ln=False, train_proj=False)
    touched.objective = "both"
    touched(batch)
    touched.objective = "score"
    assert torch.equal(plain(batch)["loss"], touched(batch)["loss"])
    a, b = plain.forward_llm(batch)["loss"], touched.forward_llm(batch)["loss"]
    assert torch.equal(a, b) and not a.requires_grad and not b.requires_grad
    assert not plain.video_llm_proj.weight.requires_grad and not touched.video_llm_proj.weight.requires_grad
    from mraudio_amd._lib import MraError
    from mraudio_amd.models.xinstructblip import XInstructBLIP
    bare = XInstructBLIP(seed=0, device=dev, llm_hidden_size=LH, modalities=["audio"], op_dtype=torch.bfloat16)
    bare.enable_qformer_training()
    with pytest.raises(MraError, match="no LLM attached"):
        bare.forward_llm(batch, train=True)


# ---- 7. the trainer ------------------------------------------------------------------------------------------------------------------------
def test_trainer_with_both_objectives_saves_and_restores_the_projection(dev, tmp_path):
    from mraudio_amd.utils.trainer import Trainer, default_args

    llm, tok = _tiny_llama(dev)
    model = _model(dev, llm, tok)
    init = model.video_llm_proj.weight.detach().cpu().clone()
    kw = dict(output_dir=str(tmp_path), gpu=0, synthetic=4, dataset="Charades_STA", lr=2e-5, warmup_steps=1, objective="both", train_proj=True,
              val_freq=2)                                   # (validation, which stays on the scorer, after epoch 0 only)
    tr = Trainer(default_args(max_epoch=2, **kw), model=model)
    assert model.objective == "both" and model.train_proj
    tr.train()
    assert len(tr.history) == 2 and tr.history[1]["loss_value"] < tr.history[0]["loss_value"], tr.history
    path = os.path.join(tmp_path, "checkpoint_1.pth")
    ck = torch.load(path, weights_only=True)
    saved = ck["model"]["video_llm_proj.weight"]
    assert "audio_llm_proj.bias" in ck["model"] and not torch.equal(saved, init)
    assert not any(k.startswith("llm_model") for k in ck["model"])
    with torch.no_grad():                                   # a resume puts the trained projection back
        model.video_llm_proj.weight.copy_(init)
    tr2 = Trainer(default_args(max_epoch=3, resume_ckpt_path=path, **kw), model=model)
    tr2._load_checkpoint(path)
    assert tr2.start_epoch == 2 and torch.equal(model.video_llm_proj.weight.detach().cpu(), saved)
