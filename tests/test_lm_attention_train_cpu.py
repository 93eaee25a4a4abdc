"""The LM's training attention without a GPU (``-m "not gpu"``): ``register_train`` / ``hip_train`` of ``mraudio_amd/models/lm_attention.py``
on fp32 CPU Llamas (the torch-op route of ``causal_attention`` under autograd) against the stock implementation -- the loss and every
gradient, in train and in eval mode -- a call with dropout, which must fall through to SDPA under the full mask, and the model's, the
trainer's and the command line's ``lm_attention`` switch."""
import pytest
import torch

from mraudio_amd import _lib
from mraudio_amd.models import lm_attention as LA
from mraudio_amd.models import lm_decode as LD
from test_lm_decode_cpu import _stub, _trainer
from test_lm_prefill_cpu import LAYERS, S0, _llama, _positions, _prefix


def _labels(mask):
    gen = torch.Generator().manual_seed(9)
    lab = torch.randint(3, 64, mask.shape, generator=gen)
    lab[:, :S0 - 9] = -100                                         # the answer: the last rows
    return lab.masked_fill(mask == 0, -100)


def _step(llm, embeds, mask):
    x = embeds.clone().requires_grad_(True)
    for p in llm.parameters():
        p.grad = None
    loss = llm(inputs_embeds=x, attention_mask=mask, position_ids=_positions(mask), labels=_labels(mask), return_dict=True).loss
    loss.backward()
    return loss.detach(), x.grad, {n: p.grad.clone() for n, p in llm.named_parameters() if p.grad is not None}


def test_register_train_is_idempotent_and_leaves_the_other_names_alone():
    from transformers import AttentionInterface
    from transformers.masking_utils import AttentionMaskInterface

    assert LA.register_train() == "mra_train" == LA.register_train() == LA.TRAIN_NAME
    assert AttentionInterface._global_mapping["mra_train"] is LA.train_attention_forward
    assert AttentionMaskInterface._global_mapping["mra_train"] is LD.prefill_mask
    assert LD.register(prefill=True) == "mra_prefill" and AttentionInterface._global_mapping["mra_prefill"] is LD.prefill_attention_forward
    assert LD.register() == "mra_decode" and AttentionInterface._global_mapping["mra_decode"] is LD.attention_forward


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("kv_heads", [4, 2])
def test_loss_and_every_gradient_agree_with_the_stock_implementation(monkeypatch, kv_heads, training):
    import transformers.integrations.sdpa_attention as SA

    llm = _llama(kv_heads).requires_grad_(True).train(training)
    embeds, mask = _prefix()
    before, state = llm.config._attn_implementation, {k: v.clone() for k, v in llm.state_dict().items()}
    want = _step(llm, embeds, mask)
    routed, sdpa = [], []
    real, real_sdpa = LA.causal_attention, SA.sdpa_attention_forward
    monkeypatch.setattr(LA, "causal_attention", lambda q, k, v, m, *a, **kw: routed.append((tuple(q.shape), tuple(k.shape), tuple(m.shape), m.dtype))
                        or real(q, k, v, m, *a, **kw))
    monkeypatch.setattr(SA, "sdpa_attention_forward", lambda *a, **kw: sdpa.append(1) or real_sdpa(*a, **kw))
    with LA.hip_train(llm):
        assert llm.config._attn_implementation == "mra_train"
        got = _step(llm, embeds, mask)
    assert llm.config._attn_implementation == before and llm.training == training
    assert all(torch.equal(v, llm.state_dict()[k]) for k, v in state.items())
    assert routed == [((3, 4, S0, 64), (3, kv_heads, S0, 64), (3, 1, 1, S0), torch.bool)] * LAYERS and not sdpa     # no [S, S] tensor on this route
    assert abs(got[0].item() - want[0].item()) <= 1e-5
    keep = mask.bool()[:, :, None]
    assert ((got[1] - want[1]) * keep).abs().max().item() <= 1e-5 and bool(torch.isfinite(got[1]).all())       # pad rows: nothing attends them
    unused = {n for n, _ in llm.named_parameters()} - set(want[2])
    assert set(got[2]) == set(want[2]) and unused == {"model.embed_tokens.weight"} and all(v.abs().max() > 0 for v in want[2].values())
    for name, g in got[2].items():
        assert (g - want[2][name]).abs().max().item() <= 1e-5, name


def test_a_call_with_dropout_falls_through_to_sdpa_under_the_full_mask(monkeypatch):
    import transformers.integrations.sdpa_attention as SA

    llm = _llama(2).train()
    llm.config.attention_dropout = 0.25
    for layer in llm.model.layers:
        layer.self_attn.attention_dropout = 0.25
    embeds, mask = _prefix()
    routed, sdpa = [], []
    real, real_sdpa = LA.causal_attention, SA.sdpa_attention_forward
    monkeypatch.setattr(LA, "causal_attention", lambda *a, **kw: routed.append(1) or real(*a, **kw))
    monkeypatch.setattr(SA, "sdpa_attention_forward",
                        lambda module, query, key, value, attention_mask, **kw: sdpa.append((tuple(attention_mask.shape), kw.get("dropout")))
                        or real_sdpa(module, query, key, value, attention_mask, **kw))
    with torch.no_grad(), LA.hip_train(llm):
        llm(inputs_embeds=embeds, attention_mask=mask, position_ids=_positions(mask), return_dict=True)
    assert not routed and sdpa == [((3, 1, S0, S0), 0.25)] * LAYERS                  # the causal mask was rebuilt from the key mask
    llm.eval()
    with torch.no_grad(), LA.hip_train(llm):                                         # an evaluating module has no dropout: the HIP route's call
        llm(inputs_embeds=embeds, attention_mask=mask, position_ids=_positions(mask), return_dict=True)
    assert len(routed) == LAYERS and len(sdpa) == LAYERS


def test_hip_train_puts_the_implementation_back_after_an_exception():
    llm = _llama(4)
    before = llm.config._attn_implementation
    with pytest.raises(RuntimeError, match="boom"):
        with LA.hip_train(llm):
            raise RuntimeError("boom")
    assert llm.config._attn_implementation == before


# ---- the switch -------------------------------------------------------------------------------------------------------------------------------
class _Ce:
    """The part of XInstructBLIP that ``_lm_ce`` touches."""
    from mraudio_amd.models.xinstructblip import XInstructBLIP as _X

    lm_loss = "stock"
    _lm_ce = _X._lm_ce

    def __init__(self, llm, lm_attention=None):
        self.llm_model = llm
        if lm_attention is not None:
            self.lm_attention = lm_attention


def test_model_option_accepts_its_two_values_and_refuses_a_third():
    import inspect

    from mraudio_amd.models.xinstructblip import LM_ATTENTIONS, XInstructBLIP

    assert LM_ATTENTIONS == ("stock", "hip") and XInstructBLIP.lm_attention == "stock"
    assert inspect.signature(XInstructBLIP.__init__).parameters["lm_attention"].default == "stock"
    with pytest.raises(ValueError, match="lm_attention must be 'stock' or 'hip', got 'bogus'"):
        XInstructBLIP(lm_attention="bogus")
    with pytest.raises(ValueError, match="lm_prefill='hip' needs lm_decode"):         # independent of the pair: its rule is untouched
        XInstructBLIP(lm_attention="hip", lm_prefill="hip")
    llm = _llama(2)
    with pytest.raises(_lib.MraError, match="lm_attention must be"):
        _Ce(llm, "fast")._lm_ce(*_prefix(), _labels(_prefix()[1]))


@pytest.mark.parametrize("lm_loss", ["stock", "rows"])
def test_lm_ce_default_is_the_call_as_it_was_and_hip_runs_inside_hip_train(monkeypatch, lm_loss):
    llm = _llama(2)
    embeds, mask = _prefix()
    targets = _labels(mask)
    with torch.no_grad():
        before = llm(inputs_embeds=embeds, attention_mask=mask, return_dict=True, labels=targets).loss     # the call before the option existed
    routed = []
    real = LA.causal_attention
    monkeypatch.setattr(LA, "causal_attention", lambda *a, **kw: routed.append(1) or real(*a, **kw))
    for model in (_Ce(llm), _Ce(llm, "stock")):
        model.lm_loss = lm_loss
        with torch.no_grad():
            got = model._lm_ce(embeds, mask, targets)
        assert not routed
        if lm_loss == "stock":
            assert torch.equal(got, before)                                             # bit for bit
    model = _Ce(llm, "hip")
    model.lm_loss = lm_loss
    impl = llm.config._attn_implementation
    with torch.no_grad():
        hip = model._lm_ce(embeds, mask, targets)
    assert len(routed) == LAYERS and llm.config._attn_implementation == impl
    assert abs(hip.item() - before.item()) <= 1e-5
    with torch.no_grad():
        assert torch.equal(_Ce(llm)._lm_ce(embeds, mask, targets), before)             # a following stock call: the bits of the one before


def test_trainer_and_command_line_pass_lm_attention_on(tmp_path):
    from mraudio_amd import finetune
    from mraudio_amd.utils.trainer import default_args

    assert default_args().lm_attention == "stock"
    stub = _stub()
    _trainer(tmp_path, stub, objective="llm", lm_attention="hip")
    assert stub.lm_attention == "hip"
    stub2 = _stub()
    _trainer(tmp_path, stub2, objective="llm")
    assert getattr(stub2, "lm_attention", "stock") == "stock"
    with pytest.raises(ValueError, match="lm_attention must be"):
        _trainer(tmp_path, _stub(), objective="llm", lm_attention="bogus")
    with pytest.raises(ValueError, match="needs objective"):
        _trainer(tmp_path, _stub(), lm_attention="hip")
    ap, base = finetune.build_parser(), ["--output-dir", "out", "--dataset", "QVH"]
    assert ap.parse_args(base).lm_attention == "stock"
    assert ap.parse_args(base + ["--objective", "llm", "--lm-attention", "hip"]).lm_attention == "hip"
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--lm-attention", "fast"])
    flags = {a.dest: a for a in ap._actions}
    assert flags["lm_attention"].default == "stock" and tuple(flags["lm_attention"].choices) == ("stock", "hip")


@pytest.mark.parametrize("reentrant", [True, False], ids=["reentrant", "non_reentrant"])
def test_activation_checkpointing_recomputes_under_the_same_attention(monkeypatch, reentrant):
    """``_lm_ce`` leaves ``hip_train`` before ``backward()``; the layers a checkpoint recomputes hold the key mask alone, which SDPA would
    read as non-causal.  ``hold_for_backward`` puts the training attention back for the pass and the stock name back at its end."""
    import transformers.integrations.sdpa_attention as SA

    llm = _llama(2).requires_grad_(True).train()
    embeds, mask = _prefix()
    targets = _labels(mask)

    def step(model):
        x = embeds.clone().requires_grad_(True)
        for p in llm.parameters():
            p.grad = None
        loss = model._lm_ce(x, mask, targets)
        loss.backward()
        return loss.detach(), x.grad, {n: p.grad.clone() for n, p in llm.named_parameters() if p.grad is not None}

    want = step(_Ce(llm))                                                            # stock, no checkpointing
    llm.gradient_checkpointing_enable(gradient_checkpointing_kwargs={"use_reentrant": reentrant})
    assert llm.is_gradient_checkpointing
    impl = llm.config._attn_implementation
    routed, sdpa = [], []
    real, real_sdpa = LA.causal_attention, SA.sdpa_attention_forward
    monkeypatch.setattr(LA, "causal_attention", lambda *a, **kw: routed.append(torch.is_grad_enabled()) or real(*a, **kw))
    monkeypatch.setattr(SA, "sdpa_attention_forward", lambda *a, **kw: sdpa.append(1) or real_sdpa(*a, **kw))
    got = step(_Ce(llm, "hip"))
    assert llm.config._attn_implementation == impl and not sdpa                     # back where it was once the pass has ended
    assert len(routed) == 2 * LAYERS and sum(routed) >= LAYERS                      # every layer ran it twice: the forward and the recomputation
    assert abs(got[0].item() - want[0].item()) <= 1e-5
    assert ((got[1] - want[1]) * mask.bool()[:, :, None]).abs().max().item() <= 1e-5
    assert set(got[2]) == set(want[2])
    for name, g in got[2].items():
        assert (g - want[2][name]).abs().max().item() <= 1e-5, name
    with torch.no_grad():                                                            # no gradient wanted: nothing is held, nothing is left behind
        assert not _Ce(llm, "hip")._lm_ce(embeds, mask, targets).requires_grad
    assert llm.config._attn_implementation == impl
    assert LA.hold_for_backward(_llama(2), got[0].clone().requires_grad_(True)).grad_fn is None      # no checkpointing: the loss itself
