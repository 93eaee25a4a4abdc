"""The LM prefill's host side without a GPU (``-m "not gpu"``): ``register(prefill=True)`` / ``hip_decode(llm, prefill=True)`` of
``mraudio_amd/models/lm_decode.py`` on fp32 CPU Llamas (the torch-op route of ``prefill_attention``) against the stock implementation -- a
prefill over a ``DynamicCache``, a whole ``generate`` over a static cache, a continuation call that must fall back to SDPA under the full mask --
the mask builder, ``HipLmDecoder(prefill=)``, the model's and the trainer's ``lm_prefill`` switch and the command-line flags."""
import pytest
import torch
from torch import nn

from mraudio_amd import _lib
from mraudio_amd.models import lm_decode as LD
from mraudio_amd.models import lm_step as LS
from test_lm_decode_cpu import LAYERS, LH, SAMPLES, _stub, _tiny_llama, _trainer

S0 = 40


def _llama(kv_heads):
    tf = pytest.importorskip("transformers")
    torch.manual_seed(3)
    cfg = tf.LlamaConfig(vocab_size=64, hidden_size=256, intermediate_size=128, num_hidden_layers=LAYERS, num_attention_heads=4,
                         num_key_value_heads=kv_heads, max_position_embeddings=512, pad_token_id=0, bos_token_id=2, eos_token_id=2)
    return tf.LlamaForCausalLM(cfg).eval().requires_grad_(False)          # head_dim 64, 4 query heads over 4 or 2 K/V heads


def _prefix(hidden=256):
    """B = 3 prefixes of 40 rows: left padding in one sequence, holes inside another, each under a fifth of the sequence."""
    gen = torch.Generator().manual_seed(6)
    embeds = torch.randn(3, S0, hidden, generator=gen)
    mask = torch.ones(3, S0, dtype=torch.long)
    mask[1, :7] = 0
    mask[2, 5:8] = 0
    mask[2, 21:25] = 0
    assert int((mask == 0).sum(1).max()) < S0 // 5
    return embeds, mask


def _positions(mask):
    pos = mask.long().cumsum(-1) - 1
    return pos.masked_fill(mask == 0, 1)


def _spies(monkeypatch):
    import transformers.integrations.sdpa_attention as SA

    pre, sdpa = [], []
    real_pre, real_sdpa = LD.prefill_attention, SA.sdpa_attention_forward
    monkeypatch.setattr(LD, "prefill_attention", lambda q, k, v, m, *a, **kw: pre.append((tuple(q.shape), tuple(k.shape), tuple(m.shape), m.dtype))
                        or real_pre(q, k, v, m, *a, **kw))
    monkeypatch.setattr(SA, "sdpa_attention_forward",
                        lambda module, query, key, value, attention_mask, **kw: sdpa.append((query.shape[2], None if attention_mask is None else tuple(attention_mask.shape)))
                        or real_sdpa(module, query, key, value, attention_mask, **kw))
    return pre, sdpa


def test_register_prefill_is_idempotent_and_leaves_the_decode_name_alone():
    from transformers import AttentionInterface
    from transformers.masking_utils import AttentionMaskInterface, sdpa_mask

    assert LD.register(prefill=True) == "mra_prefill" == LD.register(prefill=True) == LD.PREFILL_NAME
    assert AttentionInterface._global_mapping["mra_prefill"] is LD.prefill_attention_forward
    assert AttentionMaskInterface._global_mapping["mra_prefill"] is LD.prefill_mask
    assert LD.register() == "mra_decode"
    assert AttentionInterface._global_mapping["mra_decode"] is LD.attention_forward and AttentionMaskInterface._global_mapping["mra_decode"] is sdpa_mask


def test_mask_builder_hands_a_first_prefill_the_key_mask_alone():
    from transformers.masking_utils import causal_mask_function, sdpa_mask

    pad = torch.ones(2, 6, dtype=torch.bool)
    pad[1, :2] = False
    m = LD.prefill_mask(batch_size=2, q_length=6, kv_length=6, q_offset=0, kv_offset=0, mask_function=causal_mask_function, attention_mask=pad,
                        allow_is_causal_skip=True, dtype=torch.float32, config=None, use_vmap=False, device="cpu")
    assert m.dtype == torch.bool and tuple(m.shape) == (2, 1, 1, 6) and torch.equal(m[:, 0, 0], pad)
    # a static cache: kv_length beyond the padding mask's end is the unwritten tail
    m = LD.prefill_mask(batch_size=2, q_length=6, kv_length=9, q_offset=torch.tensor(0), mask_function=causal_mask_function, attention_mask=pad, device="cpu")
    assert tuple(m.shape) == (2, 1, 1, 9) and torch.equal(m[:, 0, 0, :6], pad) and not m[..., 6:].any()
    m = LD.prefill_mask(batch_size=2, q_length=6, kv_length=6, mask_function=causal_mask_function, attention_mask=None, device="cpu")
    assert tuple(m.shape) == (2, 1, 1, 6) and m.all()
    # everything else is sdpa_mask's answer
    for kw in (dict(q_length=1, kv_length=7, q_offset=6), dict(q_length=3, kv_length=9, q_offset=6), dict(q_length=6, kv_length=6, q_offset=0, local_size=3)):
        padk = torch.ones(2, kw["kv_length"], dtype=torch.bool)
        padk[1, :2] = False
        got = LD.prefill_mask(batch_size=2, mask_function=causal_mask_function, attention_mask=padk, allow_is_causal_skip=False, device="cpu", **kw)
        want = sdpa_mask(batch_size=2, mask_function=causal_mask_function, attention_mask=padk, allow_is_causal_skip=False, device="cpu", **kw)
        assert torch.equal(got, want) and got.shape[2] == kw["q_length"]
    other = lambda b, h, q, k: k <= q                                                                  # noqa: E731  (not THE causal function)
    got = LD.prefill_mask(batch_size=2, q_length=6, kv_length=6, mask_function=other, attention_mask=pad, allow_is_causal_skip=False, device="cpu")
    assert tuple(got.shape) == (2, 1, 6, 6)


@pytest.mark.parametrize("kv_heads", [4, 2])
def test_prefill_over_a_dynamic_cache_agrees_with_the_stock_implementation(monkeypatch, kv_heads):
    llm = _llama(kv_heads)
    embeds, mask = _prefix()
    kw = dict(inputs_embeds=embeds, attention_mask=mask, position_ids=_positions(mask), use_cache=True, return_dict=True, logits_to_keep=1)
    before, state = llm.config._attn_implementation, {k: v.clone() for k, v in llm.state_dict().items()}
    want = llm(**kw)
    pre, sdpa = _spies(monkeypatch)
    with LD.hip_decode(llm, prefill=True):
        assert llm.config._attn_implementation == "mra_prefill"
        got = llm(**kw)
    assert llm.config._attn_implementation == before and all(torch.equal(v, llm.state_dict()[k]) for k, v in state.items())
    assert pre == [((3, 4, S0, 64), (3, kv_heads, S0, 64), (3, 1, 1, S0), torch.bool)] * LAYERS and not sdpa      # no [S, S] tensor on this route
    assert (got.logits[:, -1] - want.logits[:, -1]).abs().max().item() <= 1e-5
    keep = mask.bool()[:, None, :, None]
    for a, b in zip(got.past_key_values.layers, want.past_key_values.layers):
        for x, y in ((a.keys, b.keys), (a.values, b.values)):
            assert x.shape == y.shape == (3, kv_heads, S0, 64)
            assert ((x - y) * keep).abs().max().item() <= 1e-5                              # pad positions are left out: nothing attends them


@pytest.mark.parametrize("kv_heads", [4, 2])
def test_generate_over_a_static_cache_agrees_with_the_stock_implementation(monkeypatch, kv_heads):
    llm = _llama(kv_heads)
    embeds, mask = _prefix()
    n_new = 7
    kw = dict(inputs_embeds=embeds, attention_mask=mask, max_new_tokens=n_new, min_new_tokens=n_new, do_sample=False, output_logits=True,
              return_dict_in_generate=True)
    before, state = llm.config._attn_implementation, {k: v.clone() for k, v in llm.state_dict().items()}
    want = llm.generate(**kw)
    pre, sdpa = _spies(monkeypatch)
    one = []
    real_decode = LD.decode_attention
    monkeypatch.setattr(LD, "decode_attention", lambda *a, **k: one.append(a[1].shape[2]) or real_decode(*a, **k))
    with LD.hip_decode(llm, prefill=True):
        got = llm.generate(cache_implementation="static", disable_compile=True, **kw)
    assert llm.config._attn_implementation == before and all(torch.equal(v, llm.state_dict()[k]) for k, v in state.items())
    # the prefill: once per layer over the WHOLE static cache (Skv = Smax > Sq: causality and the padded key mask hide the unwritten tail)
    assert len(pre) == LAYERS and all(p[0] == (3, 4, S0, 64) and p[1][2] >= S0 + n_new - 1 and p[2] == (3, 1, 1, p[1][2]) for p in pre)
    assert len(one) == LAYERS * (n_new - 1) and not sdpa
    assert torch.equal(got.sequences, want.sequences)
    for a, b in zip(got.logits, want.logits):
        assert (a - b).abs().max().item() <= 1e-5


@pytest.mark.parametrize("kv_heads", [4, 2])
def test_a_continuation_call_falls_back_to_sdpa_under_the_full_mask(monkeypatch, kv_heads):
    from transformers import DynamicCache

    llm = _llama(kv_heads)
    embeds, mask = _prefix()
    cut = 28                                                                               # 28 rows first, then 12 more: 1 < Sq < Skv
    pos = _positions(mask)

    def two_calls():
        cache = DynamicCache(config=llm.config)
        llm(inputs_embeds=embeds[:, :cut], attention_mask=mask[:, :cut], position_ids=pos[:, :cut], past_key_values=cache, use_cache=True)
        return llm(inputs_embeds=embeds[:, cut:], attention_mask=mask, position_ids=pos[:, cut:], past_key_values=cache, use_cache=True, return_dict=True)

    want = two_calls()
    pre, sdpa = _spies(monkeypatch)
    with LD.hip_decode(llm, prefill=True):
        got = two_calls()
    assert len(pre) == LAYERS and all(p[0][2] == cut for p in pre)                         # the first call is a first prefill
    assert sdpa == [(S0 - cut, (3, 1, S0 - cut, S0))] * LAYERS                             # the second: SDPA under the [Sq, Skv] mask
    assert (got.logits[:, -1] - want.logits[:, -1]).abs().max().item() <= 1e-5
    keep = mask.bool()[:, None, :, None]
    for a, b in zip(got.past_key_values.layers, want.past_key_values.layers):
        assert ((a.keys - b.keys) * keep).abs().max().item() <= 1e-5 and ((a.values - b.values) * keep).abs().max().item() <= 1e-5


def test_a_key_mask_call_that_is_not_accepted_goes_to_sdpa_under_the_full_causal_mask(monkeypatch):
    import transformers.integrations.sdpa_attention as SA

    seen = []
    monkeypatch.setattr(SA, "sdpa_attention_forward", lambda module, q, k, v, m, **kw: seen.append((m, kw)) or ("sdpa", None))
    mod = nn.Module().eval()
    q, k = torch.randn(2, 4, 5, 64), torch.randn(2, 2, 9, 64)
    key = torch.ones(2, 1, 1, 9, dtype=torch.bool)
    key[1, ..., :2] = False
    out, _ = LD.prefill_attention_forward(mod, q, k, k, key, scaling=0.125)
    assert tuple(out.shape) == (2, 5, 4, 64) and not seen                                  # [B, Sq, Hq, D]: no transpose afterwards
    want = key & (torch.arange(9)[None, :] <= torch.arange(5)[:, None])[None, None]
    for kw, qq, kk in ((dict(dropout=0.1), q, k), (dict(sliding_window=4), q, k), (dict(softcap=30.0), q, k), (dict(), q[..., :32], k[..., :32]),
                       (dict(), torch.randn(2, 6, 5, 64), k)):
        assert LD.prefill_attention_forward(mod, qq, kk, kk, key, scaling=0.125, **kw) == ("sdpa", None)
        m, got_kw = seen.pop()
        assert m.dtype == torch.bool and tuple(m.shape) == (2, 1, 5, 9) and torch.equal(m, want.expand(2, 1, 5, 9))
        assert got_kw == dict(dropout=kw.get("dropout", 0.0), scaling=0.125, **{a: b for a, b in kw.items() if a != "dropout"})
    mod.train()
    assert LD.prefill_attention_forward(mod, q, k, k, key, scaling=0.125) == ("sdpa", None) and tuple(seen.pop()[0].shape) == (2, 1, 5, 9)
    # a full [Sq, Skv] mask or a one-token call is attention_forward's business, arguments untouched
    mod.eval()
    full = want.expand(2, 1, 5, 9).clone()
    assert LD.prefill_attention_forward(mod, q, k, k, full, scaling=0.125) == ("sdpa", None) and seen.pop()[0] is full
    assert tuple(LD.prefill_attention_forward(mod, q[:, :, :1], k, k, key, scaling=0.125)[0].shape) == (2, 1, 4, 64) and not seen


# ---- HipLmDecoder, the model's switch, the trainer and the flags ------------------------------------------------------------------------------
def test_hip_lm_decoder_ref_with_a_hip_prefill_gives_the_stock_prefills_tokens(monkeypatch):
    llm = _tiny_llama(kv_heads=1)
    gen = torch.Generator().manual_seed(6)
    embeds = torch.randn(3, 20, LH, generator=gen)
    mask = torch.ones(3, 20, dtype=torch.long)
    mask[1, :4] = 0
    mask[2, 5:8] = 0
    before = llm.config._attn_implementation
    stock = LS.HipLmDecoder(llm, ref=True, prefill="stock").generate(embeds, mask, 9, ignore_eos=True)
    pre, _ = _spies(monkeypatch)
    hip = LS.HipLmDecoder(llm, ref=True, prefill="hip").generate(embeds, mask, 9, ignore_eos=True)
    assert len(pre) == LAYERS and torch.equal(hip, stock) and llm.config._attn_implementation == before
    assert LS.HipLmDecoder(llm, ref=True).prefill == "stock"
    with pytest.raises(ValueError, match="prefill"):
        LS.HipLmDecoder(llm, ref=True, prefill="fast")
    # the implementation is put back after an exception inside the prefill
    monkeypatch.setattr(LD, "prefill_attention", lambda *a, **k: (_ for _ in ()).throw(RuntimeError("inside the prefill")))
    with pytest.raises(RuntimeError, match="inside the prefill"):
        LS.HipLmDecoder(llm, ref=True, prefill="hip").generate(embeds, mask, 2)
    assert llm.config._attn_implementation == before


def test_constructor_and_decode_refuse_a_hip_prefill_without_a_hip_decode():
    from mraudio_amd.models.xinstructblip import XInstructBLIP

    with pytest.raises(ValueError, match="lm_prefill='hip' needs lm_decode"):
        XInstructBLIP(lm_prefill="hip", lm_decode="stock")
    with pytest.raises(ValueError, match="lm_prefill must be"):
        XInstructBLIP(lm_prefill="bogus")
    with pytest.raises(ValueError, match="lm_prefill must be"):
        XInstructBLIP(lm_prefill="bogus", lm_decode="hip_step")
    assert XInstructBLIP.lm_prefill == "stock"


def test_lm_prefill_hip_reaches_the_prefill_of_the_hip_decode(monkeypatch):
    stub = _stub()
    llm = stub.llm_model
    stock = stub.generate_llm(SAMPLES, max_new_tokens=12)
    before = llm.config._attn_implementation
    pre, _ = _spies(monkeypatch)
    stub.lm_decode = "hip"
    assert stub.generate_llm(SAMPLES, max_new_tokens=12) == stock and not pre              # the default prefill is the stock one
    stub.lm_prefill = "hip"
    assert stub.generate_llm(SAMPLES, max_new_tokens=12) == stock and len(pre) == LAYERS and llm.config._attn_implementation == before
    stub.lm_decode = "stock"
    with pytest.raises(ValueError, match="lm_prefill='hip' needs lm_decode"):
        stub.generate_llm(SAMPLES, max_new_tokens=12)
    stub.lm_prefill = "stock"
    assert stub.generate_llm(SAMPLES, max_new_tokens=12) == stock and len(pre) == LAYERS


def test_trainer_passes_lm_prefill_on(tmp_path):
    from mraudio_amd.utils.trainer import default_args

    assert default_args().lm_prefill == "stock"
    stub = _stub()
    _trainer(tmp_path, stub, val_decode="llm", lm_decode="hip", lm_prefill="hip")
    assert stub.lm_decode == "hip" and stub.lm_prefill == "hip"
    stub2 = _stub()
    _trainer(tmp_path, stub2, val_decode="llm", lm_decode="hip")
    assert getattr(stub2, "lm_prefill", "stock") == "stock"
    with pytest.raises(ValueError, match="lm_prefill='hip' needs lm_decode"):
        _trainer(tmp_path, _stub(), val_decode="llm", lm_prefill="hip")
    with pytest.raises(ValueError, match="lm_prefill must be"):
        _trainer(tmp_path, _stub(), val_decode="llm", lm_decode="hip", lm_prefill="bogus")


def test_cli_flags_parse_and_default(capsys):
    from mraudio_amd import evaluate, finetune

    ap, base = finetune.build_parser(), ["--output-dir", "out", "--dataset", "QVH"]
    assert ap.parse_args(base).lm_prefill == "stock"
    args = ap.parse_args(base + ["--val-decode", "llm", "--lm-decode", "hip_step", "--lm-prefill", "hip"])
    assert args.lm_decode == "hip_step" and args.lm_prefill == "hip"
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--lm-prefill", "fast"])
    ep = evaluate.build_parser()
    flags = {a.dest: a for a in ep._actions}
    assert flags["lm_prefill"].default == "stock" and tuple(flags["lm_prefill"].choices) == ("stock", "hip")
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--output-file", "out.json", "--lm-prefill", "hip"])
    assert e.value.code == 2 and "--lm-prefill hip needs --llm-path" in capsys.readouterr().err
