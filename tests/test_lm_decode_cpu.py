"""The LM decode's host side without a GPU (``-m "not gpu"``): ``register`` / ``hip_decode`` of ``mraudio_amd/models/lm_decode.py`` on a CPU
Llama (static cache, ``disable_compile``, the torch-op route: the tokens of the default ``generate``), the model's ``lm_decode`` switch and the
trainer's ``val_decode`` on a stand-in (the model itself needs a GPU), and the command-line flags."""
import pytest
import torch
from torch import nn

from mraudio_amd import _lib
from mraudio_amd.models import lm_decode as LD

LH, HEADS, LAYERS, Q, T = 128, 2, 2, 4, 3        # head_dim 64: a shape the one-token route accepts


def _tiny_llama(vocab=64, kv_heads=1):
    tf = pytest.importorskip("transformers")
    torch.manual_seed(0)
    cfg = tf.LlamaConfig(vocab_size=vocab, hidden_size=LH, intermediate_size=128, num_hidden_layers=LAYERS, num_attention_heads=HEADS,
                         num_key_value_heads=kv_heads, max_position_embeddings=512, pad_token_id=0, bos_token_id=2, eos_token_id=2)
    return tf.LlamaForCausalLM(cfg).eval().requires_grad_(False)


def _prefix(B=3, S=20):
    gen = torch.Generator().manual_seed(6)
    embeds = torch.randn(B, S, LH, generator=gen)
    mask = torch.ones(B, S, dtype=torch.long)
    mask[1, :4] = 0                                # left padding
    mask[2, 5:8] = 0                               # padding inside the prefix
    return embeds, mask


# ---- register / hip_decode --------------------------------------------------------------------------------------------------------------------
def test_register_is_idempotent():
    from transformers import AttentionInterface
    from transformers.masking_utils import AttentionMaskInterface, sdpa_mask

    assert LD.register() == "mra_decode" and LD.register() == "mra_decode"
    assert AttentionInterface._global_mapping["mra_decode"] is LD.attention_forward
    assert AttentionMaskInterface._global_mapping["mra_decode"] is sdpa_mask


@pytest.mark.parametrize("kv_heads", [2, 1])
def test_hip_decode_on_a_cpu_llama_gives_the_default_tokens(monkeypatch, kv_heads):
    import transformers.integrations.sdpa_attention as SA

    llm = _tiny_llama(kv_heads=kv_heads)
    embeds, mask = _prefix()
    n_new = 9
    kw = dict(inputs_embeds=embeds, attention_mask=mask, max_new_tokens=n_new, min_new_tokens=n_new, do_sample=False)
    stock = llm.generate(**kw)
    before = llm.config._attn_implementation
    one, many = [], []
    real_decode, real_sdpa = LD.decode_attention, SA.sdpa_attention_forward

    def spy_decode(q, k, v, m, scale, hip=None):
        one.append((tuple(q.shape), tuple(k.shape), None if m is None else (m.dtype, tuple(m.shape))))
        return real_decode(q, k, v, m, scale, hip=hip)

    def spy_sdpa(module, query, *a, **k):
        many.append(query.shape[2])
        return real_sdpa(module, query, *a, **k)

    monkeypatch.setattr(LD, "decode_attention", spy_decode)
    monkeypatch.setattr(SA, "sdpa_attention_forward", spy_sdpa)
    with LD.hip_decode(llm):
        assert llm.config._attn_implementation == "mra_decode"
        got = llm.generate(cache_implementation="static", disable_compile=True, **kw)
    assert llm.config._attn_implementation == before
    assert torch.equal(got, stock) and got.shape == (3, n_new)
    # the prefill went to SDPA once per layer; every later step came with one query row, the un-repeated K/V heads of the whole static cache
    # and a bool mask over it
    assert many == [embeds.shape[1]] * LAYERS
    assert len(one) == LAYERS * (n_new - 1)
    for qs, ks, ms in one:
        assert qs == (3, HEADS, 1, LH // HEADS) and ks[:2] == (3, kv_heads) and ks[2] >= embeds.shape[1] + n_new - 1 and ks[3] == LH // HEADS
        assert ms == (torch.bool, (3, 1, 1, ks[2]))


def test_hip_decode_restores_the_implementation_after_an_exception():
    llm = _tiny_llama()
    before = llm.config._attn_implementation
    with pytest.raises(RuntimeError, match="inside"):
        with LD.hip_decode(llm):
            assert llm.config._attn_implementation == "mra_decode"
            raise RuntimeError("inside the block")
    assert llm.config._attn_implementation == before
    embeds, mask = _prefix()
    assert llm.generate(inputs_embeds=embeds, attention_mask=mask, max_new_tokens=2).shape[0] == 3


def test_other_calls_go_to_sdpa_with_the_arguments_untouched(monkeypatch):
    import transformers.integrations.sdpa_attention as SA

    seen = []
    monkeypatch.setattr(SA, "sdpa_attention_forward", lambda module, *a, **k: seen.append((a, k)) or ("sdpa", None))
    mod = nn.Module().eval()
    q1, q2 = torch.zeros(2, 4, 1, 64), torch.zeros(2, 4, 5, 64)
    k = torch.zeros(2, 2, 9, 64)
    bmask, fmask = torch.ones(2, 1, 1, 9, dtype=torch.bool), torch.zeros(2, 1, 1, 9)
    assert LD.attention_forward(mod, q1, k, k, bmask)[0].shape == (2, 1, 4, 64) and not seen
    assert LD.attention_forward(mod, q1, k, k, None, dropout=0.0, scaling=0.5, position_ids=None, use_cache=True)[0].shape == (2, 1, 4, 64) and not seen
    calls = [dict(q=q2, m=None), dict(q=q1, m=fmask), dict(q=q1, m=bmask, dropout=0.1), dict(q=q1, m=bmask, train=True),
             dict(q=torch.zeros(2, 4, 1, 32), kk=torch.zeros(2, 2, 9, 32), m=bmask), dict(q=torch.zeros(2, 6, 1, 64), m=bmask),
             dict(q=q1, m=bmask, sliding_window=4)]
    for c in calls:
        mod.train(bool(c.get("train")))
        kk = c.get("kk", k)
        extra = {"sliding_window": c["sliding_window"]} if "sliding_window" in c else {}
        out = LD.attention_forward(mod, c["q"], kk, kk, c["m"], dropout=c.get("dropout", 0.0), scaling=0.25, use_cache=True, **extra)
        assert out == ("sdpa", None)
        a, kw = seen.pop()
        assert a[0] is c["q"] and a[1] is kk and a[2] is kk and a[3] is c["m"]
        assert kw == dict(dropout=c.get("dropout", 0.0), scaling=0.25, use_cache=True, **extra)


# ---- the model's switch and the trainer, on a stand-in (the model itself needs a GPU) -----------------------------------------------------
class _Stub(nn.Module):
    """What ``generate_llm`` touches, with the Q-Former side replaced by fixed tensors: everything from the prompt assembly on is the model's
    own code.  ``generate`` stands in for the scorer's decode."""
    from mraudio_amd.models.xinstructblip import XInstructBLIP as _X

    lora, objective, lm_loss, prompt_assembly, lm_decode = False, "score", "stock", "cat", "stock"
    attach_llm, generate_llm, _llm_decode, train = _X.attach_llm, _X.generate_llm, _X._llm_decode, _X.train

    def __init__(self, llm, tok):
        super().__init__()
        self.modalities, self.num_query_token, self.max_txt_len, self.max_output_txt_len = ["audio"], Q, 128, 64
        self.llm_hidden_size, self._device, self.prompt_assembler = LH, torch.device("cpu"), None
        self.attach_llm(llm, tok)
        self.z = torch.randn(2, T * Q, LH, generator=torch.Generator().manual_seed(8)) * 0.1
        self.knob = nn.Parameter(torch.zeros(1))                                     # the trainer wants something to optimise
        self.scored, self.decoded = 0, 0

    def _llm_inputs(self, samples):
        self.decoded += 1
        n = len(samples["text_input"])
        return {"audio": self.z[:n]}, {"audio": torch.ones(n, T * Q, dtype=torch.long)}

    def generate(self, samples):
        self.scored += 1
        return ["[[0, 13]]"] * len(samples["text_input"])

    def forward(self, samples):
        return {"loss": (self.knob * 0).sum()}


def _stub():
    from mraudio_amd.models.llm_prompt import SimpleLlmTokenizer

    tok = SimpleLlmTokenizer()
    return _Stub(_tiny_llama(vocab=len(tok), kv_heads=2), tok)


SAMPLES = {"audio": torch.zeros(2, T, 1), "text_input": ["when does the dog bark", "find the song"], "timestamps": [[0, 2, 4], [0, 2, 4]],
           "duration": [6, 6]}


def test_lm_decode_hip_passes_disable_compile_and_decodes_the_stock_tokens(monkeypatch):
    stub = _stub()
    llm = stub.llm_model
    calls, tokens = [], []
    real = llm.generate

    def generate(**kw):
        calls.append({k: v for k, v in kw.items() if not torch.is_tensor(v)})
        tokens.append(real(**kw).clone())
        return tokens[-1].clone()

    monkeypatch.setattr(llm, "generate", generate)
    stock = stub.generate_llm(SAMPLES, max_new_tokens=12)
    assert calls == [dict(max_new_tokens=12)]                                        # the parent's call, keyword for keyword
    before = llm.config._attn_implementation
    routed = []
    real_decode = LD.decode_attention
    monkeypatch.setattr(LD, "decode_attention", lambda *a, **k: routed.append(1) or real_decode(*a, **k))
    stub.lm_decode = "hip"
    hip = stub.generate_llm(SAMPLES, max_new_tokens=12)
    assert calls[1] == dict(max_new_tokens=12, cache_implementation="static", disable_compile=True)
    assert routed and llm.config._attn_implementation == before
    assert torch.equal(tokens[0], tokens[1]) and hip == stock and len(hip) == 2
    stub.lm_decode = "stock"
    assert stub.generate_llm(SAMPLES, max_new_tokens=12) == stock and calls[2] == dict(max_new_tokens=12)
    stub.lm_decode = "fast"
    with pytest.raises(_lib.MraError, match="lm_decode"):
        stub.generate_llm(SAMPLES, max_new_tokens=12)


def test_constructor_refuses_an_unknown_lm_decode():
    from mraudio_amd.models.xinstructblip import XInstructBLIP

    with pytest.raises(ValueError, match="lm_decode"):
        XInstructBLIP(lm_decode="fast")
    assert XInstructBLIP.lm_decode == "stock"


def _trainer(tmp_path, model, **kw):
    from mraudio_amd.utils.mr_dataset import SyntheticMRDataset
    from mraudio_amd.utils.trainer import Trainer, default_args

    ds = SyntheticMRDataset(4, T=T, seed=3, duration=2 * T, kv_audio=2, modalities=("audio",))
    args = default_args(output_dir=str(tmp_path), gpu="cpu", max_epoch=1, batch_size=2, train_qformers=False, **kw)
    return Trainer(args, model=model, train_dataset=ds, val_dataset=ds), ds


def test_trainer_validates_on_the_decoded_strings(tmp_path):
    from mraudio_amd.eval.mr_eval import eval_submission
    from mraudio_amd.utils.mr_dataset import collate_fn
    from mraudio_amd.utils.spans import moment_str_to_list, post_process
    from mraudio_amd.utils.trainer import default_args

    assert default_args().val_decode == "score" and default_args().lm_decode == "stock"
    stub = _stub()
    tr, ds = _trainer(tmp_path, stub, val_decode="llm")
    assert tr.val_decode == "llm" and stub.lm_decode == "stock"
    got = tr.eval_epoch()
    assert stub.scored == 0 and stub.decoded == 2                                   # two batches of two, none through the scorer
    results = []
    for lo in (0, 2):
        batch = collate_fn([ds[i] for i in range(lo, lo + 2)])
        for i, txt in enumerate(stub.generate_llm(batch)):
            r = ds[lo + i]
            results.append({"qid": r["qid"], "query": r["query"], "vid": r["vid"], "relevant_windows": moment_str_to_list(post_process(r["text_output"])),
                            "pred_relevant_windows": moment_str_to_list(post_process(txt))})
    want = eval_submission(results, results, verbose=False)
    assert got["brief"] == want["brief"] and "MR-full-R1-avg" in got["brief"]
    # the default never decodes
    stub2 = _stub()
    tr2, _ = _trainer(tmp_path, stub2)
    assert tr2.val_decode == "score"
    tr2.eval_epoch()
    assert stub2.scored == 2 and stub2.decoded == 0
    # lm_decode reaches the model
    stub3 = _stub()
    _trainer(tmp_path, stub3, val_decode="llm", lm_decode="hip")
    assert stub3.lm_decode == "hip"


def test_trainer_flattens_a_grouped_validation_batch_in_order(tmp_path):
    stub = _stub()
    tr, ds = _trainer(tmp_path, stub, val_decode="llm")
    seen = []

    def generate_multi_llm(samples):
        seen.append(samples["text_input"])
        return [["[[2, 10]]", "[[2, 11]]"], ["[[1, 10]]"]]

    stub.generate_multi_llm = generate_multi_llm
    a, b, c = ds[0], ds[1], ds[2]
    grouped = {"audio_embeds": torch.zeros(2, T, 2, 768), "timestamps": [a["timestamps"]] * 2, "duration": [a["duration"]] * 2, "vid": ["v0", "v1"],
               "qid": [[0, 1], [2]], "query": [[a["query"], b["query"]], [c["query"]]], "text_input": [[a["text_input"], b["text_input"]], [c["text_input"]]],
               "text_output": [["[[2, 10]]", "[[0, 4]]"], ["[[1, 10]]"]]}
    tr.val_dataloader = [grouped]
    out = tr.eval_epoch()
    assert len(seen) == 1 and stub.scored == 0 and stub.decoded == 0
    # predictions [[2, 10]], [[2, 11]], [[1, 10]] against the targets above: the first and the last are exact, in the loader's order
    assert out["brief"]["MR-full-R1@0.7"] == pytest.approx(100 * 2 / 3, abs=0.01)


def test_trainer_refuses_val_decode_llm_without_an_lm(tmp_path):
    stub = _stub()
    object.__setattr__(stub, "llm_model", None)
    with pytest.raises(_lib.MraError, match="LM attached"):
        _trainer(tmp_path, stub, val_decode="llm")
    with pytest.raises(ValueError, match="val_decode"):
        _trainer(tmp_path, _stub(), val_decode="both")
    with pytest.raises(ValueError, match="lm_decode"):
        _trainer(tmp_path, _stub(), lm_decode="fast")


# ---- the command-line flags -----------------------------------------------------------------------------------------------------------------
def test_cli_flags_parse_and_default(capsys):
    from mraudio_amd import evaluate, finetune

    ap, base = finetune.build_parser(), ["--output-dir", "out", "--dataset", "QVH"]
    args = ap.parse_args(base)
    assert args.val_decode == "score" and args.lm_decode == "stock"
    args = ap.parse_args(base + ["--val-decode", "llm", "--lm-decode", "hip"])
    assert args.val_decode == "llm" and args.lm_decode == "hip"
    for bad in (["--val-decode", "both"], ["--lm-decode", "fast"]):
        with pytest.raises(SystemExit):
            ap.parse_args(base + bad)
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        finetune.main(base + ["--val-decode", "llm"])
    assert e.value.code == 2 and "--val-decode llm needs --llm-path" in capsys.readouterr().err
    ep = evaluate.build_parser()
    flags = {a.dest: a for a in ep._actions}
    assert flags["lm_decode"].default == "stock" and tuple(flags["lm_decode"].choices) == ("stock", "hip")
