"""The LM head + cross-entropy on the labelled rows without a GPU (``-m "not gpu"``): the fp32 emulation of csrc/lm_head.hip sits inside
the derived bounds of tests/lm_head_cases.py and every named mutant lands outside; the torch route of ``mraudio_amd/models/lm_head.py``
against float64 and against a stock ``LlamaForCausalLM``'s own loss; the model's ``lm_loss`` switch on a stand-in (the model itself needs a
GPU); the entries' argument refusals with host pointers; the workspace formula; the command-line flag."""
import ctypes as C
import math

import pytest
import torch
from torch import nn

import lm_head_cases as HC
from mraudio_amd import _lib
from mraudio_amd.models import lm_head as H


def _id(dt):
    return str(dt).split(".")[-1]


# ---- the table ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", HC.DTYPES, ids=_id)
def test_emulation_sits_inside_every_bound(dtype):
    worst = [0.0, 0.0, 0.0]
    for R, V, K in HC.cases():
        r = HC.ratios(R, V, K, dtype, *HC.emulate(R, V, K, dtype))
        assert max(r) <= 1.0, ((R, V, K), r)
        worst = [max(a, b) for a, b in zip(worst, r)]
    print(f"{_id(dtype)}: worst |d| / bound of the emulation: nll {worst[0]:.3f} lse {worst[1]:.3f} dh {worst[2]:.3f}")
    assert all(w > 0.0 for w in worst)


MUTANT_CASES = [c for c in HC.cases() if c[0] >= 16 and c[1] in (257, 1000, 2200)]


@pytest.mark.parametrize("dtype", HC.DTYPES, ids=_id)
@pytest.mark.parametrize("mutant", HC.MUTANTS)
def test_mutants_land_outside_somewhere(mutant, dtype):
    assert len(MUTANT_CASES) >= 8
    worst = max(max(HC.ratios(R, V, K, dtype, *HC.emulate(R, V, K, dtype, mutant=mutant))) for R, V, K in MUTANT_CASES)
    assert worst > 1.0, (mutant, worst)


def test_table_covers_what_it_says():
    cs = HC.cases()
    assert {c[0] for c in cs} == set(HC.ROWS) and {c[1] for c in cs} == set(HC.VOCABS) and {c[2] for c in cs} == set(HC.KS)
    assert {(r, v) for r, v, _ in cs} >= {(r, v) for r in (1, 130) for v in (1, 1000)}
    assert HC.splits(130, 2200, 512) == 12 and HC.splits(16, 1000, 64) == 16 and HC.splits(80, 32001, 4096) == 16
    seen_fam, seen_nan = set(), 0
    for R, V, K in cs:
        c = HC.make_case(R, V, K, torch.bfloat16)
        seen_fam |= set(c["family"])
        seen_nan += int((c["labels"] == -1).sum()) + int((c["labels"] == V).sum())
        if R >= 16 and V >= 130:
            lab = set(c["labels"].tolist())
            assert {0, 63, 64, V - 1, (HC.tiles(V) - 1) * 64} <= lab and len(lab) < R
        assert c["g"].min() < 0 < c["g"].max() or R < 3
    assert seen_fam == set(range(8)) and seen_nan > 0
    c = HC.make_case(17, 1000, 64, torch.float16)                                  # the all-equal row: log V exactly
    ref = HC.reference(17, 1000, 64, torch.float16)
    r = c["family"].index(5)
    assert abs(ref["lse"][r].item() - math.log(1000)) < 1e-12


# ---- the torch route ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 257, 64), (3, 1000, 200), (1, 8, 8)])
def test_torch_route_is_the_float64_definition(shape):
    R, V, K = shape
    c, ref = HC.make_case(R, V, K, torch.bfloat16), HC.reference(R, V, K, torch.bfloat16)
    h = c["h"].double().requires_grad_(True)
    nll = H.lm_head_ce_rows(h, c["W"].double(), c["labels"].long(), hip=False, reduction="none")
    assert nll.dtype == torch.float64
    (nll * c["g"].double()).sum().backward()
    assert (nll.detach() - ref["nll"]).abs().max() <= 1e-6 * ref["nll"].abs().max()
    assert (h.grad - ref["dh"]).abs().max() <= 1e-6 * ref["dh"].abs().max()
    mean = H.lm_head_ce_rows(c["h"].double(), c["W"].double(), c["labels"].long(), hip=False)
    assert abs(mean.item() - ref["nll"].mean().item()) <= 1e-6 * abs(ref["nll"].mean().item())
    # 16-bit operands compute in fp32: inside the kernels' own bounds
    h16 = c["h"].clone().requires_grad_(True)
    nll16 = H.lm_head_ce_rows(h16, c["W"], c["labels"].long(), hip=False, reduction="none")
    assert nll16.dtype == torch.float32
    (nll16 * c["g"]).sum().backward()
    assert HC.ratio(nll16.detach(), ref["nll"], ref["nll_b"]) <= 1.0 and HC.ratio(h16.grad, ref["dh"], ref["dh_b"]) <= 1.0


def test_routes_and_refusals_of_the_python_entry():
    hidden, weight, labels = torch.randn(2, 5, 16), torch.randn(11, 16), torch.full((2, 5), -100)
    labels[0, 2] = 3
    assert H.lm_head_ce(hidden, weight, labels).dtype == torch.float32              # hip=None on the CPU: the torch route
    with pytest.raises(_lib.MraError, match="CUDA"):
        H.lm_head_ce(hidden, weight, labels, hip=True)
    with pytest.raises(ValueError, match="reduction"):
        H.lm_head_ce(hidden, weight, labels, reduction="sum")
    with pytest.raises(ValueError, match="expected"):
        H.lm_head_ce(hidden, weight[:, :8], labels)
    none = H.lm_head_ce(hidden, weight, labels, reduction="none")
    assert none.shape == (1,)
    z = hidden[0, 1] @ weight.t()                                                    # position 1 predicts labels[2]
    assert abs(none.item() - (torch.logsumexp(z, 0) - z[3]).item()) < 1e-5
    # no labelled row at all: what cross_entropy gives (NaN for the mean, an empty vector for "none"), and still differentiable
    empty = torch.full((2, 5), -100)
    empty[1, 0] = 4                                                                  # a label at position 0 predicts nothing
    hg = hidden.clone().requires_grad_(True)
    loss = H.lm_head_ce(hg, weight, empty)
    assert torch.isnan(loss) and loss.requires_grad
    assert H.lm_head_ce(hidden, weight, empty, reduction="none").shape == (0,)
    assert torch.isnan(nn.functional.cross_entropy(torch.zeros(0, 11), torch.zeros(0, dtype=torch.long)))


def _tiny_llama(dtype=torch.float32, vocab=64, hidden=32):
    tf = pytest.importorskip("transformers")
    torch.manual_seed(0)
    cfg = tf.LlamaConfig(vocab_size=vocab, hidden_size=hidden, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4,
                         num_key_value_heads=4, max_position_embeddings=512, pad_token_id=0, bos_token_id=2, eos_token_id=2)
    return tf.LlamaForCausalLM(cfg).to(dtype).eval().requires_grad_(False)


def test_lm_head_ce_is_the_llamas_own_loss_and_gradients():
    llm = _tiny_llama().requires_grad_(True)
    gen = torch.Generator().manual_seed(4)
    B, S = 3, 12
    embeds = torch.randn(B, S, 32, generator=gen)
    mask = torch.ones(B, S, dtype=torch.long)
    labels = torch.full((B, S), -100)
    labels[0, 7:] = torch.randint(3, 64, (5,), generator=gen)
    labels[0, 0] = 9                                                                 # the shift drops it
    labels[2, 4:9] = torch.randint(3, 64, (5,), generator=gen)                       # sample 1 has no label at all
    e1 = embeds.clone().requires_grad_(True)
    stock = llm(inputs_embeds=e1, attention_mask=mask, return_dict=True, labels=labels).loss
    stock.backward()
    want = {n: p.grad.clone() for n, p in llm.named_parameters() if p.grad is not None}        # embed_tokens is not on this path
    llm.zero_grad()
    e2 = embeds.clone().requires_grad_(True)
    hidden = llm.get_decoder()(inputs_embeds=e2, attention_mask=mask, return_dict=True).last_hidden_state
    loss = H.lm_head_ce(hidden, llm.get_output_embeddings().weight, labels)
    loss.backward()
    assert abs(loss.item() - stock.item()) <= 1e-5 * abs(stock.item())
    assert (e2.grad - e1.grad).abs().max() <= 1e-5 * e1.grad.abs().max()
    assert {n for n, p in llm.named_parameters() if p.grad is not None} == set(want)
    for n in want:                                                                   # lm_head.weight among them: the torch route has dW
        p = llm.get_parameter(n)
        assert (p.grad - want[n]).abs().max() <= 1e-5 * max(want[n].abs().max().item(), 1e-3), n
    assert want["lm_head.weight"].abs().max() > 0
    per_row = H.lm_head_ce(hidden.detach(), llm.lm_head.weight.detach(), labels, reduction="none")
    assert per_row.shape == (5 + 5,) and abs(per_row.mean().item() - stock.item()) <= 1e-5 * abs(stock.item())


# ---- the model's switch, on a stand-in (the model itself needs a GPU) ------------------------------------------------------------------------
LH, Q, T = 32, 4, 3


class _Stub(nn.Module):
    """What ``forward`` / ``forward_llm`` touch under the LM objectives with frozen Q-Formers, with the Q-Former side replaced by fixed
    tensors: everything from the prompt assembly on is the model's own code."""
    from mraudio_amd.models.xinstructblip import XInstructBLIP as _X

    lora, objective, lm_weight, loss_scale, lm_loss = False, "llm", 1.0, 1.0, "stock"
    forward, forward_llm, _lm_ce, _lora_loss, _lora_unscale = _X.forward, _X.forward_llm, _X._lm_ce, _X._lora_loss, _X._lora_unscale
    attach_llm, enable_lora, lora_parameters, train, _present, _targets = (_X.attach_llm, _X.enable_lora, _X.lora_parameters, _X.train, _X._present,
                                                                          _X._targets)
    parse_windows, _WINDOW = _X.parse_windows, _X._WINDOW

    def __init__(self, llm, tok):
        super().__init__()
        self.modalities, self.num_query_token, self.max_txt_len, self.max_output_txt_len = ["audio"], Q, 128, 64
        self.llm_hidden_size, self._device, self.prompt_assembler = LH, torch.device("cpu"), None
        self.attach_llm(llm, tok)
        gen = torch.Generator().manual_seed(8)
        self.z = torch.randn(2, T * Q, LH, generator=gen) * 0.1
        self.fused = torch.randn(2 * T, generator=gen)

    def _llm_inputs(self, samples):
        return {"audio": self.z}, {"audio": torch.ones(2, T * Q, dtype=torch.long)}

    def encode_fuse(self, samples, want_llm=False):
        return {"fused": self.fused, "bs": 2, "num": T, "inputs_llm": {"audio": self.z}, "atts_llm": {"audio": torch.ones(2, T * Q, dtype=torch.long)}}


def _stub(lora=False):
    from mraudio_amd.models.llm_prompt import SimpleLlmTokenizer

    tok = SimpleLlmTokenizer()
    stub = _Stub(_tiny_llama(vocab=len(tok), hidden=LH), tok)
    if lora:
        stub.enable_lora(r=4, alpha=8, dropout=0.0)
        gen = torch.Generator().manual_seed(2)
        with torch.no_grad():
            for p in stub.lora_parameters():
                p.copy_(torch.randn(p.shape, generator=gen) * 0.05)
    return stub


SAMPLES = {"audio": torch.zeros(2, T, 1), "text_input": ["when does the dog bark", "find the song"], "text_output": ["[[0, 2]]", "[[2, 4]]"],
           "timestamps": [[0, 2, 4], [0, 2, 4]], "duration": [6, 6]}


def test_stock_is_the_parents_call_and_rows_never_runs_lm_head():
    stub = _stub()
    fired = []
    stub.llm_model.lm_head.register_forward_hook(lambda *a: fired.append(1))
    inputs_llm, atts = stub._llm_inputs(SAMPLES)
    embeds, mask, targets = stub.prompt_assembler.assemble_forward(SAMPLES, inputs_llm, atts)
    parent = stub.llm_model(inputs_embeds=embeds, attention_mask=mask, return_dict=True, labels=targets).loss
    assert fired == [1]
    assert stub.lm_loss == "stock" and torch.equal(stub.forward_llm(SAMPLES, train=False)["loss"], parent)      # the same bits
    assert fired == [1, 1]
    del fired[:]
    stub.lm_loss = "rows"
    rows = stub.forward_llm(SAMPLES, train=False)["loss"]
    assert fired == [] and abs(rows.item() - parent.item()) <= 1e-5 * abs(parent.item())
    stub.lm_loss = "fused"                                                           # on the CPU: the torch route, silently
    assert torch.equal(stub.forward_llm(SAMPLES, train=False)["loss"], rows) and fired == []
    stub.lm_loss = "other"
    with pytest.raises(_lib.MraError, match="lm_loss"):
        stub.forward_llm(SAMPLES, train=False)


@pytest.mark.parametrize("objective", ["llm", "both"])
def test_rows_equals_stock_with_frozen_qformers_and_lora(objective):
    out = {}
    for mode in ("stock", "rows"):
        stub = _stub(lora=True)
        stub.objective, stub.lm_loss, stub.lm_weight, stub.loss_scale = objective, mode, 0.5, 4.0
        stub.train()
        res = stub(SAMPLES)
        res["loss"].backward()
        out[mode] = (res, [p.grad.clone() for p in stub.lora_parameters()])
    (a, ga), (b, gb) = out["stock"], out["rows"]
    assert set(a) == set(b) == ({"loss"} if objective == "llm" else {"loss", "loss_score", "loss_lm"})
    for k in a:
        assert abs(a[k].item() - b[k].item()) <= 1e-5 * abs(a[k].item()), k
    assert len(ga) == len(gb) > 0 and max(g.abs().max().item() for g in ga) > 0
    for x, y in zip(ga, gb):
        assert (x - y).abs().max() <= 1e-5 * max(x.abs().max().item(), 1e-4)


def test_an_lm_with_a_biased_head_or_no_decoder_is_refused():
    stub = _stub()
    stub.lm_loss = "rows"
    head = stub.llm_model.lm_head
    stub.llm_model.lm_head = nn.Linear(LH, head.out_features, bias=True)
    with pytest.raises(_lib.MraError, match="bias"):
        stub.forward_llm(SAMPLES, train=False)

    class _NoDecoder(nn.Module):
        def __init__(self, llm):
            super().__init__()
            self.llm = llm

        def get_input_embeddings(self):
            return self.llm.get_input_embeddings()

        def forward(self, **kw):
            return self.llm(**kw)

    stub.llm_model.lm_head = head
    object.__setattr__(stub, "llm_model", _NoDecoder(stub.llm_model))
    with pytest.raises(_lib.MraError, match="decoder"):
        stub.forward_llm(SAMPLES, train=False)
    stub.lm_loss = "stock"
    assert torch.isfinite(stub.forward_llm(SAMPLES, train=False)["loss"])


# ---- the ABI entries without a device ---------------------------------------------------------------------------------------------------------
def test_entries_refuse_bad_arguments_before_any_launch():
    lib = _lib.lib()
    buf = C.create_string_buffer(1 << 16)
    p = (C.addressof(buf) + 15) // 16 * 16
    BF = _lib.MRA_BF16
    need = HC.workspace_bytes(4, 100, 32, True)

    def fwd(h=p, ldh=32, R=4, K=32, W=p, ldw=32, V=100, dt=BF, labels=p, nll=p, lse=p, ws=p, nbytes=need, want=1):
        return lib.mra_lm_head_ce_forward(h, ldh, R, K, W, ldw, V, dt, labels, nll, lse, ws, nbytes, want, None)

    def bwd(g=p, W=p, ldw=32, V=100, K=32, dt=BF, labels=p, lse=p, ws=p, nbytes=need, dh=p, lddh=32, R=4):
        return lib.mra_lm_head_ce_backward(g, W, ldw, V, K, dt, labels, lse, ws, nbytes, dh, lddh, R, None)

    bad_f = [("null", dict(h=None)), ("null", dict(W=None)), ("null", dict(labels=None)), ("null", dict(nll=None)), ("null", dict(lse=None)),
             ("null", dict(ws=None)), ("ldh < K", dict(ldh=24)), ("ldw < K", dict(ldw=24)), ("pitches", dict(ldh=36)), ("pitches", dict(ldw=44)),
             ("16-byte aligned", dict(h=p + 8)), ("16-byte aligned", dict(W=p + 2)), ("16-byte aligned", dict(ws=p + 4)),
             ("4-byte aligned", dict(labels=p + 2)), ("4-byte aligned", dict(nll=p + 1)), ("K must", dict(K=36, ldh=40, ldw=40)), ("K must", dict(K=0)),
             ("V must", dict(V=0)), ("dtype", dict(dt=_lib.MRA_F32)), ("negative R", dict(R=-1)), ("workspace too small", dict(nbytes=need - 1)),
             ("workspace too small", dict(want=0, nbytes=HC.workspace_bytes(4, 100, 32, False) - 1))]
    for msg, kw in bad_f:
        assert fwd(**kw) == -1, kw
        assert msg.encode() in lib.mra_last_error(), (kw, lib.mra_last_error())
    bad_b = [("null", dict(g=None)), ("null", dict(dh=None)), ("null", dict(lse=None)), ("lddh < K", dict(lddh=24)), ("pitches", dict(lddh=36)),
             ("ldw < K", dict(ldw=8)), ("16-byte aligned", dict(dh=p + 8)), ("4-byte aligned", dict(g=p + 2)), ("K must", dict(K=12)),
             ("V must", dict(V=-3)), ("dtype", dict(dt=7)), ("negative R", dict(R=-2)), ("workspace too small", dict(nbytes=need - 1)),
             ("workspace too small", dict(nbytes=HC.workspace_bytes(4, 100, 32, False)))]
    for msg, kw in bad_b:
        assert bwd(**kw) == -1, kw
        assert msg.encode() in lib.mra_last_error(), (kw, lib.mra_last_error())
    # R == 0 launches nothing and needs nothing, not even pointers
    assert fwd(R=0, h=None, W=None, ws=None, nbytes=0) == 0 and bwd(R=0, g=None, dh=None, ws=None, nbytes=0) == 0


def test_workspace_bytes_agree_with_the_header_formula():
    lib = _lib.lib()
    for R, V, K in HC.cases() + [(80, 32001, 4096), (0, 5, 8), (300, 70000, 1024)]:
        for dt in (_lib.MRA_F16, _lib.MRA_BF16):
            for want in (0, 1):
                assert lib.mra_lm_head_ce_workspace_bytes(R, V, K, dt, want) == HC.workspace_bytes(R, V, K, bool(want)), (R, V, K, want)
    assert HC.workspace_bytes(80, 32001, 4096, True) * 10 < 2 * 2700 * 32001 * 2          # a tenth of the 16-bit [B, S, V] logits of B = 2, S = 2700
    for bad in ((-1, 5, 8, _lib.MRA_BF16), (1, 0, 8, _lib.MRA_BF16), (1, 5, 12, _lib.MRA_BF16), (1, 5, 8, _lib.MRA_F32)):
        assert lib.mra_lm_head_ce_workspace_bytes(*bad, 1) == 0
        assert b"lm_head_ce_workspace_bytes" in lib.mra_last_error()


def test_cli_flag_parses_and_defaults_to_stock(capsys):
    from mraudio_amd import finetune

    ap, base = finetune.build_parser(), ["--output-dir", "out", "--dataset", "QVH"]
    assert ap.parse_args(base).lm_loss == "stock"
    assert ap.parse_args(base + ["--lm-loss", "fused"]).lm_loss == "fused" and ap.parse_args(base + ["--lm-loss", "rows"]).lm_loss == "rows"
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--lm-loss", "fast"])
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        finetune.main(base + ["--lm-loss", "fused"])                                 # the default objective is the scorer's
    assert e.value.code == 2 and "--lm-loss rows / fused needs" in capsys.readouterr().err
