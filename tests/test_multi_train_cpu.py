"""Multi-query training step without a GPU: the float64 reference of the shared-K/V backward core against a torch emulation of the
kernel's arithmetic and its named mutants (tests/multi_train_cases.py), the loss layout of ``XInstructBLIP.forward_multi`` for ragged
and chunked groups on a stub Q-Former, the trainer / ``finetune`` flag wiring on a stub model, and the argument checks of the new ABI
entries."""
import ctypes as C

import pytest
import torch
from torch import nn

import multi_train_cases as MT
from mraudio_amd import _lib
from mraudio_amd.models.xinstructblip import HashTokenizer, XInstructBLIP
from mraudio_amd.utils import mr_dataset as D
from mraudio_amd.utils.trainer import Trainer, default_args

DTYPES = [torch.float16, torch.bfloat16]
SHAPES = [(1, 1, 1, 32), (3, 2, 1, 20), (1, 2, 31, 32), (3, 3, 33, 20), (3, 5, 129, 20), (1, 14, 257, 32)]   # kv_items, share, kv, q_rows


def _case(kind, kv_items, share, kv, q_rows, dtype):
    q, k, v, d_o = MT.make_bwd(kind, kv_items, share, 2, q_rows, kv, dtype)
    o, lse, dq, dk, dv = MT.bwd_ref(q, k, v, d_o, share)
    return (q, k, v, o.to(dtype), d_o, lse.float()), (dq, dk, dv)


# ---- the backward core ------------------------------------------------------------------------------------------------------------
def test_reference_is_autograd_of_the_float64_forward():
    q, k, v, d_o = MT.make_bwd("mild", 2, 3, 2, 20, 33, torch.float16)
    o, lse, dq, dk, dv = MT.bwd_ref(q, k, v, d_o, 3)
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    s = qd @ kd.repeat_interleave(3, 0).transpose(-1, -2) / 8.0
    out = torch.softmax(s, -1) @ vd.repeat_interleave(3, 0)
    (out * d_o.double()).sum().backward()
    for got, want in ((dq, qd.grad), (dk, kd.grad), (dv, vd.grad)):
        assert torch.allclose(got, want, rtol=1e-10, atol=1e-12)
    assert torch.allclose(out.detach(), o, rtol=1e-12, atol=1e-14)
    assert torch.allclose(lse, torch.log2(torch.exp2(s.detach() * MT.LOG2E).sum(-1)), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("kind", ["mild", "peaked"])
def test_emulated_core_sits_inside_the_gradient_bars(kind, dtype):
    for kv_items, share, kv, q_rows in SHAPES:
        ins, (dq, dk, dv) = _case(kind, kv_items, share, kv, q_rows, dtype)
        got = MT.emulate_bwd(*ins, share)
        for name, g, ref in zip(("dq", "dk", "dv"), got, (dq, dk, dv)):
            assert MT.inside(g, ref, dtype, dv), (kind, kv_items, share, kv, q_rows, name, MT.grad_errors(g, ref, dv))


MUTANT_SHAPES = [s for s in SHAPES if s[1] > 1 and s[2] > 1]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_mutant_lse_of_slot_0_lands_outside(dtype):
    kinds = ("peaked", "mild") if dtype == torch.float16 else ("peaked",)
    for kind in kinds:
        for kv_items, share, kv, q_rows in MUTANT_SHAPES:
            ins, (dq, dk, dv) = _case(kind, kv_items, share, kv, q_rows, dtype)
            got = MT.emulate_bwd(*ins, share, mutant="lse_slot0")
            for g, ref in zip(got, (dq, dk, dv)):     # slot 0 itself is right, every other slot is off: all three tensors miss
                assert not MT.inside(g, ref, dtype), (kind, kv_items, share, kv, q_rows)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("kind", ["mild", "peaked"])
def test_mutant_dkv_of_the_last_slot_only_lands_outside(kind, dtype):
    for kv_items, share, kv, q_rows in MUTANT_SHAPES:
        ins, (dq, dk, dv) = _case(kind, kv_items, share, kv, q_rows, dtype)
        gq, gk, gv = MT.emulate_bwd(*ins, share, mutant="dkv_last")
        assert MT.inside(gq, dq, dtype)
        assert not MT.inside(gk, dk, dtype) and not MT.inside(gv, dv, dtype), (kind, kv_items, share, kv, q_rows)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("kind", ["mild", "peaked"])
def test_mutant_dq_written_to_slot_0_lands_outside(kind, dtype):
    for kv_items, share, kv, q_rows in MUTANT_SHAPES:
        ins, (dq, dk, dv) = _case(kind, kv_items, share, kv, q_rows, dtype)
        gq, gk, gv = MT.emulate_bwd(*ins, share, mutant="dq_slot0")
        assert not MT.inside(gq, dq, dtype), (kind, kv_items, share, kv, q_rows)
        assert MT.inside(gk, dk, dtype) and MT.inside(gv, dv, dtype)


# ---- XInstructBLIP.forward_multi on a stub Q-Former ---------------------------------------------------------------------------------
class StubQFormer:
    """``modality_ln`` / ``forward_train`` / ``forward_multi_train`` with the real row order on a one-parameter torch model: the output of
    chain row (item i, slot p) depends on the item's features, on the row's own prompt and mask, and on ``w`` -- so a wrong row order, a
    padded slot that leaks into the loss or a wrong weight of a chunk changes the loss or ``w.grad``."""

    def __init__(self, width: int):
        g = torch.Generator().manual_seed(width)
        self.w = nn.Parameter(torch.randn(16, generator=g))
        self.proj = torch.randn(width, 16, generator=g)
        self.calls, self.d_out = [], []

    def modality_ln(self, raw, item_index=None, items=None):
        return raw.float()

    def _rows(self, ids, att, enc_rows):
        txt = ((ids.float() * att[:, 32:].float()).sum(1, keepdim=True) % 97.0) / 97.0            # [N, 1] from the row's own prompt
        feat = enc_rows.mean(1) @ self.proj                                                          # [N, 16]
        z = torch.sin(feat[:, None, :] * self.w + torch.arange(32.0)[None, :, None] * 0.1 + txt[:, :, None])
        cls = torch.cos(feat * self.w.flip(0) + 3.0 * txt)
        z.register_hook(lambda g: self.d_out.append(g.clone()))
        return z, cls

    def forward_train(self, ids, att, enc, want_cls=True):
        self.calls.append(("single", int(enc.shape[0]), 1))
        return self._rows(ids, att, enc)

    def forward_multi_train(self, ids, att, enc, prompts, want_cls=True):
        assert ids.shape[0] == enc.shape[0] * prompts and att.shape == (ids.shape[0], 32 + ids.shape[1])
        self.calls.append(("multi", int(enc.shape[0]), int(prompts)))
        return self._rows(ids, att, enc.repeat_interleave(prompts, 0))


class StubModel(XInstructBLIP):
    def __init__(self):
        nn.Module.__init__(self)
        self.modalities = ("video", "audio")
        self._device = torch.device("cpu")
        self.tokenizer = HashTokenizer(truncation_side="left")
        self.max_txt_len, self.num_query_token, self.fuse_weights, self.compat_repeat = 128, 32, None, False
        self.train_qformers = True
        object.__setattr__(self, "video_Qformer", StubQFormer(24))
        object.__setattr__(self, "audio_Qformer", StubQFormer(12))

    def _sync(self):
        pass

    def grads(self):
        return [getattr(self, f"{m}_Qformer").w.grad.clone() for m in self.modalities]

    def zero(self):
        for m in self.modalities:
            qf = getattr(self, f"{m}_Qformer")
            qf.w.grad, qf.calls, qf.d_out = None, [], []


T = 5
QUERIES = [["a man opens the door", "he sits", "a dog", "someone is cooking dinner", "the end"], ["one"], ["x y", "z", "a b c d"]]
WINDOWS = [["[[0, 2]]", "[[4, 6], [8, 8]]", "[[-1, -1]]", "[[2.5, 7]]", "[[8, 8]]"], ["[[0, 8]]"], ["[[2, 4]]", "[[6, 8]]", "[[0, 0]]"]]


def _grouped():
    g = torch.Generator().manual_seed(1)
    return {"video_embeds": torch.randn(3, T, 4, 24, generator=g), "audio_embeds": torch.randn(3, T, 3, 12, generator=g),
            "text_input": [[D.build_prompt(q) for q in qs] for qs in QUERIES], "text_output": WINDOWS,
            "timestamps": [[0, 2, 4, 6, 8]] * 3, "duration": [10] * 3}


def _single(samples, b, p):
    return {"video_embeds": samples["video_embeds"][b: b + 1], "audio_embeds": samples["audio_embeds"][b: b + 1],
            "text_input": [samples["text_input"][b][p]], "text_output": [samples["text_output"][b][p]],
            "timestamps": [samples["timestamps"][b]], "duration": [10]}


@pytest.fixture(scope="module")
def per_pair():
    """The definition: one ordinary ``forward`` per (video, query); mean loss and mean gradient over the nine pairs."""
    model, samples = StubModel(), _grouped()
    losses = []
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(torch.cuda, "current_stream", lambda device=None: None)     # forward() asks for the device's stream; there is none here
        for b, qs in enumerate(QUERIES):
            for p in range(len(qs)):
                loss = model(_single(samples, b, p))["loss"]
                loss.backward()
                losses.append(loss.item())
    n = len(losses)
    assert n == 9 and all(c[0] == "single" for c in model.video_Qformer.calls)
    return sum(losses) / n, [g / n for g in model.grads()]


@pytest.mark.parametrize("step,calls", [(8, [(3, 5)]), (5, [(3, 5)]), (2, [(3, 2), (2, 2), (1, 1)]), (1, [(3, 1), (2, 1), (2, 1), (1, 1), (1, 1)]),
                                        (3, [(3, 3), (1, 2)])])
def test_forward_multi_is_the_mean_over_video_query_pairs(per_pair, step, calls):
    want_loss, want_grads = per_pair
    model, samples = StubModel(), _grouped()
    model.max_queries_per_call = step
    loss = model(samples)["loss"]                       # forward() dispatches on the list-valued text_input
    loss.backward()
    assert abs(loss.item() - want_loss) < 1e-6
    for got, want in zip(model.grads(), want_grads):
        assert torch.allclose(got, want, rtol=1e-5, atol=1e-7)
    # the calls: (videos, prompts) per round, the videos with no query left dropped from the encoder rows
    assert model.video_Qformer.calls == [("multi", nb * T, P) for nb, P in calls] == model.audio_Qformer.calls


def test_padded_slots_get_exactly_zero_gradient():
    model, samples = StubModel(), _grouped()
    model(samples)["loss"].backward()
    (d_z,) = model.video_Qformer.d_out                # [3 * T * 5, 32, 16], row (b * T + t) * 5 + p
    d_z = d_z.view(3, T, 5, 32, 16)
    for b, qs in enumerate(QUERIES):
        assert d_z[b, :, :len(qs)].abs().sum().item() > 0
        if len(qs) < 5:
            assert d_z[b, :, len(qs):].abs().max().item() == 0.0


def test_explicit_queries_and_targets_override_the_record_and_are_validated():
    model, samples = StubModel(), _grouped()
    a = model.forward_multi(samples)["loss"].item()
    bare = {k: v for k, v in samples.items() if k not in ("text_input", "text_output")}
    b = model.forward_multi(bare, queries=samples["text_input"], targets=WINDOWS)["loss"].item()
    assert a == b
    other = [[w for w in reversed(ws)] for ws in WINDOWS]
    assert model.forward_multi(bare, queries=samples["text_input"], targets=other)["loss"].item() != a
    with pytest.raises(Exception, match="one text_output per query"):
        model.forward_multi(bare, queries=samples["text_input"], targets=[ws[:1] for ws in WINDOWS])
    with pytest.raises(Exception, match="at least one query"):
        model.forward_multi(bare, queries=[[], ["a"], ["b"]])
    with pytest.raises(ValueError):                    # a malformed annotation cannot train on an empty target
        model.forward_multi(bare, queries=[["a"], ["b"], ["c"]], targets=[["none"], ["[[1, 2]]"], ["[[1, 2]]"]])


def test_flat_text_input_takes_the_single_query_path(monkeypatch):
    model, samples = StubModel(), _grouped()
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: None)
    model(_single(samples, 0, 1))
    assert model.video_Qformer.calls == [("single", T, 1)]


# ---- trainer / finetune wiring ----------------------------------------------------------------------------------------------------
class GroupScorer(nn.Module):
    """forward -> {"loss"} on grouped and on flat records; remembers what it was given."""

    def __init__(self):
        super().__init__()
        self.w = nn.Linear(16, 1)
        self.max_queries_per_call = 8
        self.seen = []

    def forward(self, samples):
        self.seen.append(samples["text_input"])
        x = self.w(samples["video_embeds"][..., :16].mean(2)).squeeze(-1)
        return {"loss": (x ** 2).mean()}

    @torch.no_grad()
    def generate(self, samples):
        assert isinstance(samples["text_input"][0], str)            # validation keeps one record per annotation line
        return ["[[0, 2]]"] * len(samples["text_input"])


def _trainer(tmp_path, **kw):
    args = default_args(output_dir=str(tmp_path), gpu="cpu", max_epoch=1, warmup_steps=2, **kw)
    ds = dict(T=20, kv_video=2, modalities=("video",), signal=1.0)
    return Trainer(args, model=GroupScorer(), train_dataset=D.SyntheticMRDataset(3, seed=0, queries_per_video=3, **ds),
                   val_dataset=D.SyntheticMRDataset(2, seed=1, **ds))


def test_trainer_default_is_one_record_per_annotation_line(tmp_path):
    tr = _trainer(tmp_path)
    assert tr.group_by_video is False and tr.max_queries_per_call == 8
    tr.train_epoch(0)
    assert len(tr.model.seen) == 9 and all(isinstance(t[0], str) for t in tr.model.seen)


def test_trainer_group_by_video_feeds_one_record_per_video(tmp_path):
    tr = _trainer(tmp_path, group_by_video=True, max_queries_per_call=2)
    assert tr.model.max_queries_per_call == 2 and isinstance(tr.train_dataloader.dataset, D.VideoGroupedDataset)
    stats = tr.train_epoch(0)
    assert len(tr.model.seen) == 3 and all(len(t) == 1 and len(t[0]) == 3 for t in tr.model.seen)
    assert stats["loss_value"] == stats["loss_value"]
    res = tr.eval_epoch()                                            # flat records, as before
    assert "MR-full-R1@0.5" in res["brief"]
    with pytest.raises(ValueError):
        _trainer(tmp_path, group_by_video=True, max_queries_per_call=0)


def test_finetune_flags_are_spelled_as_in_evaluate():
    from mraudio_amd import evaluate, finetune

    base = ["--output-dir", "o", "--dataset", "QVH"]
    a = finetune.build_parser().parse_args(base)
    assert a.group_by_video is False and a.max_queries_per_call == 8 and a.synthetic_queries == 1
    a = finetune.build_parser().parse_args(base + ["--group-by-video", "--max-queries-per-call", "4", "--synthetic", "2", "--synthetic-queries", "3"])
    assert a.group_by_video is True and a.max_queries_per_call == 4 and a.synthetic_queries == 3
    ev = evaluate.build_parser().parse_args(["--output-file", "o", "--group-by-video", "--max-queries-per-call", "4"]) if hasattr(evaluate, "build_parser") else None
    if ev is not None:
        assert ev.group_by_video is True and ev.max_queries_per_call == 4


def test_synthetic_dataset_keeps_its_output_and_can_group():
    kw = dict(T=6, modalities=("audio",), kv_audio=2, signal=1.0)
    one, many = D.SyntheticMRDataset(3, **kw), D.SyntheticMRDataset(3, queries_per_video=3, **kw)
    assert len(one) == 3 and len(many) == 9
    # the default: the records of the generator the class has always used (window, then features, from one seeded stream)
    g = torch.Generator().manual_seed(1)
    s = int(torch.randint(0, 4, (1,), generator=g))
    e = min(5, s + 1 + int(torch.randint(1, 2, (1,), generator=g)))
    ts = [round(k * 40 / 6) for k in range(6)]
    x = torch.randn(6, 2, 768, generator=g)
    x[s:e + 1] += torch.randn(1, 1, 768, generator=torch.Generator().manual_seed(7))
    assert one[1]["text_output"] == str([[ts[s], ts[e]]]) and torch.equal(one[1]["audio_embeds"], x) and one[1]["qid"] == 1
    for i in range(3):
        for k in ("text_input", "text_output", "vid", "query"):
            assert many[3 * i][k] == one[i][k]                        # query 0 of a video is the single-query record
        for r in range(3):
            assert torch.equal(many[3 * i + r]["audio_embeds"], one[i]["audio_embeds"]) and many[3 * i + r]["vid"] == f"syn{i}"
        assert len({many[3 * i + r]["text_input"] for r in range(3)}) == 3
    for j, a in enumerate(many.annotation):
        rec = many[j]
        assert (a["qid"], a["query"], a["vid"], str(a["relevant_windows"])) == (rec["qid"], rec["query"], rec["vid"], rec["text_output"])
    grouped = D.VideoGroupedDataset(many)
    assert len(grouped) == 3 and [len(grouped[g]["text_input"]) for g in range(3)] == [3, 3, 3]


# ---- the ABI entries without a device ---------------------------------------------------------------------------------------------
def test_new_entries_reject_bad_arguments_before_any_launch():
    L = _lib.lib()
    assert L.mra_qformer_multi_train_workspace_bytes(None, 2, 3, 9, 257) == 0
    for call in (lambda p: L.mra_qformer_forward_multi_train(None, None, None, None, 2, p, 9, 257, None, None, None, 0, None),
                 lambda p: L.mra_qformer_backward_multi(None, None, None, None, 2, p, 9, 257, None, None, None, None, 0, None)):
        assert call(3) == -1 and b"null handle" in L.mra_last_error()
        assert call(0) == -1 and b"prompts" in L.mra_last_error()      # refused on its own ground, ahead of everything else
    # the single entries: the same checks behind a null-handle test of their own
    assert L.mra_qformer_train_workspace_bytes(None, 2, 9, 257) == 0
    assert L.mra_qformer_forward_train(None, None, None, None, 2, 9, 257, None, None, None, 0, None) == -1 and b"null handle" in L.mra_last_error()
    assert L.mra_qformer_backward(None, None, None, None, 2, 9, 257, None, None, None, None, 0, None) == -1 and b"null handle" in L.mra_last_error()
    # the core's debug entry: host buffers stand in for device memory, every call below must return before it would launch
    f = C.create_string_buffer(1 << 12)
    args = lambda **kw: [kw.get(k, d) for k, d in (("q", f), ("k", f), ("v", f), ("o", f), ("d_o", f), ("lse", f), ("dtype", _lib.MRA_F16),   # noqa: E731
                                                   ("kv_items", 1), ("share", 2), ("heads", 2), ("q_rows", 32), ("kv", 8), ("dq", f), ("dk", f),
                                                   ("dv", f), ("stream", None))]
    for name in ("q", "k", "v", "o", "d_o", "lse", "dq", "dk", "dv"):
        assert L.mra_debug_attention_bwd(*args(**{name: None})) == -1 and b"null" in L.mra_last_error(), name
    for name in ("kv_items", "share", "heads", "q_rows", "kv"):
        for bad in (0, -1):
            assert L.mra_debug_attention_bwd(*args(**{name: bad})) == -1 and b"sizes" in L.mra_last_error(), name
    assert L.mra_debug_attention_bwd(*args(dtype=_lib.MRA_F32)) == -1 and b"dtype" in L.mra_last_error()
    assert L.mra_debug_attention_bwd(*args(share=15)) == -1
    assert b"15" in L.mra_last_error() and b"14" in L.mra_last_error() and b"LDS" in L.mra_last_error()
    assert L.mra_debug_attention_bwd(*args(share=8, q_rows=33)) == -1 and b"exceeds 7" in L.mra_last_error()   # two query blocks per slot
    assert L.mra_debug_attention_bwd(*args(share=1, q_rows=15 * 32)) == -1 and b"exceeds 0" in L.mra_last_error()
