"""Multi-query training step on the GPU (``-m gpu``): the backward attention core over a shared K/V item (through
``mra_debug_attention_bwd`` = ``launch_attn_bwd`` in the cross-attention layout of the backward) against the float64 reference of
``tests/multi_train_cases.py``; ``forward_multi_train`` + backward against the single-query step, against torch.autograd over the CPU
oracle on replicated encoder rows (the definition), and its accumulation and workspace; ``XInstructBLIP.forward_multi`` against one
ordinary training call per (video, query); one epoch of the grouped trainer.

Bars: those of tests/test_gpu_backward.py for a gradient tensor (relative Frobenius 2e-2, peak 5e-2 in f16, 8 x in bf16)."""
import functools

import pytest
import torch

import multi_train_cases as MT
from oracle import qformer_ref as O
from test_gpu_backward import DTYPES, _setup
from test_gpu_multi_query import make_rows

pytestmark = pytest.mark.gpu

HEADS, GUARD = 2, 256


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


# ---- 1. the core against float64 ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(kind, kv_items, share, q_rows, kv, dtype):
    """Inputs and float64 reference of one case, computed once."""
    q, k, v, d_o = MT.make_bwd(kind, kv_items, share, HEADS, q_rows, kv, dtype)
    o, lse, dq, dk, dv = MT.bwd_ref(q, k, v, d_o, share)
    return (q, k, v, o.to(dtype), d_o, lse.float()), (dq, dk, dv)


def pack(x):
    """[N, heads, rows, 64] -> the core's compact [N][rows][heads * 64]."""
    n, h, r, d = x.shape
    return x.transpose(1, 2).reshape(n, r, h * d).contiguous()


def unpack(x, heads):
    n, r, w = x.shape
    return x.view(n, r, heads, w // heads).transpose(1, 2)


def guarded(shape, dtype, dev):
    """A NaN-filled output of ``shape`` between two NaN guards: (whole buffer, the output's view)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((GUARD + n + GUARD,), float("nan"), dtype=dtype, device=dev)
    return buf, buf[GUARD: GUARD + n].view(shape)


def run_core(ins, share, dev, expect=0):
    from mraudio_amd import _lib

    L = _lib.lib()
    q, k, v, o, d_o, lse = ins
    N, heads, q_rows, _ = q.shape
    kv_items, kv = k.shape[0], k.shape[2]
    qd, od, gd = (pack(t).to(dev) for t in (q, o, d_o))
    kd, vd, ld = k.contiguous().to(dev), v.contiguous().to(dev), lse.contiguous().to(dev)
    (bq, dq), (bk, dk), (bv, dv) = guarded(qd.shape, q.dtype, dev), guarded(kd.shape, q.dtype, dev), guarded(vd.shape, q.dtype, dev)
    with torch.cuda.device(dev):
        rc = L.mra_debug_attention_bwd(_lib.ptr(qd), _lib.ptr(kd), _lib.ptr(vd), _lib.ptr(od), _lib.ptr(gd), _lib.ptr(ld), _lib.mra_dtype(q.dtype),
                                       kv_items, share, heads, q_rows, kv, _lib.ptr(dq), _lib.ptr(dk), _lib.ptr(dv), _lib.current_stream())
    torch.cuda.synchronize(dev)
    assert rc == expect, (rc, L.mra_last_error())
    for buf in (bq, bk, bv):      # nothing outside the outputs is written; with rc == 0 every element inside is
        assert torch.isnan(buf[:GUARD]).all().item() and torch.isnan(buf[-GUARD:]).all().item()
        assert torch.isnan(buf[GUARD:-GUARD]).any().item() == (rc != 0)
    return unpack(dq.cpu(), heads), dk.cpu(), dv.cpu()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("q_rows", (32, 20))
@pytest.mark.parametrize("share", (1, 2, 3, 5, 14))
def test_core_against_float64(share, q_rows, dtype, dev):
    worst = {}
    for kv_items in (1, 3):
        for kv in (1, 31, 32, 33, 129, 257):
            for kind in ("mild", "peaked"):
                ins, refs = case(kind, kv_items, share, q_rows, kv, dtype)
                got = run_core(ins, share, dev)
                for name, g, ref in zip(("dq", "dk", "dv"), got, refs):
                    rel, peak = MT.grad_errors(g, ref, refs[2])
                    worst[name] = max(worst.get(name, (0, 0)), (rel, peak))
                    assert rel < MT.BARS[dtype][0] and peak < MT.BARS[dtype][1], (kind, kv_items, share, q_rows, kv, name, rel, peak)
    print(f"share {share} q_rows {q_rows} {dtype}: worst (relative Frobenius, peak) {worst}")


def test_core_refuses_a_share_the_lds_cannot_hold(dev):
    from mraudio_amd import _lib

    ins, _ = case("mild", 1, 1, 32, 33, torch.float16)
    q, k, v, o, d_o, lse = ins
    rep = lambda t: t.repeat(15, 1, 1, 1)   # noqa: E731
    run_core((rep(q), k, v, rep(o), rep(d_o), lse.repeat(15, 1, 1)), 15, dev, expect=-1)       # MRA_EINVAL, nothing written
    assert b"14" in _lib.lib().mra_last_error()


# ---- 2. forward_multi_train: one prompt is the existing step -------------------------------------------------------------------------
def _enc(w, enc_items, kv, E, seed, op_dtype):
    feats = torch.randn(enc_items, kv, E, generator=torch.Generator().manual_seed(seed))
    return O.modality_layernorm(feats, w["ln.weight"], w["ln.bias"]).to(op_dtype)


def test_one_prompt_is_the_existing_training_step(dev):
    """``mra_qformer_forward_train`` + ``mra_qformer_backward`` called directly, on a workspace and a gradient buffer of the test's own,
    against ``forward_train`` + ``backward()``, which go through the multi entries with one prompt per item."""
    from mraudio_amd import _lib

    qf, cfg, ocfg, w = _setup(dev, 768, 1)
    n, L, kv = 3, 5, 40
    ids, att = make_rows(cfg, n, L, 3)
    ids, att = ids.to(dev).contiguous(), att.to(dev).contiguous()
    enc = _enc(w, n, kv, 768, 4, torch.float16).to(dev).contiguous()
    g = torch.Generator().manual_seed(5)
    rq, rc = torch.randn(n, 32, 768, generator=g).to(dev), torch.randn(n, 768, generator=g).to(dev)
    qf.enable_training()
    L_ = _lib.lib()
    nbytes = int(L_.mra_qformer_train_workspace_bytes(qf._handle, n, L, kv))
    assert nbytes > 0 and nbytes == L_.mra_qformer_multi_train_workspace_bytes(qf._handle, n, 1, L, kv)
    # the single entries, directly: d loss / d q = rq and d loss / d cls = rc for the loss below
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    grads = torch.zeros_like(qf._grad_flat)
    q0, c0 = torch.empty(n, 32, 768, device=dev), torch.empty(n, 768, device=dev)
    with torch.cuda.device(dev):
        rc_ = L_.mra_qformer_forward_train(qf._handle, _lib.ptr(ids), _lib.ptr(att), _lib.ptr(enc), n, L, kv, _lib.ptr(q0), _lib.ptr(c0), _lib.ptr(ws),
                                           nbytes, _lib.current_stream())
        assert rc_ == 0, L_.mra_last_error()
        rc_ = L_.mra_qformer_backward(qf._handle, _lib.ptr(ids), _lib.ptr(att), _lib.ptr(enc), n, L, kv, _lib.ptr(rq), _lib.ptr(rc), _lib.ptr(grads),
                                      _lib.ptr(ws), nbytes, _lib.current_stream())
        assert rc_ == 0, L_.mra_last_error()
    torch.cuda.synchronize()
    qf._grad_flat.zero_()
    q, c = qf.forward_train(ids, att, enc)
    ((q * rq).sum() + (c * rc).sum()).backward()
    torch.cuda.synchronize()
    assert torch.equal(q0, q.detach()) and torch.equal(c0, c.detach())
    assert grads.abs().max().item() > 0
    assert torch.allclose(qf._grad_flat, grads, rtol=1e-3, atol=1e-5)


# ---- 2b. one node, one tape policy --------------------------------------------------------------------------------------------------------
STEPS = {"A": (2, 5, 24, 3), "B": (3, 7, 40, 13)}       # enc items, L, kv, seed; B's tape is the larger one


@functools.lru_cache(maxsize=None)
def _tape_qf():
    return _setup(torch.device("cuda:0"), 768, 1)


@functools.lru_cache(maxsize=None)
def _step_inputs(name, P):
    """Inputs of step ``name`` with ``P`` prompts per item (0: ``forward_train``), on the device."""
    qf, cfg, ocfg, w = _tape_qf()
    dev = torch.device("cuda:0")
    n, L, kv, seed = STEPS[name]
    N = n * max(P, 1)
    ids, att = make_rows(cfg, N, L, seed)
    g = torch.Generator().manual_seed(seed + 1)
    rq, rc = torch.randn(N, 32, 768, generator=g).to(dev), torch.randn(N, 768, generator=g).to(dev)
    return ids.to(dev), att.to(dev), _enc(w, n, kv, 768, seed + 2, torch.float16).to(dev), rq, rc


def _forward(name, P):
    """The forward of a step: (loss, q, cls, enc leaf)."""
    qf = _tape_qf()[0]
    ids, att, enc0, rq, rc = _step_inputs(name, P)
    enc = enc0.clone().requires_grad_(True)
    q, c = qf.forward_multi_train(ids, att, enc, P) if P else qf.forward_train(ids, att, enc)
    return (q * rq).sum() + (c * rc).sum(), q, c, enc


@functools.lru_cache(maxsize=None)
def _step_alone(name, P):
    """One step on its own from a zeroed gradient buffer: (q, cls, enc.grad, flat gradient buffer), computed once."""
    qf = _tape_qf()[0]
    qf.enable_training()
    qf._grad_flat.zero_()
    loss, q, c, enc = _forward(name, P)
    loss.backward()
    torch.cuda.synchronize()
    return q.detach().clone(), c.detach().clone(), enc.grad.clone(), qf._grad_flat.clone()


@pytest.mark.parametrize("PA,PB", [(0, 0), (0, 3), (3, 0)], ids=["single-single", "single-multi3", "multi3-single"])
def test_overlapping_tapes_do_not_disturb_each_other(dev, PA, PB):
    """Forward A, forward B (a larger tape), backward B, backward A on one ``QFormer`` give what A and B give alone.  Before the training
    node owned its tape, the single-prompt forward wrote it into a buffer of the owner that B's forward overwrote or replaced: the single
    cases then gave wrong gradients for A with no error (not measured: that code is not run for this)."""
    qf = _tape_qf()[0]
    alone = {"A": _step_alone("A", PA), "B": _step_alone("B", PB)}
    qf._grad_flat.zero_()
    fa = _forward("A", PA)
    fb = _forward("B", PB)
    assert fa[1].grad_fn.ws is not fb[1].grad_fn.ws
    fb[0].backward()
    fa[0].backward()
    torch.cuda.synchronize()
    for name, (_, q, c, enc) in (("A", fa), ("B", fb)):
        q1, c1, d_enc1, _ = alone[name]
        assert torch.equal(q.detach(), q1) and torch.equal(c.detach(), c1), name
        assert d_enc1.abs().max().item() > 0 and torch.equal(enc.grad, d_enc1), (name, (enc.grad - d_enc1).abs().max().item())
    want = alone["A"][3] + alone["B"][3]
    assert want.abs().max().item() > 0
    assert torch.allclose(qf._grad_flat, want, rtol=1e-3, atol=1e-5), (qf._grad_flat - want).abs().max().item()


def test_a_training_loop_reuses_one_tape_buffer(dev):
    qf = _tape_qf()[0]
    ids, att, enc, rq, rc = _step_inputs("B", 0)
    ptrs, allocated = [], []
    for _ in range(3):
        q, c = qf.forward_train(ids, att, enc)
        ptrs.append(q.grad_fn.ws.data_ptr())
        ((q * rq).sum() + (c * rc).sum()).backward()
        del q, c
        torch.cuda.synchronize()
        allocated.append(torch.cuda.memory_allocated(dev))
    assert ptrs[0] == ptrs[1] == ptrs[2], ptrs
    assert allocated[2] == allocated[1], allocated


def test_forward_train_validates_its_arguments_before_any_launch(dev):
    from mraudio_amd import _lib
    from mraudio_amd._lib import MraError

    qf, cfg, ocfg, w = _tape_qf()
    n, L, kv, _ = STEPS["A"]
    ids, att, enc, _, _ = _step_inputs("A", 0)
    qf.enable_training()
    qf._grad_flat.fill_(1.0)
    nbytes = int(_lib.lib().mra_qformer_train_workspace_bytes(qf._handle, n + 1, L, kv))
    spare = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=dev).view(torch.uint8)
    qf._train_ws = spare
    before = spare.clone()
    bad = {"attention_mask [N, L]": (ids, att[:, 32:], enc),
           "input_ids with N + 1 rows": (torch.cat([ids, ids[:1]]), att, enc),
           "enc of the wrong width": (ids, att, enc[..., :704]),
           "no items": (ids[:0], att[:0], enc[:0])}
    for what, (i, a, e) in bad.items():
        with pytest.raises(MraError):
            qf.forward_train(i, a, e)
        torch.cuda.synchronize()
        assert qf._train_ws is spare and torch.equal(spare, before), what
        assert bool((qf._grad_flat == 1.0).all()), what
    qf._grad_flat.zero_()


# ---- 3. gradients against oracle autograd on replicated encoder rows -------------------------------------------------------------------
ORACLE_CASES = [(2, 3, 9, 40, 1408, torch.float16), (2, 3, 9, 40, 1408, torch.bfloat16), (1, 5, 4, 33, 768, torch.float16),
                (1, 2, 9, 257, 1408, torch.float16), (1, 2, 4, 2049, 768, torch.float16)]


@pytest.mark.parametrize("enc_items,P,L,kv,E,op_dtype", ORACLE_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_forward_backward_matches_oracle_autograd_on_replicated_rows(dev, enc_items, P, L, kv, E, op_dtype):
    fwd_tol, rel_tol, peak_tol = next(d[1:] for d in DTYPES if d[0] == op_dtype)
    qf, cfg, ocfg, w = _setup(dev, E, 0, op_dtype)
    N = enc_items * P
    ids, att = make_rows(cfg, N, L, 77)                    # a different ragged prompt per slot
    enc = _enc(w, enc_items, kv, E, 78, op_dtype)          # the exact operand the kernels see, once per encoder item
    g = torch.Generator().manual_seed(5)
    rq, rc = torch.randn(N, 32, 768, generator=g), torch.randn(N, 768, generator=g)

    # oracle: fp32 autograd, chain row i * P + p over the encoder rows of item i
    wl = {k: (v.clone().requires_grad_(True) if k.startswith("bert.") or k == "query_tokens" else v) for k, v in w.items()}
    h = O.qformer_forward(wl, ocfg, ids, att, wl["query_tokens"].expand(N, -1, -1), enc.float().repeat_interleave(P, 0))
    ((h[:, :32] * rq).sum() + (h[:, 32] * rc).sum()).backward()

    q, c = qf.forward_multi_train(ids.to(dev), att.to(dev), enc.to(dev), P)
    assert (q.cpu() - h[:, :32].detach()).abs().max().item() < fwd_tol
    assert (c.cpu() - h[:, 32].detach()).abs().max().item() < fwd_tol
    ((q * rq.to(dev)).sum() + (c * rc.to(dev)).sum()).backward()
    torch.cuda.synchronize()

    worst, worst_name = 0.0, ""
    for k, ref in wl.items():
        if not (k.startswith("bert.") or k == "query_tokens"):
            continue
        gref = ref.grad
        got = qf.grad_of(k).view_as(gref).cpu()
        if k.endswith("key.bias"):
            # softmax is invariant to a per-query shift of the scores: the true key-bias gradient is 0 (tests/test_gpu_backward.py)
            scale = wl[k.replace(".key.", ".query.")].grad.norm().item()
            assert got.norm().item() < rel_tol * scale + 1e-4, (k, got.norm().item(), scale)
            continue
        rel = ((got - gref).norm() / gref.norm()).item()
        peak = (got - gref).abs().max().item() / gref.abs().max().item()
        if rel > worst:
            worst, worst_name = rel, k
        assert rel < rel_tol and peak < peak_tol, (k, rel, peak)
    print("worst relative gradient error", (enc_items, P, L, kv, E, op_dtype), worst, worst_name)


# ---- 4. accumulation, 5. the tape shares the cache ---------------------------------------------------------------------------------------
def test_two_backward_calls_give_twice_the_gradient(dev):
    qf, cfg, ocfg, w = _setup(dev, 768, 1)
    n, P, L, kv = 2, 3, 5, 24
    ids, att = make_rows(cfg, n * P, L, 3)
    enc = _enc(w, n, kv, 768, 4, torch.float16).to(dev)
    keys = ("bert.encoder.layer.0.crossattention.self.value.weight", "bert.encoder.layer.2.crossattention.self.key.weight", "query_tokens")

    def run():
        q, c = qf.forward_multi_train(ids.to(dev), att.to(dev), enc, P)
        (q.sum() + c.sum()).backward()

    run()
    g1 = {k: qf.grad_of(k).clone() for k in keys}
    run()
    for k in keys:
        assert g1[k].abs().max().item() > 0
        assert torch.allclose(qf.grad_of(k), 2 * g1[k], rtol=1e-3, atol=1e-5), k
    for p in qf.bert.parameters():                   # what optimizer.zero_grad(set_to_none=True) does
        p.grad = None
    run()
    assert torch.allclose(qf.grad_of(keys[0]), g1[keys[0]], rtol=1e-3, atol=1e-5)


@pytest.mark.parametrize("n,P,L,kv", [(2, 3, 9, 257), (1, 8, 4, 40), (20, 4, 32, 257)])
def test_the_tape_holds_one_kv_cache_per_encoder_item(dev, n, P, L, kv):
    from mraudio_amd import _lib

    qf, cfg, _, _ = _setup(dev, 1408, 0)
    L_ = _lib.lib()
    single = int(L_.mra_qformer_train_workspace_bytes(qf._handle, n * P, L, kv))
    multi = int(L_.mra_qformer_multi_train_workspace_bytes(qf._handle, n, P, L, kv))
    cache = int(L_.mra_kv_cache_bytes(qf._handle, n, kv))
    assert cache > 0 and multi > 0
    assert single - multi >= 2 * (P - 1) * cache - 64 * 1024, (single, multi, cache)     # K/V and dK/dV


def test_prompts_beyond_the_lds_limit_are_refused(dev):
    from mraudio_amd._lib import MraError

    qf, cfg, ocfg, w = _setup(dev, 768, 1)
    ids, att = make_rows(cfg, 15, 4, 3)
    enc = _enc(w, 1, 24, 768, 4, torch.float16).to(dev)
    with pytest.raises(MraError, match="14"):
        qf.forward_multi_train(ids.to(dev), att.to(dev), enc, 15)


# ---- 6. the model ----------------------------------------------------------------------------------------------------------------------
PROMPT = "Query: {}\nGiven the video and the query, find the relevant windows.\nRelevant windows: "
QUERIES = [["a person opens the door.", "someone sits down on the sofa and reads", "a dog barks"], ["the light is switched off"]]
WINDOWS = [["[[2, 4]]", "[[0, 0], [6, 6]]", "[[4, 6]]"], ["[[0, 2]]"]]


def _grouped_batch():
    g = torch.Generator().manual_seed(2)
    T = 4
    return {"video_embeds": torch.randn(2, T, 257, 1408, generator=g), "audio_embeds": torch.randn(2, T, 256, 768, generator=g),
            "text_input": [[PROMPT.format(q) for q in qs] for qs in QUERIES], "text_output": WINDOWS,
            "timestamps": [list(range(0, 2 * T, 2))] * 2, "duration": [2 * T] * 2}


@pytest.fixture(scope="module")
def trained_model(dev):
    """One model with trainable Q-Formers for the tests below, which run in file order (the last one moves the weights)."""
    from mraudio_amd.models.xinstructblip import XInstructBLIP

    model = XInstructBLIP(seed=3, perturb=True, device=dev)
    model.enable_qformer_training()
    return model


def test_model_forward_multi_equals_one_training_call_per_video_and_query(trained_model):
    model = trained_model
    batch = _grouped_batch()
    qfs = {m: getattr(model, f"{m}_Qformer") for m in model.modalities}
    losses = []
    for b, qs in enumerate(QUERIES):
        for p in range(len(qs)):
            one = {"video_embeds": batch["video_embeds"][b: b + 1], "audio_embeds": batch["audio_embeds"][b: b + 1],
                   "text_input": [batch["text_input"][b][p]], "text_output": [WINDOWS[b][p]], "timestamps": [batch["timestamps"][b]], "duration": [8]}
            loss = model(one)["loss"]
            loss.backward()
            losses.append(loss.item())
    torch.cuda.synchronize()
    want_loss = sum(losses) / 4
    want = {m: qf._grad_flat.clone() / 4 for m, qf in qfs.items()}
    for qf in qfs.values():
        qf._grad_flat.zero_()
    loss = model(batch)["loss"]                            # list-valued text_input: forward_multi
    assert abs(loss.item() - want_loss) <= 1e-3 * max(1.0, abs(want_loss)), (loss.item(), want_loss)
    loss.backward()
    torch.cuda.synchronize()
    rel_bar, peak_bar = 2 * MT.BARS[torch.float16][0], 2 * MT.BARS[torch.float16][1]     # both sides carry 16-bit noise
    for m, qf in qfs.items():
        got, ref = qf._grad_flat, want[m]
        assert ref.abs().max().item() > 0 and torch.isfinite(got).all().item()
        rel = ((got - ref).norm() / ref.norm()).item()
        peak = ((got - ref).abs().max() / ref.abs().max()).item()
        print(f"{m}: grouped vs per-pair gradient, relative Frobenius {rel:.3e} peak {peak:.3e}")
        assert rel < rel_bar and peak < peak_bar, (m, rel, peak)
    assert model.video_query_tokens.grad is not None and torch.isfinite(model.video_query_tokens.grad).all()
    # chunked groups: at most 2 queries per call, the same loss
    model.max_queries_per_call = 2
    for qf in qfs.values():
        qf._grad_flat.zero_()
    loss2 = model(batch)["loss"]
    assert abs(loss2.item() - want_loss) <= 1e-3 * max(1.0, abs(want_loss))
    loss2.backward()                                       # two tapes per Q-Former alive at once: each call holds its own workspace
    torch.cuda.synchronize()
    for m, qf in qfs.items():
        rel = ((qf._grad_flat - want[m]).norm() / want[m].norm()).item()
        assert rel < rel_bar, (m, rel)
    model.max_queries_per_call = 8


def test_one_adam_step_over_a_grouped_batch_lowers_its_loss(trained_model):
    from mraudio_amd.utils.optim import FusedQFormerAdam

    model = trained_model
    batch = _grouped_batch()
    opt = FusedQFormerAdam(model, lr=2e-5)
    opt.zero_grad()
    before = model(batch)["loss"]
    before.backward()
    opt.step()
    after = model(batch)["loss"]
    assert torch.isfinite(after) and after.item() < before.item(), (before.item(), after.item())


def test_forward_multi_without_training_is_the_forward_only_value(dev):
    from mraudio_amd.models.xinstructblip import XInstructBLIP

    model = XInstructBLIP(seed=3, perturb=True, device=dev)
    batch = _grouped_batch()
    frozen = model(batch)["loss"]
    assert not frozen.requires_grad
    model.enable_qformer_training()
    trained = model(batch)["loss"]
    assert trained.requires_grad and abs(frozen.item() - trained.item()) <= 1e-3 * max(1.0, abs(trained.item()))


# ---- 7. the trainer ----------------------------------------------------------------------------------------------------------------------
def test_one_epoch_of_the_grouped_trainer(dev, tmp_path):
    import math

    from mraudio_amd.models.xinstructblip import XInstructBLIP
    from mraudio_amd.utils.mr_dataset import SyntheticMRDataset, VideoGroupedDataset
    from mraudio_amd.utils.trainer import Trainer, default_args

    args = default_args(output_dir=str(tmp_path), gpu=0, max_epoch=1, warmup_steps=2, group_by_video=True, max_queries_per_call=2, lr=1e-5)
    tr = Trainer(args, model=XInstructBLIP(seed=3, perturb=True, device=dev),
                 train_dataset=SyntheticMRDataset(2, T=4, seed=0, signal=1.0, queries_per_video=3), val_dataset=SyntheticMRDataset(2, T=4, seed=1, signal=1.0))
    assert isinstance(tr.train_dataloader.dataset, VideoGroupedDataset) and len(tr.train_dataloader) == 2
    stats = tr.train_epoch(0)
    assert math.isfinite(stats["loss_value"]) and stats["loss_value"] > 0
    assert all(torch.isfinite(getattr(tr.model, f"{m}_Qformer")._master_flat).all().item() for m in tr.model.modalities)
