"""Prompt assembly as a row gather on the GPU (``-m gpu``): ``mra_gather_rows`` alone against ``index_select`` + ``.to()`` bit for bit;
``assemble_plan`` on the HIP route against its torch route; and the model on a tiny bf16 Llama: the ``prompt_assembly`` switch, the LM
objective on grouped batches (``forward`` / ``forward_llm`` over ``forward_multi``'s pass) against the flattened batch, ``generate_multi_llm``.

A gather has no rounding of its own: kernel and assembly comparisons are exact (NaN compared as NaN).  Grouped against flattened goes
through two different Q-Former forwards (shared K/V against replicated rows), so it is held to the bars tests/test_gpu_multi_train.py
uses for exactly that: the loss to 1e-3 * max(1, |loss|), a gradient tensor to twice ``multi_train_cases.BARS`` of the operand dtype."""
import itertools

import pytest
import torch

import multi_train_cases as MT
import prompt_plan_cases as K

pytestmark = pytest.mark.gpu

LH = 256


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


# ---- 1. the entry alone -----------------------------------------------------------------------------------------------------------------
def _bits(x):
    return x.view(torch.int32 if x.dtype == torch.float32 else torch.int16)


def _same(a, b):
    """Bit for bit, NaN compared as NaN."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(na, nb) and torch.equal(_bits(a)[~na], _bits(b)[~nb])


def _f32(bits):
    return torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32).view(torch.float32)


# exact round-to-even ties of both 16-bit types (down to even, up to even), the largest finite values and the first value that overflows,
# subnormals of f32 / bf16 / f16 with their ties, signed zeros, +-inf, NaN
SPECIAL_F32 = _f32([0x3F808000, 0x3F818000, 0x3F801000, 0x3F803000, 0xBF808000, 0xBF818000,       # ties: bf16 (1 + 2^-8 ...), f16 (1 + 2^-11 ...)
                    0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F0000, 0x7F7F8000, 0x477FE000, 0x477FF000, 0xC77FF000,   # f32 max, bf16 max and its tie, 65504, 65520
                    0x00000001, 0x00400000, 0x00008000, 0x00018000, 0x80008000,                  # f32 / bf16 subnormals and bf16 ties among them
                    0x33800000, 0x33000000, 0x33C00000, 0x387FC000, 0xB3800000,                  # 2^-24 (f16's smallest), 2^-25 (tie to 0), 3 * 2^-25, f16's largest subnormal
                    0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x3F800000])
SPECIAL_16 = {torch.float16: [0x0001, 0x03FF, 0x0400, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00, 0xFE01, 0x0000, 0x8000, 0x3C00],
              torch.bfloat16: [0x0001, 0x007F, 0x0080, 0x7F7F, 0xFF7F, 0x7F80, 0xFF80, 0x7FC0, 0xFFC1, 0x0000, 0x8000, 0x3F80]}
ACCEPTED = {torch.bfloat16: (torch.float32, torch.bfloat16), torch.float16: (torch.float32, torch.float16),
            torch.float32: (torch.float32, torch.float16, torch.bfloat16)}


def _source(dtype, rows, width, pad, gen, dev):
    """A pitched source [rows, width] inside [rows, width + pad]: random values with the special ones scattered through every row."""
    x = torch.randn(rows, width + pad, generator=gen) * 4.0
    if dtype == torch.float32:
        sp = SPECIAL_F32
    else:
        sp = torch.tensor([b - 65536 if b >= 32768 else b for b in SPECIAL_16[dtype]], dtype=torch.int16).view(dtype)
    x = x.to(dtype)
    pos = torch.randint(0, width, (rows, sp.numel()), generator=gen)
    x.scatter_(1, pos, sp[None, :].expand(rows, -1).contiguous())
    return x.to(dev)[:, :width]


CASES = list(itertools.product((torch.bfloat16, torch.float16, torch.float32), (8, 264, 4096), (1, 5, 257), (1, 2, 3, 4)))


@pytest.mark.parametrize("out_dtype,width,n_rows,n_src", CASES,
                         ids=[f"{str(o)[6:]}-w{w}-n{n}-s{s}" for o, w, n, s in CASES])
def test_gather_rows_against_index_select(dev, out_dtype, width, n_rows, n_src):
    from mraudio_amd.models.llm_prompt import gather_rows

    gen = torch.Generator().manual_seed(width * 1000 + n_rows * 10 + n_src)
    kinds = ACCEPTED[out_dtype]
    # every accepted source dtype appears: the cycle starts at a different one per source count
    srcs = [_source(kinds[(k + n_src) % len(kinds)], 3 + 4 * k, width, 8 * (k % 2 + (n_src > 2)), gen, dev) for k in range(n_src)]
    s = torch.randint(0, n_src, (n_rows,), generator=gen)
    r = torch.stack([torch.randint(0, srcs[int(k)].shape[0], (1,), generator=gen)[0] for k in s])
    plan = torch.stack([s, r], dim=1)
    if n_rows >= 5:
        plan[1] = torch.tensor([-1, 0])
        plan[3] = torch.tensor([0, srcs[0].shape[0]])              # one past the last row
    if n_rows >= 257:
        for i, e in zip((7, 64, 65, 128, 255, 256), ([-1, 5], [n_src, 0], [0, -1], [-2, 0], [7, 3], [n_src - 1, 1 << 30])):
            plan[i] = torch.tensor(e)
    ldo, guard = width + 16, 64
    buf = torch.full((guard + n_rows * ldo + guard,), 1.0, dtype=torch.float32).to(out_dtype).to(dev)
    _bits(buf).fill_(0x5A5A if out_dtype != torch.float32 else 0x5A5A5A5A)
    want_buf = buf.clone()
    out = buf[guard: guard + n_rows * ldo].view(n_rows, ldo)[:, :width]
    want = want_buf[guard: guard + n_rows * ldo].view(n_rows, ldo)[:, :width]
    for i, (si, ri) in enumerate(plan.tolist()):
        if si == -1:
            want[i] = 0
        elif 0 <= si < n_src and 0 <= ri < srcs[si].shape[0]:
            want[i] = srcs[si].index_select(0, torch.tensor([ri], device=dev)).to(out_dtype)[0]
        else:
            want[i] = float("nan")
    dplan = plan.to(torch.int32).to(dev)
    gather_rows(srcs, dplan, out=out)
    torch.cuda.synchronize(dev)
    assert _same(buf, want_buf)                                    # the rows, and the sentinels before, between and behind them
    first = buf.clone()
    _bits(buf).fill_(0)
    gather_rows(srcs, dplan, out=out)
    torch.cuda.synchronize(dev)
    assert torch.equal(_bits(out), _bits(first[guard: guard + n_rows * ldo].view(n_rows, ldo)[:, :width]))     # two runs, the same bits


def test_gather_rows_wrapper_refuses_what_the_entry_refuses(dev):
    from mraudio_amd._lib import MraError
    from mraudio_amd.models.llm_prompt import gather_rows

    plan = torch.zeros(2, 2, dtype=torch.int32, device=dev)
    with pytest.raises(MraError, match="f16 <-> bf16"):
        gather_rows([torch.zeros(2, 8, dtype=torch.float16, device=dev)], plan, torch.bfloat16)
    with pytest.raises(MraError, match="multiple of 8"):
        gather_rows([torch.zeros(2, 12, device=dev)], plan, torch.bfloat16)


# ---- 2. assemble_plan: the HIP route against the torch route ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["ordinary", "grouped"])
def test_assemble_plan_hip_equals_torch_route(dev, layout):
    from mraudio_amd.models.llm_prompt import assemble_plan

    D = 264
    asm, emb = K.make_assembler("both", layout == "ordinary", True, torch.bfloat16, D, device=dev)
    if layout == "ordinary":
        B, T = 3, 5
        plan = asm.plan_forward(K.make_samples(B, T), num=T)
        rows = B * T * K.Q
    else:
        flat, pairs, media_rows, rows = K.grouped_case()
        plan = asm.plan_forward(flat, media_rows, K.Q, num=K.G_T, rows=rows)
    media = K.make_media(("video", "audio"), rows, D, seed=9, device=dev)
    a = {m: v.clone().requires_grad_(True) for m, v in media.items()}
    b = {m: v.clone().requires_grad_(True) for m, v in media.items()}
    e_hip, m_hip, t_hip = assemble_plan(plan, emb.weight, a, hip=True)
    e_ref, m_ref, t_ref = assemble_plan(plan, emb.weight, b, hip=False)
    assert e_hip.dtype == torch.bfloat16 and torch.equal(_bits(e_hip), _bits(e_ref)) and torch.equal(m_hip, m_ref) and torch.equal(t_hip, t_ref)
    cot = torch.randn(e_ref.shape, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).to(dev)
    e_hip.backward(cot)
    e_ref.backward(cot)
    for m in media:
        assert a[m].grad.dtype == torch.float32 and torch.equal(_bits(a[m].grad), _bits(b[m].grad)), m
        assert a[m].grad.abs().sum().item() > 0
        if layout == "grouped":
            assert (plan.inverse[m] < 0).any() and a[m].grad[(plan.inverse[m] < 0).to(dev)].abs().max().item() == 0.0


# ---- 3. the model on a tiny bf16 Llama (helpers as in tests/test_gpu_llm_objective.py) ---------------------------------------------------
def _tiny_llama(dev, dtype=torch.bfloat16):
    tf = pytest.importorskip("transformers")
    from mraudio_amd.models.llm_prompt import SimpleLlmTokenizer

    torch.manual_seed(0)
    tok = SimpleLlmTokenizer()
    cfg = tf.LlamaConfig(vocab_size=len(tok), hidden_size=LH, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                         num_key_value_heads=4, max_position_embeddings=4096, pad_token_id=tok.pad_token_id, bos_token_id=2, eos_token_id=2)
    llm = tf.LlamaForCausalLM(cfg).to(dev).to(dtype).eval().requires_grad_(False)
    return llm, tok


def _model(dev, llm, tok, seed=0, **kw):
    from mraudio_amd.models.xinstructblip import XInstructBLIP

    model = XInstructBLIP(seed=seed, perturb=True, device=dev, llm_hidden_size=LH, op_dtype=torch.bfloat16, **kw)
    model.attach_llm(llm, tok)
    return model


def _batch(dev, n=2, T=6):
    from mraudio_amd.utils.mr_dataset import SyntheticMRDataset, collate_fn

    ds = SyntheticMRDataset(n, T=T, seed=5, duration=2 * T)
    batch = collate_fn([ds[i] for i in range(n)])
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}


PROMPT = "Query: {}\nGiven the video and the query, find the relevant windows.\nRelevant windows: "
QUERIES = [["a person opens the door.", "someone sits down on the sofa and reads", "a dog barks"], ["the light is switched off", "a cat"]]
WINDOWS = [["[[2, 4]]", "[[0, 0], [6, 6]]", "[[4, 6]]"], ["[[0, 2]]", "[[2, 6]]"]]
T = 4


def _grouped_batch():
    g = torch.Generator().manual_seed(2)
    return {"video_embeds": torch.randn(2, T, 257, 1408, generator=g), "audio_embeds": torch.randn(2, T, 256, 768, generator=g),
            "text_input": [[PROMPT.format(q) for q in qs] for qs in QUERIES], "text_output": WINDOWS,
            "timestamps": [list(range(0, 2 * T, 2)), [1, 3, 105, 7]], "duration": [2 * T, 110]}


def _flatten(batch, pairs):
    """One sample per (video, query) pair."""
    vid = [b for b, _ in pairs]
    return {"video_embeds": batch["video_embeds"][vid], "audio_embeds": batch["audio_embeds"][vid],
            "text_input": [batch["text_input"][b][p] for b, p in pairs], "text_output": [batch["text_output"][b][p] for b, p in pairs],
            "timestamps": [batch["timestamps"][b] for b in vid], "duration": [batch["duration"][b] for b in vid]}


ALL_PAIRS = [(b, p) for b, qs in enumerate(QUERIES) for p in range(len(qs))]


@pytest.fixture(scope="module")
def lm(dev):
    return _tiny_llama(dev)


@pytest.fixture(scope="module")
def full(dev, lm):
    """Everything trains together: LoRA adapters (no dropout, so two forwards see the same LM), Q-Formers, query tokens, projections.  The
    tests below leave the weights alone until the training test, which runs last."""
    model = _model(dev, *lm)
    model.enable_lora(dropout=0.0)
    model.enable_qformer_training(train_proj=True)
    model.objective = "llm"
    model.compat_repeat = False
    model.grouped_lm = True
    return model


def _zero(model):
    for p in model.lora_parameters() + [q for m in model.modalities for q in getattr(model, f"{m}_llm_proj").parameters()]:
        p.grad = None
    for m in model.modalities:
        getattr(model, f"{m}_Qformer")._grad_flat.zero_()


def _grads(model):
    torch.cuda.synchronize()
    out = {}
    for m in model.modalities:
        out[f"{m}.qformer"] = getattr(model, f"{m}_Qformer")._grad_flat.clone()
        out[f"{m}.query_tokens"] = getattr(model, f"{m}_query_tokens").grad.clone()
        out[f"{m}.proj.weight"] = getattr(model, f"{m}_llm_proj").weight.grad.clone()
        out[f"{m}.proj.bias"] = getattr(model, f"{m}_llm_proj").bias.grad.clone()
    lora = [p.grad for p in model.lora_parameters()]
    out["lora"] = torch.cat([g.reshape(-1).float() for g in lora if g is not None])
    return out


def _within_bars(got, want, what):
    rel_bar, peak_bar = 2 * MT.BARS[torch.bfloat16][0], 2 * MT.BARS[torch.bfloat16][1]        # both sides carry 16-bit noise
    worst = (0.0, 0.0)
    for k, ref in want.items():
        assert ref.abs().max().item() > 0 and torch.isfinite(got[k]).all().item(), (what, k)
        rel = ((got[k] - ref).norm() / ref.norm()).item()
        peak = ((got[k] - ref).abs().max() / ref.abs().max()).item()
        print(f"{what}: {k}: relative Frobenius {rel:.3e} (bar {rel_bar:.1e}) peak {peak:.3e} (bar {peak_bar:.1e})")
        worst = (max(worst[0], rel / rel_bar), max(worst[1], peak / peak_bar))
        assert rel < rel_bar and peak < peak_bar, (what, k, rel, peak)
    print(f"{what}: worst ratios to the bars: relative {worst[0]:.3e}, peak {worst[1]:.3e}")


def _labelled(model, samples):
    plan = model.prompt_assembler.plan_forward(samples, num=T)
    return int((plan.targets[:, 1:] != -100).sum())


def test_switch_gives_the_same_loss_bits_frozen_lora(dev, lm):
    model = _model(dev, *lm)
    model.enable_lora(dropout=0.0)
    model.objective = "llm"
    batch = _batch(dev)
    losses = {}
    for route in ("cat", "plan", "cat"):
        model.prompt_assembly = route
        loss = model(batch)["loss"]
        assert loss.requires_grad
        loss.backward()
        losses.setdefault(route, []).append(loss.detach().clone())
    assert torch.equal(losses["cat"][0], losses["cat"][1]) and torch.equal(losses["cat"][0], losses["plan"][0]), losses
    model.objective = "both"                                       # the frozen branch of forward
    both = {}
    for route in ("cat", "plan"):
        model.prompt_assembly = route
        both[route] = model(batch)
    assert torch.equal(both["cat"]["loss"], both["plan"]["loss"]) and torch.equal(both["cat"]["loss_lm"], both["plan"]["loss_lm"])
    gen = {}
    for route in ("cat", "plan"):
        model.prompt_assembly = route
        gen[route] = model.generate_llm(batch, max_new_tokens=4)
    assert gen["cat"] == gen["plan"] and len(gen["cat"]) == 2


def test_switch_gives_the_same_loss_bits_with_trained_qformers(dev, full):
    model, batch = full, _batch(dev)
    out = {}
    try:
        for route in ("cat", "plan"):
            model.prompt_assembly = route
            _zero(model)
            loss = model(batch)["loss"]
            loss.backward()
            out[route] = (loss.detach().clone(), _grads(model))
    finally:
        model.prompt_assembly = "cat"
    assert torch.equal(out["cat"][0], out["plan"][0]), (out["cat"][0].item(), out["plan"][0].item())
    _within_bars(out["plan"][1], out["cat"][1], "plan against cat")            # (the same d_embeds rows arrive; only the LM's backward could differ)


def test_grouped_equals_flattened(dev, full):
    model, batch = full, _grouped_batch()
    flat = _flatten(batch, ALL_PAIRS)
    _zero(model)
    want = model.forward_llm(flat)["loss"]
    want.backward()
    want_g = _grads(model)
    seen = []
    model._lm_probe = seen.append
    try:
        _zero(model)
        got = model(batch)["loss"]                             # list-valued text_input and objective "llm": the grouped LM pass
    finally:
        model._lm_probe = None
    got.backward()
    got_g = _grads(model)
    assert abs(got.item() - want.item()) <= 1e-3 * max(1.0, abs(want.item())), (got.item(), want.item())
    print(f"grouped {got.item():.6f} flattened {want.item():.6f}")
    _within_bars(got_g, want_g, "grouped against flattened")
    a = model.forward_llm(batch)["loss"]                        # forward_llm takes the grouped batch the same way
    assert abs(a.item() - got.item()) <= 1e-6 * abs(got.item())
    # what went into the LM: the cat-route assembly of the flattened batch over projections of the SAME z, bit for bit
    assert len(seen) == 1
    probe = seen[0]
    call = probe["call"]
    assert call["pairs"] == ALL_PAIRS and call["P"] == 3
    inputs = {}
    with torch.no_grad():
        for m, (z, _) in call["out"].items():
            zz = z.detach().view(2, T, 3, 32, -1)
            picked = torch.stack([zz[k, :, p] for k, p in ALL_PAIRS]).reshape(len(ALL_PAIRS) * T, 32, -1)
            y = getattr(model, f"{m}_Qformer").llm_proj(picked).reshape(len(ALL_PAIRS), T * 32, -1)
            inputs[m] = y.to(torch.bfloat16)
        atts = {m: torch.ones(v.shape[:2], dtype=torch.long, device=dev) for m, v in inputs.items()}
        embeds, mask, targets = model.prompt_assembler.assemble_forward(flat, inputs, atts)
    assert torch.equal(_bits(probe["embeds"]), _bits(embeds)) and torch.equal(probe["mask"], mask) and torch.equal(probe["targets"], targets)


def test_two_calls_are_the_token_weighted_sum(dev, full):
    model, batch = full, _grouped_batch()
    first, second = [(0, 0), (0, 1), (1, 0), (1, 1)], [(0, 2)]
    fa, fb = _flatten(batch, first), _flatten(batch, second)
    na, nb = _labelled(model, fa), _labelled(model, fb)
    assert na == sum(len(WINDOWS[b][p]) + 1 for b, p in first) and nb == len(WINDOWS[0][2]) + 1
    _zero(model)
    want = (model.forward_llm(fa)["loss"] * na + model.forward_llm(fb)["loss"] * nb) / (na + nb)
    want.backward()
    want_g = _grads(model)
    model.max_queries_per_call = 2
    try:
        _zero(model)
        got = model(batch)["loss"]
        got.backward()
        got_g = _grads(model)
    finally:
        model.max_queries_per_call = 8
    assert abs(got.item() - want.item()) <= 1e-3 * max(1.0, abs(want.item())), (got.item(), want.item())
    _within_bars(got_g, want_g, "two calls against two flattened calls")


def test_both_objectives_over_one_qformer_backward_per_call(dev, full):
    model, batch = full, _grouped_batch()
    model.lm_weight = 0.5
    bce = model.forward_multi(batch)["loss"].item()
    lm = model.forward_llm(batch)["loss"].item()
    model.objective = "both"
    calls, fwd = {}, {}
    restore = []
    for m in model.modalities:
        qf = getattr(model, f"{m}_Qformer")
        inner_b, inner_f = qf._run_backward, qf.forward_multi_train
        restore.append((qf, inner_b, inner_f))

        def counted_b(*a, _m=m, _inner=inner_b, **kw):
            calls[_m] = calls.get(_m, 0) + 1
            return _inner(*a, **kw)

        def counted_f(*a, _m=m, _inner=inner_f, **kw):
            fwd[_m] = fwd.get(_m, 0) + 1
            return _inner(*a, **kw)

        qf._run_backward, qf.forward_multi_train = counted_b, counted_f
    try:
        _zero(model)
        out = model(batch)
        out["loss"].backward()
        torch.cuda.synchronize(dev)
        assert fwd == {"video": 1, "audio": 1} and calls == {"video": 1, "audio": 1}, (fwd, calls)
        model.max_queries_per_call = 2
        fwd.clear(), calls.clear()
        out2 = model(batch)
        out2["loss"].backward()
        torch.cuda.synchronize(dev)
        assert fwd == {"video": 2, "audio": 2} and calls == {"video": 2, "audio": 2}, (fwd, calls)
    finally:
        model.max_queries_per_call, model.objective, model.lm_weight = 8, "llm", 1.0
        for qf, b, f in restore:
            qf._run_backward, qf.forward_multi_train = b, f
    want = bce + 0.5 * lm
    assert abs(out["loss"].item() - want) <= 1e-6 * abs(want), (out["loss"].item(), bce, lm)
    assert abs(out["loss_score"].item() - bce) <= 1e-6 * abs(bce) and abs(out["loss_lm"].item() - lm) <= 1e-6 * abs(lm)
    assert abs(out2["loss_score"].item() - bce) <= 1e-3 * max(1.0, abs(bce)) and abs(out2["loss_lm"].item() - lm) <= 1e-3 * max(1.0, abs(lm))


def test_grouped_frozen_lora_regime_and_lm_loss_routes(dev, lm):
    """Only the adapters train: the Q-Former side runs ``forward_multi`` under no_grad, the loss reaches the adapters; every ``lm_loss``
    route and ``loss_scale`` work on the grouped pass as on the ordinary one."""
    model = _model(dev, *lm)
    model.enable_lora(dropout=0.0)
    model.objective, model.compat_repeat, model.grouped_lm = "llm", False, True
    batch = _grouped_batch()
    want = model.forward_llm(_flatten(batch, ALL_PAIRS))["loss"]
    losses = {}
    for route in ("stock", "rows", "fused"):
        model.lm_loss = route
        loss = model(batch)["loss"]
        assert loss.requires_grad
        losses[route] = loss.item()
        assert abs(loss.item() - want.item()) <= 1e-3 * max(1.0, abs(want.item())), (route, loss.item(), want.item())
    model.lm_loss, model.loss_scale = "stock", 1024.0
    for p in model.lora_parameters():
        p.grad = None
    scaled = model(batch)["loss"]
    scaled.backward()
    torch.cuda.synchronize(dev)
    assert scaled.item() == losses["stock"]
    g = [p.grad for p in model.lora_parameters() if p.grad is not None]
    assert g and all(torch.isfinite(x).all() for x in g) and sum(x.abs().sum().item() for x in g) > 0
    model.objective = "both"
    out = model(batch)
    assert not out["loss_score"].requires_grad and out["loss"].requires_grad and set(out) == {"loss", "loss_score", "loss_lm"}


def test_generate_multi_llm_is_generate_llm_on_the_flattened_batch(dev, lm):
    model = _model(dev, *lm)
    model.compat_repeat = False
    batch = _grouped_batch()
    texts = model.generate_multi_llm(batch, batch["text_input"], max_new_tokens=6)
    assert [len(t) for t in texts] == [3, 2] and all(isinstance(s, str) for t in texts for s in t)
    want = model.generate_llm(_flatten(batch, ALL_PAIRS), max_new_tokens=6)
    print("generate_multi_llm:", texts, "generate_llm on the flattened batch:", want)
    assert [s for t in texts for s in t] == want
    model.max_queries_per_call = 2
    assert model.generate_multi_llm(batch, max_new_tokens=6) == texts


def test_defaults_give_the_parents_bits(dev, lm):
    """A model that went through the plan, the grouped LM pass and back against a model of the same seed that never saw them: the default
    arguments give the same bits on every path that existed before."""
    plain, touched = _model(dev, *lm), _model(dev, *lm)
    from mraudio_amd._lib import MraError

    assert plain.prompt_assembly == "cat" and plain.grouped_lm is False
    batch, grouped = _batch(dev), _grouped_batch()
    for model in (plain, touched):
        model.enable_qformer_training()
    for objective in ("llm", "both"):            # the grouped LM pass is opt-in: with the default such a batch is refused as it always was
        plain.objective = objective
        with pytest.raises(MraError, match="multi-query"):
            plain(grouped)
    plain.objective = "score"
    touched.objective, touched.prompt_assembly, touched.grouped_lm = "both", "plan", True
    touched(batch)
    touched(grouped)
    touched.objective, touched.prompt_assembly, touched.grouped_lm = "score", "cat", False
    assert torch.equal(plain(batch)["loss"], touched(batch)["loss"])
    assert torch.equal(plain(grouped)["loss"], touched(grouped)["loss"])           # forward_multi over the shared pass
    assert torch.equal(plain.forward_llm(batch)["loss"], touched.forward_llm(batch)["loss"])
    assert torch.equal(plain.forward_llm(batch, train=True)["loss"], touched.forward_llm(batch, train=True)["loss"])
    assert plain.generate_llm(batch, max_new_tokens=4) == touched.generate_llm(batch, max_new_tokens=4)
    with pytest.raises(ValueError, match="prompt_assembly"):
        _model(dev, *lm, prompt_assembly="gather")


def test_three_adam_steps_on_a_grouped_batch_lower_the_lm_loss(dev, full):
    model, batch = full, _grouped_batch()
    opt = torch.optim.Adam(model.flat_optimizer_params() + model.lora_parameters(), lr=1e-4, fused=True)
    losses = []
    for it in range(4):
        opt.zero_grad(set_to_none=False)
        loss = model(batch)["loss"]
        assert torch.isfinite(loss)
        losses.append(loss.item())
        if it == 3:
            break
        loss.backward()
        opt.step()
    print("grouped LM loss over three fused-Adam steps:", losses)
    assert losses[3] < losses[0], losses


def test_trainer_takes_group_by_video_with_an_lm_objective(dev, lm, tmp_path):
    from mraudio_amd.utils.trainer import Trainer, default_args

    model = _model(dev, *lm)
    args = default_args(output_dir=str(tmp_path), gpu=0, synthetic=2, synthetic_queries=3, dataset="Charades_STA", lr=2e-5, warmup_steps=1,
                        objective="both", train_proj=True, group_by_video=True, max_queries_per_call=2, prompt_assembly="plan", max_epoch=1,
                        val_freq=5)
    tr = Trainer(args, model=model)
    assert model.prompt_assembly == "plan" and tr.group_by_video and model.objective == "both" and model.grouped_lm is True
    tr.train()
    assert len(tr.history) == 1 and torch.isfinite(torch.tensor(tr.history[0]["loss_value"]))
    with pytest.raises(ValueError, match="prompt_assembly"):
        Trainer(default_args(output_dir=str(tmp_path), gpu=0, synthetic=2, prompt_assembly="plan"), model=model)     # objective "score"
