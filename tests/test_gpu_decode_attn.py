"""The one-token attention on the GPU (``-m gpu``): ``mra_decode_attention`` on every element of out and lse against float64 under the DERIVED
bounds of tests/decode_attn_cases.py -- K / V as views of a longer, poisoned buffer, q / out with padded head strides, sentinel guards around
out, lse and the workspace and between the output rows, two runs bit for bit, ``lse = NULL`` -- and the decode of the tiny bf16 Llama of
tests/test_gpu_llm_objective.py (and a second one with two K/V heads) through it.

Bars of the model level.  (i) Every one-token call a real ``generate`` makes is held to the case file's bound around the float64 reference of
those very tensors, on the stock trajectory.  (ii) Greedy strings of two routes cannot be compared for equality: near-ties flip under 16-bit
rounding.  With L32 the teacher-forced logits of an fp32 copy of the same weights and d_stock = max |L_stock_bf16 - L32| measured here, a
route's token may give away at most 2 d_stock of fp32 logit to the fp32 argmax at every step -- two routes are two draws of rounding noise of
the same order; the stock route is held to the same bar, which guards the bar itself."""
import copy

import pytest
import torch

import decode_attn_cases as DC
from mraudio_amd import _lib
from mraudio_amd.models import lm_decode as LD
from test_gpu_llm_objective import LH, _batch, _model, _tiny_llama

pytestmark = pytest.mark.gpu

GUARD = 64                       # elements on either side of every output (a multiple of 8: the views stay 16-byte aligned)
SENT = 77.0                      # exact in f16, bf16 and fp32
WS_GUARD, WS_SENT = 256, 0xA5    # bytes on either side of the workspace


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _id(dt):
    return "f16" if dt == torch.float16 else "bf16"


def _run(dev, case, dtype, want_lse=True):
    """One call of the entry on guarded, strided buffers: (out [B, Hq, D], lse [B, Hq] or None) on the device, after the guard checks."""
    B, Hq, Hkv, S, D, _ = case
    lib, stream = _lib.lib(), _lib.current_stream()
    c, lay = DC.make_case(*case, dtype), DC.layout(B, Hq, Hkv, S, D)
    Smax, k_ss, v_ss, q_sh, o_sh = lay["Smax"], lay["k_ss"], lay["v_ss"], lay["q_sh"], lay["o_sh"]
    qbuf = torch.full((2 * GUARD + B * Hq * q_sh,), float("nan"), dtype=dtype, device=dev)
    q = qbuf[GUARD: GUARD + B * Hq * q_sh].view(B, Hq, q_sh)[:, :, :D]
    q.copy_(c["q"])
    kbuf = torch.full((B, Hkv, Smax, k_ss), float("nan"), dtype=dtype, device=dev)       # everything past S and past D: NaN / Inf
    vbuf = torch.full((B, Hkv, Smax, v_ss), float("-inf"), dtype=dtype, device=dev)
    k, v = kbuf[:, :, :S, :D], vbuf[:, :, :S, :D]
    k.copy_(c["k"])
    v.copy_(c["v"])
    obuf = torch.full((2 * GUARD + B * Hq * o_sh,), SENT, dtype=dtype, device=dev)
    out = obuf[GUARD: GUARD + B * Hq * o_sh].view(B, Hq, o_sh)[:, :, :D]
    lbuf = torch.full((2 * GUARD + B * Hq,), SENT, dtype=torch.float32, device=dev)
    lse = lbuf[GUARD: GUARD + B * Hq]
    mask, m_sb = None, 0
    if c["mask"] is not None:
        m_sb = S + 3
        mask = torch.ones(B, m_sb, dtype=torch.uint8, device=dev)                         # the bytes past S say "attend": they must not be read
        mask[:, :S] = c["mask"].to(dev).to(torch.uint8) * (1 + 6 * (S % 2))               # any nonzero byte attends
    nbytes = int(lib.mra_decode_attention_workspace_bytes(B, Hq, S, D))
    assert nbytes == DC.workspace_bytes(B, Hq, S, D)
    wbuf = torch.full((2 * WS_GUARD + nbytes,), WS_SENT, dtype=torch.uint8, device=dev)
    ws = wbuf[WS_GUARD: WS_GUARD + nbytes]
    for t in (q, k, v, out, ws):
        assert t.data_ptr() % 16 == 0
    _lib.check(lib.mra_decode_attention(_lib.ptr(q), Hq * q_sh, q_sh, _lib.ptr(k), k.stride(0), k.stride(1), k_ss, _lib.ptr(v), v.stride(0), v.stride(1), v_ss,
                                        None if mask is None else _lib.ptr(mask), m_sb, B, Hq, Hkv, S, D, _lib.mra_dtype(dtype), c["scale"], _lib.ptr(out),
                                        Hq * o_sh, o_sh, _lib.ptr(lse) if want_lse else None, _lib.ptr(ws), nbytes, stream), "decode_attention")
    body = obuf[GUARD: GUARD + B * Hq * o_sh].view(B * Hq, o_sh)
    assert bool((obuf[:GUARD] == SENT).all() and (obuf[GUARD + B * Hq * o_sh:] == SENT).all() and (body[:, D:] == SENT).all()), case
    assert bool((lbuf[:GUARD] == SENT).all() and (lbuf[GUARD + B * Hq:] == SENT).all()), case
    assert bool((wbuf[:WS_GUARD] == WS_SENT).all() and (wbuf[WS_GUARD + nbytes:] == WS_SENT).all()), case
    if not want_lse:
        assert bool((lse == SENT).all()), case
    assert torch.equal(q.cpu().view(torch.int16), c["q"].view(torch.int16)) and torch.equal(k.cpu().view(torch.int16), c["k"].view(torch.int16))
    return out.clone(), lse.view(B, Hq).clone() if want_lse else None


@pytest.mark.parametrize("dtype", DC.DTYPES, ids=_id)
def test_entry_against_float64(dev, dtype):
    worst = [0.0, 0.0]
    for case in DC.cases():
        out, lse = _run(dev, case, dtype)
        r = DC.ratios(*case, dtype, out, lse)
        print(f"decode_attention {_id(dtype)} {case}: |d| / bound out {r[0]:.3g} lse {r[1]:.3g}")
        assert max(r) <= 1.0, (case, r)
        worst = [max(a, b) for a, b in zip(worst, r)]
        out2, lse2 = _run(dev, case, dtype)                                           # two runs, the same bits
        assert torch.equal(out.view(torch.int16), out2.view(torch.int16)) and torch.equal(lse.view(torch.int32), lse2.view(torch.int32)), case
        out0, _ = _run(dev, case, dtype, want_lse=False)                              # lse = NULL: the same out bits
        assert torch.equal(out.view(torch.int16), out0.view(torch.int16)), case
    print(f"decode_attention {_id(dtype)}: worst |d| / bound out {worst[0]:.3g} lse {worst[1]:.3g}")
    assert all(w > 0.0 for w in worst)


def test_zero_batch_touches_nothing(dev):
    lib, stream = _lib.lib(), _lib.current_stream()
    out = torch.full((64,), SENT, device=dev)
    assert lib.mra_decode_attention_workspace_bytes(0, 4, 9, 64) == 0
    assert lib.mra_decode_attention(None, 0, 0, None, 0, 0, 0, None, 0, 0, 0, None, 0, 0, 4, 4, 9, 64, _lib.MRA_BF16, 1.0, _lib.ptr(out), 0, 0,
                                    _lib.ptr(out), None, 0, stream) == 0
    torch.cuda.synchronize(dev)
    assert bool((out == SENT).all())


@pytest.mark.parametrize("dtype", DC.DTYPES, ids=_id)
def test_python_entry_takes_the_kernel_on_views_and_the_torch_ops_otherwise(dev, dtype):
    case = (3, 8, 2, 515, 128, "holes")
    B, Hq, Hkv, S, D, _ = case
    c, ref = DC.make_case(*case, dtype), DC.reference(*case, dtype)
    cache_k = torch.full((B, Hkv, S + 40, D), float("nan"), dtype=dtype, device=dev)      # the static-cache form
    cache_v = torch.full((B, Hkv, S + 40, D), float("inf"), dtype=dtype, device=dev)
    cache_k[:, :, :S], cache_v[:, :, :S] = c["k"].to(dev), c["v"].to(dev)
    q = c["q"].to(dev)[:, :, None, :]
    mask = c["mask"].to(dev)[:, None, None, :]
    hip = LD.decode_attention(q, cache_k[:, :, :S], cache_v[:, :, :S], mask, c["scale"], hip=True)
    ops = LD.decode_attention(q, cache_k[:, :, :S], cache_v[:, :, :S], mask, c["scale"], hip=False)
    assert hip.shape == ops.shape == (B, Hq, 1, D) and hip.dtype == ops.dtype == dtype
    assert max(DC.ratios_against(ref, hip[:, :, 0], None)) <= 1.0 and max(DC.ratios_against(ref, ops[:, :, 0], None)) <= 1.0
    assert torch.equal(LD.decode_attention(q, cache_k[:, :, :S], cache_v[:, :, :S], mask, c["scale"]), hip)       # hip=None: the entry
    # the whole cache with the tail masked instead of sliced away, as generate hands it over
    full = torch.cat([mask, torch.zeros(B, 1, 1, 40, dtype=torch.bool, device=dev)], 3)
    got =LD.decode_attention(q, cache_k, cache_v, full, c["scale"], hip=True)
    assert max(DC.ratios_against(ref, got[:, :, 0], None)) <= 1.0
    # what the entry does not take goes to the torch ops under hip=None and raises under hip=True
    q32 = q.float()
    assert LD.decode_attention(q32, cache_k[:, :, :S].float(), cache_v[:, :, :S].float(), mask, c["scale"]).dtype == torch.float32
    with pytest.raises(_lib.MraError, match="16-bit"):
        LD.decode_attention(q32, cache_k[:, :, :S].float(), cache_v[:, :, :S].float(), mask, c["scale"], hip=True)
    with pytest.raises(_lib.MraError, match="outside"):
        LD.decode_attention(q[..., :32], cache_k[:, :, :S, :32], cache_v[:, :, :S, :32], mask, c["scale"], hip=True)
    odd = LD.decode_attention(q[..., :32], cache_k[:, :, :S, :32], cache_v[:, :, :S, :32], mask, c["scale"])
    assert odd.shape == (B, Hq, 1, 32) and torch.isfinite(odd).all()


# ---- the model ----------------------------------------------------------------------------------------------------------------------------------
N_NEW, PREFIX = 24, 300


def _llama(dev, kv_heads):
    llm, tok = _tiny_llama(dev)
    if kv_heads != llm.config.num_key_value_heads:
        import transformers as tf

        torch.manual_seed(1)
        cfg = copy.deepcopy(llm.config)
        cfg.num_key_value_heads = kv_heads
        llm = tf.LlamaForCausalLM(cfg).to(dev).to(torch.bfloat16).eval().requires_grad_(False)
    return llm, tok


def _prefix(dev):
    """B = 3 prefixes of PREFIX embedded rows: left padding in one sequence, holes inside another."""
    gen = torch.Generator().manual_seed(12)
    embeds = (torch.randn(3, PREFIX, LH, generator=gen) * 0.5).to(torch.bfloat16).to(dev)
    mask = torch.ones(3, PREFIX, dtype=torch.long)
    mask[1, :37] = 0
    mask[2, 11:19] = 0
    mask[2, 150:163] = 0
    mask[1, 200] = 0
    return embeds, mask.to(dev)


def _generate(llm, embeds, mask, impl=None):
    kw = dict(inputs_embeds=embeds, attention_mask=mask, max_new_tokens=N_NEW, min_new_tokens=N_NEW, do_sample=False)     # no sequence stops early
    if impl is None:
        return llm.generate(**kw)
    before = llm.config._attn_implementation
    llm.set_attn_implementation(impl)
    try:
        return llm.generate(cache_implementation="static", disable_compile=True, **kw)
    finally:
        llm.set_attn_implementation(before)


@pytest.mark.parametrize("kv_heads", [4, 2])
def test_every_one_token_call_of_generate_is_inside_the_bound(dev, kv_heads):
    from transformers import AttentionInterface
    from transformers.integrations.sdpa_attention import sdpa_attention_forward
    from transformers.masking_utils import AttentionMaskInterface, sdpa_mask

    llm, _ = _llama(dev, kv_heads)
    embeds, mask = _prefix(dev)
    seen = []

    def shadow(module, query, key, value, attention_mask, dropout=0.0, scaling=None, **kw):
        """Both results on every one-token call; the SDPA one is returned, so the trajectory is the stock one."""
        if query.shape[2] == 1:
            assert attention_mask.dtype == torch.bool and tuple(attention_mask.shape) == (3, 1, 1, key.shape[2]) and key.shape[1] == kv_heads
            scale = float(scaling) if scaling is not None else query.shape[3] ** -0.5
            hip = LD.decode_attention(query, key, value, attention_mask, scale, hip=True)
            ref = DC.reference_tensors(query[:, :, 0].cpu(), key.cpu(), value.cpu(), attention_mask[:, 0, 0].cpu(), scale, torch.bfloat16)
            seen.append((max(DC.ratios_against(ref, hip[:, :, 0], None)), key.shape[2], int(attention_mask.sum())))
        return sdpa_attention_forward(module, query, key, value, attention_mask, dropout=dropout, scaling=scaling, **kw)

    AttentionInterface.register("mra_decode_shadow", shadow)
    AttentionMaskInterface.register("mra_decode_shadow", sdpa_mask)
    stock = _generate(llm, embeds, mask)
    got = _generate(llm, embeds, mask, impl="mra_decode_shadow")
    assert got.shape == (3, N_NEW)
    assert len(seen) == llm.config.num_hidden_layers * (N_NEW - 1)
    worst = max(r for r, _, _ in seen)
    print(f"kv heads {kv_heads}: {len(seen)} one-token calls over a cache of {seen[0][1]} slots, {seen[0][2]} .. {seen[-1][2]} attended; worst |d| / bound "
          f"{worst:.3g}; static-cache SDPA tokens equal the stock route's: {torch.equal(got, stock)}")
    assert worst <= 1.0 and seen[0][1] >= PREFIX + N_NEW - 1


def _teacher_forced(model, embeds, mask, tokens):
    """fp32 logits [B, N_NEW, V] that predict ``tokens`` from one uncached forward over prefix + tokens."""
    emb = model.get_input_embeddings()(tokens).to(embeds.dtype if model.dtype != torch.float32 else torch.float32)
    x = torch.cat([embeds.to(emb.dtype), emb], 1)
    m = torch.cat([mask, torch.ones_like(tokens)], 1)
    logits = model(inputs_embeds=x, attention_mask=m, return_dict=True).logits
    return logits[:, PREFIX - 1: PREFIX - 1 + N_NEW].float()


@pytest.mark.parametrize("kv_heads", [4, 2])
def test_hip_route_tokens_are_argmax_up_to_rounding_ties(dev, kv_heads):
    llm, _ = _llama(dev, kv_heads)
    llm32 = copy.deepcopy(llm).float()
    embeds, mask = _prefix(dev)
    with torch.no_grad():
        stock = _generate(llm, embeds, mask)
        hip = _generate(llm, embeds, mask, impl=LD.register())
        L32_stock = _teacher_forced(llm32, embeds, mask, stock)
        d_stock = (_teacher_forced(llm, embeds, mask, stock) - L32_stock).abs().max().item()
        gaps = {}
        for name, toks, L32 in (("stock", stock, L32_stock), ("hip", hip, _teacher_forced(llm32, embeds, mask, hip))):
            gaps[name] = (L32.max(2).values - L32.gather(2, toks[:, :, None]).squeeze(2)).max().item()
    same = int((stock == hip).sum())
    print(f"kv heads {kv_heads}: d_stock {d_stock:.4g} (logit scale {L32_stock.abs().max().item():.3g}); worst fp32 gap to the argmax: stock "
          f"{gaps['stock']:.4g}, hip {gaps['hip']:.4g} (bar 2 d_stock = {2 * d_stock:.4g}); {same} of {stock.numel()} tokens equal")
    assert d_stock > 0
    assert gaps["stock"] <= 2 * d_stock and gaps["hip"] <= 2 * d_stock


def test_generate_llm_hip_leaves_the_lm_as_it_was(dev, monkeypatch):
    llm, tok = _tiny_llama(dev)
    model = _model(dev, llm, tok)
    batch = _batch(dev)
    tokens, kws = [], []
    real = llm.generate

    def generate(**kw):
        kws.append({k: v for k, v in kw.items() if not torch.is_tensor(v)})
        tokens.append(real(**kw).clone())
        return tokens[-1].clone()

    monkeypatch.setattr(llm, "generate", generate)
    routed = []
    real_decode = LD.decode_attention
    monkeypatch.setattr(LD, "decode_attention", lambda *a, **k: routed.append(a[0].is_cuda) or real_decode(*a, **k))
    before = llm.config._attn_implementation
    first = model.generate_llm(batch, max_new_tokens=12)
    assert not routed
    model.lm_decode = "hip"
    hip = model.generate_llm(batch, max_new_tokens=12)
    assert routed and all(routed) and llm.config._attn_implementation == before
    assert kws[1] == dict(max_new_tokens=12, cache_implementation="static", disable_compile=True)
    n = len(routed)
    model.lm_decode = "stock"
    again = model.generate_llm(batch, max_new_tokens=12)
    assert len(routed) == n and kws[2] == kws[0] == dict(max_new_tokens=12)
    assert torch.equal(tokens[0], tokens[2]) and again == first and len(hip) == len(first)
    print(f"generate_llm: hip strings equal the stock ones: {hip == first}")
    model.compat_repeat = False
    multi_stock = model.generate_multi_llm({**batch, "text_input": [[t, t + " again"] for t in batch["text_input"]]}, max_new_tokens=4)
    model.lm_decode = "hip"
    n = len(routed)
    multi_hip = model.generate_multi_llm({**batch, "text_input": [[t, t + " again"] for t in batch["text_input"]]}, max_new_tokens=4)
    assert len(routed) > n and [len(x) for x in multi_hip] == [len(x) for x in multi_stock] == [2, 2]
    assert llm.config._attn_implementation == before


def test_trainer_validates_on_lm_decoded_strings(dev, tmp_path):
    from mraudio_amd.eval.mr_eval import eval_submission
    from mraudio_amd.utils.mr_dataset import prepare_sample
    from mraudio_amd.utils.spans import moment_str_to_list, post_process
    from mraudio_amd.utils.trainer import Trainer, default_args

    llm, tok = _tiny_llama(dev)
    model = _model(dev, llm, tok)
    kw = dict(output_dir=str(tmp_path), gpu=0, synthetic=4, dataset="Charades_STA", max_epoch=1)
    with pytest.raises(_lib.MraError, match="LM attached"):
        from mraudio_amd.models.xinstructblip import XInstructBLIP
        Trainer(default_args(val_decode="llm", **kw), model=XInstructBLIP(seed=0, perturb=True, device=dev, llm_hidden_size=LH, op_dtype=torch.bfloat16))
    tr = Trainer(default_args(val_decode="llm", lm_decode="hip", **kw), model=model)
    assert model.lm_decode == "hip"
    calls = []
    real = model.generate_llm
    model.generate_llm = lambda samples, **k: calls.append(len(samples["text_input"])) or real(samples, **k)
    got = tr.eval_epoch()
    model.generate_llm = real
    assert calls == [1, 1]
    results = []
    with torch.no_grad():
        for samples in tr.val_dataloader:
            samples = prepare_sample(samples, dev)
            for qid, query, vid, target, out in zip(samples["qid"], samples["query"], samples["vid"], samples["text_output"], model.generate_llm(samples)):
                results.append({"qid": qid, "query": query, "vid": vid, "relevant_windows": moment_str_to_list(post_process(target)),
                                "pred_relevant_windows": moment_str_to_list(post_process(out))})
    want = eval_submission(results, results, verbose=False)
    assert got["brief"] == want["brief"] and "MR-full-R1-avg" in got["brief"]
    assert llm.config._attn_implementation != "mra_decode"
