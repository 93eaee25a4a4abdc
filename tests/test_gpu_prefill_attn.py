"""The causal grouped-query attention of the LM's prefill on the GPU (``-m gpu``): ``mra_prefill_attention`` on every element of out and lse
against float64 under the DERIVED bounds of tests/prefill_attn_cases.py -- q as a transposed view, K / V as views of a longer, poisoned buffer,
out with padded position and head strides, sentinel guards around out and lse and between the output rows, two runs bit for bit,
``lse = NULL`` -- the last query row against ``mra_decode_attention``, every attention call of a real prefill of the tiny Llamas of
tests/test_gpu_lm_step.py, and the decode behind it end to end (the criterion of tests/test_gpu_decode_attn.py: a token may give away at most
2 d_stock of fp32 logit to the fp32 argmax, d_stock measured here against an fp32 copy of the same weights)."""
import copy

import pytest
import torch

import decode_attn_cases as DC
import prefill_attn_cases as PC
from mraudio_amd import _lib
from mraudio_amd.models import lm_decode as LD
from mraudio_amd.models import lm_step as LS
from test_gpu_llm_objective import LH, _batch, _model, _tiny_llama
from test_gpu_lm_step import N_NEW, PREFIX, _llama, _prefix, _teacher_forced

pytestmark = pytest.mark.gpu

GUARD = 64                       # elements on either side of every output (a multiple of 8: the views stay 16-byte aligned)
SENT = 77.0                      # exact in f16, bf16 and fp32
CASES = PC.cases()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _id(dt):
    return "f16" if dt == torch.float16 else "bf16"


def _operands(dev, case, dtype):
    """q as the transposed view of [B, Sq, Hq, D]; K / V as views of a longer, pitched buffer whose rest is NaN / -Inf; the mask bytes."""
    B, Hq, Hkv, Sq, Skv, off, D, _ = case
    c, lay = PC.make_case(*case, dtype), PC.layout(Hq, Sq, Skv, D)
    q = c["q"].to(dev).transpose(1, 2).contiguous().transpose(1, 2)                       # [B, Hq, Sq, D] with strides (Sq Hq D, D, Hq D, 1)
    kbuf = torch.full((B, Hkv, lay["Smax"], lay["k_ss"]), float("nan"), dtype=dtype, device=dev)
    vbuf = torch.full((B, Hkv, lay["Smax"], lay["v_ss"]), float("-inf"), dtype=dtype, device=dev)
    k, v = kbuf[:, :, :Skv, :D], vbuf[:, :, :Skv, :D]
    k.copy_(c["k"])
    v.copy_(c["v"])
    mask, m_sb = None, 0
    if c["mask"] is not None:
        m_sb = Skv + 3
        mask = torch.ones(B, m_sb, dtype=torch.uint8, device=dev)                         # the bytes past Skv say "attend": they must not be read
        mask[:, :Skv] = c["mask"].to(dev).to(torch.uint8) * (1 + 6 * (Skv % 2))           # any nonzero byte attends
    return c, lay, q, k, v, mask, m_sb


def _run(dev, case, dtype, want_lse=True):
    """One call of the entry on guarded, strided buffers: (out [B, Sq, Hq, D], lse [B, Hq, Sq] or None) on the device, after the guard checks."""
    B, Hq, Hkv, Sq, Skv, off, D, _ = case
    lib, stream = _lib.lib(), _lib.current_stream()
    c, lay, q, k, v, mask, m_sb = _operands(dev, case, dtype)
    o_ss, o_sh = lay["o_ss"], lay["o_sh"]
    obuf = torch.full((2 * GUARD + B * Sq * o_ss,), SENT, dtype=dtype, device=dev)
    body = obuf[GUARD: GUARD + B * Sq * o_ss].view(B, Sq, o_ss)
    heads = body[:, :, :Hq * o_sh].view(B, Sq, Hq, o_sh)
    out = heads[..., :D]
    lbuf = torch.full((2 * GUARD + B * Hq * Sq,), SENT, dtype=torch.float32, device=dev)
    lse = lbuf[GUARD: GUARD + B * Hq * Sq]
    for t in (q, k, v, out):
        assert t.data_ptr() % 16 == 0
    _lib.check(lib.mra_prefill_attention(_lib.ptr(q), q.stride(0), q.stride(1), q.stride(2), _lib.ptr(k), k.stride(0), k.stride(1), k.stride(2), _lib.ptr(v),
                                         v.stride(0), v.stride(1), v.stride(2), None if mask is None else _lib.ptr(mask), m_sb, B, Hq, Hkv, Sq, Skv, off, D,
                                         _lib.mra_dtype(dtype), c["scale"], _lib.ptr(out), Sq * o_ss, o_ss, o_sh, _lib.ptr(lse) if want_lse else None,
                                         stream), "prefill_attention")
    assert bool((obuf[:GUARD] == SENT).all() and (obuf[GUARD + B * Sq * o_ss:] == SENT).all()), case
    assert bool((heads[..., D:] == SENT).all() and (body[:, :, Hq * o_sh:] == SENT).all()), case       # between the heads and between the rows
    assert bool((lbuf[:GUARD] == SENT).all() and (lbuf[GUARD + B * Hq * Sq:] == SENT).all()), case
    if not want_lse:
        assert bool((lse == SENT).all()), case
    assert torch.equal(q.cpu().view(torch.int16), c["q"].view(torch.int16)) and torch.equal(k.cpu().view(torch.int16), c["k"].view(torch.int16))
    return out.clone(), lse.view(B, Hq, Sq).clone() if want_lse else None


@pytest.mark.parametrize("dtype", PC.DTYPES, ids=_id)
def test_entry_against_float64(dev, dtype):
    worst = [0.0, 0.0]
    for case in CASES:
        out, lse = _run(dev, case, dtype)
        r = PC.ratios(*case, dtype, out, lse)
        print(f"prefill_attention {_id(dtype)} {case}: |d| / bound out {r[0]:.3g} lse {r[1]:.3g}")
        assert max(r) <= 1.0, (case, r)
        worst = [max(a, b) for a, b in zip(worst, r)]
        out2, lse2 = _run(dev, case, dtype)                                           # two runs, the same bits
        assert torch.equal(out.view(torch.int16), out2.view(torch.int16)) and torch.equal(lse.view(torch.int32), lse2.view(torch.int32)), case
        out0, _ = _run(dev, case, dtype, want_lse=False)                              # lse = NULL: the same out bits
        assert torch.equal(out.view(torch.int16), out0.view(torch.int16)), case
    print(f"prefill_attention {_id(dtype)}: worst |d| / bound out {worst[0]:.3g} lse {worst[1]:.3g}")
    assert all(w > 0.0 for w in worst)


def test_zero_batch_touches_nothing(dev):
    lib, stream = _lib.lib(), _lib.current_stream()
    out = torch.full((64,), SENT, device=dev)
    assert lib.mra_prefill_attention(None, 0, 0, 0, None, 0, 0, 0, None, 0, 0, 0, None, 0, 0, 4, 4, 9, 9, 0, 64, _lib.MRA_BF16, 1.0, _lib.ptr(out), 0, 0, 0,
                                     _lib.ptr(out), stream) == 0
    torch.cuda.synchronize(dev)
    assert bool((out == SENT).all())


@pytest.mark.parametrize("dtype", PC.DTYPES, ids=_id)
def test_last_query_row_against_the_decode_entry(dev, dtype):
    """The last row of a prefill is a one-token call over the same keys: both entries sit inside their own bounds around the same float64 values,
    so their difference sits inside the sum of the two bounds."""
    picked = [c for c in CASES if c[3] in (PC.KT + 1, PC.QB + 1, 2 * PC.QB + 3, 3) and c[7] in ("null", "left_pad", "holes", "mid_tile")][:8]
    assert len(picked) >= 5
    for case in picked:
        B, Hq, Hkv, Sq, Skv, off, D, _ = case
        c, _, q, k, v, mask, m_sb = _operands(dev, case, dtype)
        S = off + Sq                                                                  # the last row attends the keys below it
        got = LD.prefill_attention(q, k, v, None if c["mask"] is None else c["mask"].to(dev)[:, None, None, :], c["scale"], q_offset=off, hip=True)
        m1 = None if c["mask"] is None else c["mask"][:, :S].to(dev)[:, None, None, :]
        one = LD.decode_attention(q[:, :, Sq - 1:Sq], k[:, :, :S], v[:, :, :S], m1, c["scale"], hip=True)[:, :, 0]       # [B, Hq, D]
        ref_p = PC.reference(*case, dtype)
        ref_d = DC.reference_tensors(c["q"][:, :, Sq - 1], c["k"][:, :, :S], c["v"][:, :, :S], None if c["mask"] is None else c["mask"][:, :S], c["scale"], dtype)
        bound = ref_p["out_b"][:, Sq - 1] + ref_d["out_b"]
        live = ~ref_d["empty"]
        assert torch.equal(live, ~ref_p["empty"][:, :, Sq - 1])
        r = PC.ratio(got[:, Sq - 1].cpu()[live], one.double().cpu()[live], bound[live])
        print(f"prefill against decode {_id(dtype)} {case}: |d| / (sum of the bounds) {r:.3g}")
        assert r <= 1.0, (case, r)


@pytest.mark.parametrize("dtype", PC.DTYPES, ids=_id)
def test_python_entry_takes_the_kernel_on_views_and_the_torch_ops_otherwise(dev, dtype):
    case = (3, 8, 2, 3, 2 * PC.QB + 40, 0, 128, "holes")                              # the static-cache shape
    B, Hq, Hkv, Sq, Skv, off, D, _ = case
    c, _, q, k, v, _, _ = _operands(dev, case, dtype)
    ref = PC.reference(*case, dtype)
    mask = c["mask"].to(dev)[:, None, None, :]
    hip, lse = LD.prefill_attention(q, k, v, mask, c["scale"], hip=True, want_lse=True)
    ops, lse_ops = LD.prefill_attention(q, k, v, mask, c["scale"], hip=False, want_lse=True)
    assert hip.shape == ops.shape == (B, Sq, Hq, D) and hip.dtype == ops.dtype == dtype and lse.shape == lse_ops.shape == (B, Hq, Sq)
    assert max(PC.ratios_against(ref, hip, lse)) <= 1.0 and max(PC.ratios_against(ref, ops, lse_ops)) <= 1.0
    assert torch.equal(LD.prefill_attention(q, k, v, mask, c["scale"]), hip)          # hip=None: the entry
    q32 = q.float()
    assert LD.prefill_attention(q32, k.float().nan_to_num(0, 0, 0), v.float().nan_to_num(0, 0, 0), mask, c["scale"]).dtype == torch.float32
    with pytest.raises(_lib.MraError, match="16-bit"):
        LD.prefill_attention(q32, k.float(), v.float(), mask, c["scale"], hip=True)
    with pytest.raises(_lib.MraError, match="outside"):
        LD.prefill_attention(q[..., :32], k[..., :32], v[..., :32], mask, c["scale"], hip=True)
    with pytest.raises(ValueError, match="q_offset"):
        LD.prefill_attention(q, k, v, mask, c["scale"], q_offset=Skv)


# ---- the model ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kv_heads", [4, 2])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_every_attention_call_of_a_real_prefill_is_inside_the_bound(dev, dtype, kv_heads, monkeypatch):
    llm, _ = _llama(dev, kv_heads, dtype, False)
    embeds, mask = _prefix(dev, dtype)
    seen = []
    real = LD.prefill_attention

    def spy(q, k, v, key_mask, scale, q_offset=0, **kw):
        out = real(q, k, v, key_mask, scale, q_offset=q_offset, hip=True)
        assert key_mask.dtype == torch.bool and tuple(key_mask.shape) == (3, 1, 1, k.shape[2]) and k.shape[1] == kv_heads and q_offset == 0
        ref = PC.reference_tensors(q.cpu(), k.cpu(), v.cpu(), key_mask[:, 0, 0].cpu(), scale, 0, dtype)
        seen.append((PC.ratios_against(ref, out, None)[0], q.shape[2], k.shape[2], q.stride()))
        return out

    monkeypatch.setattr(LD, "prefill_attention", spy)
    before = llm.config._attn_implementation
    with torch.no_grad(), LD.hip_decode(llm, prefill=True):
        llm(inputs_embeds=embeds, attention_mask=mask, use_cache=True, return_dict=True, logits_to_keep=1)
    assert llm.config._attn_implementation == before
    assert len(seen) == llm.config.num_hidden_layers and all(s[1] == s[2] == PREFIX for s in seen)
    worst = max(s[0] for s in seen)
    print(f"{_id(dtype)} kv heads {kv_heads}: {len(seen)} prefill calls of {PREFIX} rows, q strides {seen[0][3]}; worst |d| / bound {worst:.3g}")
    assert 0.0 < worst <= 1.0


@pytest.mark.parametrize("kv_heads", [4, 2])
def test_hip_step_behind_a_hip_prefill_tokens_are_argmax_up_to_rounding_ties(dev, kv_heads, monkeypatch):
    llm, _ = _llama(dev, kv_heads, torch.bfloat16, False)
    llm32 = copy.deepcopy(llm).float()
    embeds, mask = _prefix(dev, torch.bfloat16)
    kw = dict(inputs_embeds=embeds, attention_mask=mask, max_new_tokens=N_NEW, min_new_tokens=N_NEW, do_sample=False)
    routed = []
    real = LD.prefill_attention
    monkeypatch.setattr(LD, "prefill_attention", lambda *a, **k: routed.append(a[0].shape[2]) or real(*a, **k))
    with torch.no_grad():
        stock = llm.generate(**kw)
        assert not routed
        step = LS.HipLmDecoder(llm, prefill="hip").generate(embeds, mask, N_NEW, ignore_eos=True)
        L32_stock = _teacher_forced(llm32, embeds, mask, stock)
        d_stock = (_teacher_forced(llm, embeds, mask, stock) - L32_stock).abs().max().item()
        L32 = _teacher_forced(llm32, embeds, mask, step)
        gap = (L32.max(2).values - L32.gather(2, step[:, :, None]).squeeze(2)).max().item()
    print(f"kv heads {kv_heads}: d_stock {d_stock:.4g}; worst fp32 gap to the argmax under hip_step + hip prefill {gap:.4g} (bar 2 d_stock = "
          f"{2 * d_stock:.4g}); {int((stock == step).sum())} of {stock.numel()} tokens equal")
    assert routed == [PREFIX] * llm.config.num_hidden_layers
    assert d_stock > 0 and step.shape == stock.shape
    assert gap <= 2 * d_stock


def test_generate_llm_hip_prefill_leaves_the_lm_as_it_was(dev, monkeypatch):
    llm, tok = _tiny_llama(dev)
    model = _model(dev, llm, tok)
    batch = _batch(dev)
    tokens = []
    real = llm.generate
    monkeypatch.setattr(llm, "generate", lambda **kw: tokens.append(real(**kw).clone()) or tokens[-1].clone())
    routed = []
    real_prefill = LD.prefill_attention
    monkeypatch.setattr(LD, "prefill_attention", lambda *a, **k: routed.append(a[0].is_cuda) or real_prefill(*a, **k))
    before = {k: v.clone() for k, v in llm.state_dict().items()}
    impl, training = llm.config._attn_implementation, llm.training
    first = model.generate_llm(batch, max_new_tokens=12)
    assert not routed
    for decode in ("hip_step", "hip"):
        model.lm_decode, model.lm_prefill = decode, "hip"
        n = len(routed)
        hip = model.generate_llm(batch, max_new_tokens=12)
        assert len(routed) == n + llm.config.num_hidden_layers and all(routed) and len(hip) == len(first)
        after = llm.state_dict()
        assert all(torch.equal(before[k], after[k]) for k in before) and llm.config._attn_implementation == impl and llm.training == training
        print(f"generate_llm: {decode} + hip prefill strings equal the stock ones: {hip == first}")
    model.lm_decode, model.lm_prefill = "stock", "stock"
    n = len(routed)
    again = model.generate_llm(batch, max_new_tokens=12)
    assert len(routed) == n and torch.equal(tokens[0], tokens[-1]) and again == first    # a following stock call: the token bits of the one before
    model.lm_prefill = "hip"
    with pytest.raises(ValueError, match="lm_prefill='hip' needs"):
        model.generate_llm(batch, max_new_tokens=2)
    model.lm_prefill = "stock"
    model.compat_repeat = False
    multi = {**batch, "text_input": [[t, t + " again"] for t in batch["text_input"]]}
    multi_stock = model.generate_multi_llm(multi, max_new_tokens=4)
    model.lm_decode, model.lm_prefill = "hip_step", "hip"
    n = len(routed)
    multi_hip = model.generate_multi_llm(multi, max_new_tokens=4)
    assert len(routed) > n and [len(x) for x in multi_hip] == [len(x) for x in multi_stock] == [2, 2]


def test_trainer_validates_on_strings_decoded_behind_a_hip_prefill(dev, tmp_path):
    from mraudio_amd.eval.mr_eval import eval_submission
    from mraudio_amd.utils.mr_dataset import prepare_sample
    from mraudio_amd.utils.spans import moment_str_to_list, post_process
    from mraudio_amd.utils.trainer import Trainer, default_args

    llm, tok = _tiny_llama(dev)
    model = _model(dev, llm, tok)
    kw = dict(output_dir=str(tmp_path), gpu=0, synthetic=4, dataset="Charades_STA", max_epoch=1)
    with pytest.raises(ValueError, match="lm_prefill='hip' needs"):
        Trainer(default_args(val_decode="llm", lm_prefill="hip", **kw), model=model)
    tr = Trainer(default_args(val_decode="llm", lm_decode="hip_step", lm_prefill="hip", **kw), model=model)
    assert model.lm_decode == "hip_step" and model.lm_prefill == "hip"
    got = tr.eval_epoch()
    results = []
    with torch.no_grad():
        for samples in tr.val_dataloader:
            samples = prepare_sample(samples, dev)
            for qid, query, vid, target, out in zip(samples["qid"], samples["query"], samples["vid"], samples["text_output"], model.generate_llm(samples)):
                results.append({"qid": qid, "query": query, "vid": vid, "relevant_windows": moment_str_to_list(post_process(target)),
                                "pred_relevant_windows": moment_str_to_list(post_process(out))})
    want = eval_submission(results, results, verbose=False)
    assert got["brief"] == want["brief"] and "MR-full-R1-avg" in got["brief"]
    assert llm.config._attn_implementation != LD.PREFILL_NAME
