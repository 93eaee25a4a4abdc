"""The one-token step of the LM's decode on the GPU (csrc/lm_step.hip): every form of the skinny kernel through ``mra_debug_lm_skinny`` against
float64 of the rounded operands inside the derived bound of tests/lm_step_cases.py, the head and its argmax, ``mra_lm_step`` on tiny Llamas held
by composition (every launch inside its bound on the chain's own intermediates, the step bit-equal to the composition), and the ``"hip_step"``
route of XInstructBLIP end to end with the criterion tests/test_gpu_decode_attn.py uses."""
import copy
import ctypes as C

import pytest
import torch

import decode_attn_cases as DC
import lm_step_cases as LC
from mraudio_amd import _lib
from mraudio_amd.models import lm_decode as LD
from mraudio_amd.models import lm_step as LS
from test_gpu_llm_objective import LH, _batch, _model, _tiny_llama

pytestmark = pytest.mark.gpu

GUARD, SENT = 64, 77.0             # guard elements on either side of every output; the sentinel is exact in f16, bf16 and fp32
CASES = LC.skinny_cases()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _guarded(rows, ld, dtype, dev):
    """(whole buffer, the [rows, ld] view between two guards), all sentinel."""
    buf = torch.full((2 * GUARD + rows * ld,), SENT, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + rows * ld].view(rows, ld)


def _nbytes(t):
    """Bytes from a view's first element through its last."""
    return t.element_size() * (sum((n - 1) * s for n, s in zip(t.shape, t.stride())) + 1)


def skinny(dev, dtype, epi, x, K, gain, segs, outs, out_f32=False, res=None, rope=None, eps=LC.EPS):
    """One ``mra_debug_lm_skinny`` call on device tensors.  ``x`` [B, ldx] (K columns used); ``segs`` [(W [N, ldw], A, Bw, scale)]; ``outs`` per
    segment a [B, ldo] view or None; ``rope`` dict(Hq, Hkv, D, slot, pos_offset, position, cos, sin, kc, vc) with kc / vc [B, Hkv, Smax, D] views."""
    d = _lib.mra_lm_skinny_desc()
    d.struct_bytes = C.sizeof(d)
    B = x.shape[0]
    d.B, d.K, d.dtype, d.epilogue, d.nseg, d.out_f32 = B, K, _lib.mra_dtype(dtype), epi, len(segs), int(out_f32)
    d.x, d.ldx, d.x_bytes = x.data_ptr(), x.stride(0), x.element_size() * ((B - 1) * x.stride(0) + K)
    d.norm_gain, d.eps = (0 if gain is None else gain.data_ptr()), eps
    keep = []
    for s, (W, A, Bw, scale) in enumerate(segs):
        sg = d.seg[s]
        sg.W, sg.ldw, sg.N = W.data_ptr(), W.stride(0), W.shape[0]
        d.w_bytes[s] = 2 * ((W.shape[0] - 1) * W.stride(0) + K)
        if A is not None:
            sg.A, sg.Bw, sg.R, sg.scale = A.data_ptr(), Bw.data_ptr(), A.shape[0], scale
        if outs[s] is not None:
            o = outs[s]
            d.out[s], d.ldo[s], d.out_bytes[s] = o.data_ptr(), o.stride(0), o.element_size() * ((B - 1) * o.stride(0) + W.shape[0])
    if res is not None:
        d.res, d.ldres, d.res_bytes = res.data_ptr(), res.stride(0), 2 * ((B - 1) * res.stride(0) + segs[0][0].shape[0])
    if rope is not None:
        d.Hq, d.Hkv, d.D, d.slot, d.pos_offset = rope["Hq"], rope["Hkv"], rope["D"], rope["slot"], rope["pos_offset"]
        d.position, d.cos, d.sin = rope["position"].data_ptr(), rope["cos"].data_ptr(), rope["sin"].data_ptr()
        d.rope_rows, d.rope_ld = rope["cos"].shape[0], rope["cos"].stride(0)
        d.rope_bytes = 4 * ((d.rope_rows - 1) * d.rope_ld + d.D)
        kc, vc = rope["kc"], rope["vc"]
        d.kcache, d.vcache = kc.data_ptr(), vc.data_ptr()
        d.k_sb, d.k_sh, d.k_ss = kc.stride(0), kc.stride(1), kc.stride(2)
        d.v_sb, d.v_sh, d.v_ss = vc.stride(0), vc.stride(1), vc.stride(2)
        d.kcache_bytes, d.vcache_bytes = _nbytes(kc), _nbytes(vc)
    ws = torch.empty(LC.skinny_workspace_bytes(B, K), dtype=torch.uint8, device=dev)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    _lib.check(_lib.lib().mra_debug_lm_skinny(C.byref(d), _lib.current_stream()), "mra_debug_lm_skinny")
    return ws


def _run_case(ci, dtype, dev):
    """The case's launch on the GPU with sentinel-filled, guarded outputs and (rotary form) a NaN-poisoned longer cache: ``emulate``'s dict on the
    CPU, after the guards, the pitch padding and every cache entry but the one slot were found untouched."""
    c, t, _, _ = LC.reference(ci, dtype)
    B, K, epi = c["B"], c["K"], c["epi"]
    x = t["x"].to(dev)
    gain = None if t["gain"] is None else t["gain"].to(dev)
    segs = [(W.to(dev), None if A is None else A.to(dev), None if A is None else Bw.to(dev), s) for W, A, Bw, s in zip(t["W"], t["A"], t["Bw"], t["scale"])]
    odt = torch.float32 if c["f32"] else dtype
    n_out = len(c["N"]) if epi in (LC.PLAIN, LC.RES) else 1
    bufs, outs = [], []
    for s in range(len(c["N"])):
        if s < n_out:
            N = c["N"][s]
            buf, view = _guarded(B, N + (8 if c["pitch"] else 0) + (-N) % 8, odt, dev)
            bufs.append(buf)
            outs.append(view)
        else:
            outs.append(None)
    res, rope, poison = None, None, None
    if epi == LC.RES:
        N = c["N"][0]
        res = torch.full((B, N + (-N) % 8 + (16 if c["pitch"] else 0)), float("nan"), dtype=dtype, device=dev)     # a pitched residual; the padding is never read
        res[:, :N] = t["res"].to(dev)
    if epi == LC.ROPE:
        D, Hkv, Smax = c["D"], c["Hkv"], t["Smax"]
        k_ss = D + (8 if c["pitch"] else 0)
        poison = [torch.full((B, Hkv, Smax + 7, k_ss), float("nan"), dtype=dtype, device=dev) for _ in range(2)]
        rope = dict(Hq=c["Hq"], Hkv=Hkv, D=D, slot=t["slot"], pos_offset=t["pos_offset"], position=t["position"].to(dev), cos=t["cos"].to(dev),
                    sin=t["sin"].to(dev), kc=poison[0][:, :, :Smax, :D], vc=poison[1][:, :, :Smax, :D])
    skinny(dev, dtype, epi, x, K, gain, segs, outs, c["f32"], res, rope)
    torch.cuda.synchronize(dev)
    got = dict(out=[])
    for s in range(n_out):
        N = c["N"][s]
        assert bool((bufs[s][:GUARD] == SENT).all()) and bool((bufs[s][-GUARD:] == SENT).all()), "a guard was written"
        assert bool((outs[s][:, N:] == SENT).all()), "the pitch padding was written"
        got["out"].append(outs[s][:, :N].cpu())
    if epi == LC.ROPE:
        for name, p in zip("kv", poison):
            row = p[:, :, t["slot"], :c["D"]].clone()
            assert torch.isfinite(row).all()
            p[:, :, t["slot"], :c["D"]] = float("nan")
            assert bool(torch.isnan(p).all()), "more than the one slot of the cache was written"
            got[name] = row.cpu()
    return got


# ---- 1. every form of the skinny kernel, per launch -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", LC.DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[LC.case_id(c) for c in CASES])
def test_skinny_launch_is_inside_the_bound_and_repeats_bit_for_bit(dev, ci, dtype):
    got = _run_case(ci, dtype, dev)
    r = LC.ratios(ci, dtype, got)
    print(f"{LC.case_id(CASES[ci])} {dtype}: worst |d| / bound {r:.3g}")
    assert r <= 1.0
    again = _run_case(ci, dtype, dev)
    for a, b in zip(got["out"], again["out"]):
        assert torch.equal(a, b)
    if CASES[ci]["epi"] == LC.ROPE:
        assert torch.equal(got["k"], again["k"]) and torch.equal(got["v"], again["v"])


@pytest.mark.parametrize("dtype", LC.DTYPES, ids=["f16", "bf16"])
def test_a_position_outside_the_table_writes_nan_and_reads_nothing(dev, dtype):
    ci = next(i for i, c in enumerate(CASES) if c["epi"] == LC.ROPE and c["B"] == 3)
    c, t, ref, _ = LC.reference(ci, dtype)
    t2 = dict(t, position=torch.tensor([2, 40, -9], dtype=torch.int32))              # + 3: rows 1 and 2 fall outside [0, 40)
    B, K, D, Hkv = c["B"], c["K"], c["D"], c["Hkv"]
    segs = [(W.to(dev), None if A is None else A.to(dev), None if A is None else Bw.to(dev), s) for W, A, Bw, s in zip(t["W"], t["A"], t["Bw"], t["scale"])]
    q = torch.zeros(B, c["N"][0], dtype=dtype, device=dev)
    kc, vc = (torch.zeros(B, Hkv, t["Smax"], D, dtype=dtype, device=dev) for _ in range(2))
    rope = dict(Hq=c["Hq"], Hkv=Hkv, D=D, slot=t["slot"], pos_offset=t["pos_offset"], position=t2["position"].to(dev), cos=t["cos"].to(dev),
                sin=t["sin"].to(dev), kc=kc, vc=vc)
    skinny(dev, dtype, LC.ROPE, t["x"].to(dev), K, t["gain"].to(dev), segs, [q, None, None], rope=rope)
    assert torch.isfinite(q[0]).all() and torch.isnan(q[1:]).all() and torch.isnan(kc[1:, :, t["slot"]]).all()
    assert torch.isfinite(vc[:, :, t["slot"]]).all()                                   # v is not rotated


# ---- 2. the head and its argmax -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", LC.DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("V", LC.HEAD_V)
def test_head_logits_and_argmax_with_ties_and_a_nan(dev, V, dtype):
    B, K = 3, 72
    g = LC._gen(V, 5, dtype == torch.float16)
    x = torch.randn(B, K, generator=g).to(dtype)
    gain = (1 + 0.3 * torch.randn(K, generator=g)).to(dtype)
    W = (torch.randn(V, K, generator=g) / K ** 0.5).to(dtype)
    c = dict(epi=LC.PLAIN, B=B, K=K, N=(V,), R=(0,), norm=True, f32=True, pitch=False)
    t = dict(x=x, gain=gain, W=[W], A=[None], Bw=[None], scale=[0.0])
    buf, logits = _guarded(B, V, torch.float32, dev)
    skinny(dev, dtype, LC.PLAIN, x.to(dev), K, gain.to(dev), [(W.to(dev), None, None, 0.0)], [logits], out_f32=True)
    ref, bnd = LC._launch(c, t, LC.F64)["out"][0], LC.bounds(c, t, dtype)["out"][0]
    r = LC.ratio(logits.cpu(), ref, bnd)
    assert r <= 1.0 and bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all())
    lib, stream = _lib.lib(), _lib.current_stream()
    tok = torch.full((B,), -7, dtype=torch.int32, device=dev)
    _lib.check(lib.mra_debug_lm_argmax(_lib.ptr(logits), V, B, V, _lib.ptr(tok), None, 0, None, 0, stream), "argmax")
    assert torch.equal(tok.cpu().long(), LS.argmax_ref(logits.cpu()))                  # the kernel's own logits
    z = LC.argmax_case(V).to(dev)                                                       # planted ties, a NaN in the last row
    _lib.check(lib.mra_debug_lm_argmax(_lib.ptr(z), V, B, V, _lib.ptr(tok), None, 0, None, 0, stream), "argmax")
    want = LS.argmax_ref(z.cpu())
    assert torch.equal(tok.cpu().long(), want)
    if V >= 63:
        assert not torch.equal(want, LS.argmax_ref(z.cpu(), "argmax_tie_highest"))
    # the greedy bookkeeping: row 0 was finished (emits pad), row 1 emits an eos id (becomes finished), row 2 goes on
    eos = (C.c_int32 * 2)(int(want[1]), V + 5)
    fin = torch.tensor([1, 0, 0], dtype=torch.int32, device=dev)
    _lib.check(lib.mra_debug_lm_argmax(_lib.ptr(z), V, B, V, _lib.ptr(tok), _lib.ptr(fin), V + 9, eos, 2, stream), "argmax")
    wt, wf = LS.greedy_ref(want, torch.tensor([1, 0, 0]), V + 9, [int(want[1]), V + 5])
    assert tok.cpu().long().tolist() == wt.tolist() and fin.cpu().bool().tolist() == wf.tolist()
    print(f"V {V} {dtype}: worst |logit - float64| / bound {r:.3g}; argmax {want.tolist()}")


# ---- 3. the step, by composition ------------------------------------------------------------------------------------------------------------------------
N_NEW, PREFIX = 24, 300


def _llama(dev, kv_heads, dtype, lora):
    import transformers as tf

    llm, tok = _tiny_llama(dev, dtype)
    if kv_heads != llm.config.num_key_value_heads:
        torch.manual_seed(1)
        cfg = copy.deepcopy(llm.config)
        cfg.num_key_value_heads = kv_heads
        llm = tf.LlamaForCausalLM(cfg).to(dev).to(dtype).eval().requires_grad_(False)
    if lora:
        LC.add_adapters(llm, seed=kv_heads)
    return llm, tok


def _prefix(dev, dtype):
    """B = 3 prefixes of PREFIX embedded rows: left padding in one sequence, holes inside another (tests/test_gpu_decode_attn.py's)."""
    gen = torch.Generator().manual_seed(12)
    embeds = (torch.randn(3, PREFIX, LH, generator=gen) * 0.5).to(dtype).to(dev)
    mask = torch.ones(3, PREFIX, dtype=torch.long)
    mask[1, :37] = 0
    mask[2, 11:19] = 0
    mask[2, 150:163] = 0
    mask[1, 200] = 0
    return embeds, mask.to(dev)


def _check(worst, name, c, t, got, dtype):
    """One launch of the composition against float64 of ITS inputs: the ratio to the per-launch bound goes into ``worst``."""
    ref, bnd = LC._launch(c, t, LC.F64), LC.bounds(c, t, dtype)
    r = max(LC.ratio(g.cpu(), a, b) for g, a, b in zip(got["out"], ref["out"], bnd["out"]))
    if c["epi"] == LC.ROPE:
        r = max(r, LC.ratio(got["k"].cpu(), ref["k"], bnd["k"]), LC.ratio(got["v"].cpu(), ref["v"], bnd["v"]))
    worst[name] = max(worst.get(name, 0.0), r)


def _composed_step(dev, llm, w, tokens_in, cache, mask8, position, j, S0, rope, worst):
    """The launches of one ``mra_lm_step`` issued one at a time through the debug entries (and ``mra_decode_attention``), each checked against
    float64 of its own inputs: (logits, final residual rows).  ``cache``'s slot is written as the step writes it."""
    dtype, B = cache.dtype, tokens_in.shape[0]
    H, I, Hq, Hkv, D = w["hidden"], w["inter"], w["Hq"], w["Hkv"], w["D"]
    slot = S0 + j - 1
    h = w["embed"][tokens_in.long()].clone()
    cpu = lambda v: None if v is None else v.detach().cpu()
    segs = lambda *mods: [LS.split_linear(m) for m in mods]
    case = lambda epi, K, ss, norm, **kw: dict(epi=epi, B=B, K=K, N=tuple(s[0].shape[0] for s in ss), R=tuple(0 if s[1] is None else s[1].shape[0] for s in ss),
                                                norm=norm, f32=kw.pop("f32", False), pitch=False, **kw)
    tens = lambda x, gain, ss, **kw: dict(x=cpu(x), gain=cpu(gain), W=[cpu(s[0]) for s in ss], A=[cpu(s[1]) for s in ss], Bw=[cpu(s[2]) for s in ss],
                                          scale=[s[3] for s in ss], **kw)
    for l, rec in enumerate(w["layers"]):
        ss = segs(rec["q"], rec["k"], rec["v"])
        q = torch.empty(B, Hq * D, dtype=dtype, device=dev)
        kc, vc = cache[l, 0], cache[l, 1]
        skinny(dev, dtype, LC.ROPE, h, H, rec["norm1"], ss, [q, None, None], eps=w["eps"],
               rope=dict(Hq=Hq, Hkv=Hkv, D=D, slot=slot, pos_offset=j - 1, position=position, cos=rope[0], sin=rope[1], kc=kc, vc=vc))
        _check(worst, "qkv", case(LC.ROPE, H, ss, True, D=D, Hq=Hq, Hkv=Hkv),
               tens(h, rec["norm1"], ss, position=position.cpu(), pos_offset=j - 1, cos=rope[0].cpu(), sin=rope[1].cpu(), slot=slot),
               dict(out=[q], k=kc[:, :, slot], v=vc[:, :, slot]), dtype)
        S = slot + 1
        m = mask8[:, :S].bool()
        ao = LD.decode_attention(q.view(B, Hq, 1, D), kc[:, :, :S], vc[:, :, :S], m[:, None, None, :], rec["scale"], hip=True)[:, :, 0]
        ref = DC.reference_tensors(q.view(B, Hq, D).cpu(), kc[:, :, :S].cpu(), vc[:, :, :S].cpu(), m.cpu(), rec["scale"], dtype)
        worst["attention"] = max(worst.get("attention", 0.0), max(DC.ratios_against(ref, ao, None)))
        ao = ao.reshape(B, Hq * D).contiguous()
        ss = segs(rec["o"])
        h2 = torch.empty_like(h)
        skinny(dev, dtype, LC.RES, ao, Hq * D, None, ss, [h2], res=h)
        _check(worst, "o", case(LC.RES, Hq * D, ss, False), tens(ao, None, ss, res=cpu(h)), dict(out=[h2]), dtype)
        h = h2
        ss = segs(rec["gate"], rec["up"])
        act = torch.empty(B, I, dtype=dtype, device=dev)
        skinny(dev, dtype, LC.SWIGLU, h, H, rec["norm2"], ss, [act, None], eps=w["eps"])
        _check(worst, "gate_up", case(LC.SWIGLU, H, ss, True), tens(h, rec["norm2"], ss), dict(out=[act]), dtype)
        ss = segs(rec["down"])
        h2 = torch.empty_like(h)
        skinny(dev, dtype, LC.RES, act, I, None, ss, [h2], res=h)
        _check(worst, "down", case(LC.RES, I, ss, False), tens(act, None, ss, res=cpu(h)), dict(out=[h2]), dtype)
        h = h2
    logits = torch.empty(B, w["V"], dtype=torch.float32, device=dev)
    ss = [(w["head"], None, None, 0.0)]
    skinny(dev, dtype, LC.PLAIN, h, H, w["final_norm"], ss, [logits], out_f32=True, eps=w["eps"])
    _check(worst, "head", case(LC.PLAIN, H, ss, True, f32=True), tens(h, w["final_norm"], ss), dict(out=[logits]), dtype)
    return logits, h


@pytest.mark.parametrize("lora", [False, True], ids=["plain", "lora"])
@pytest.mark.parametrize("kv_heads", [4, 2])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_every_step_is_its_launches_and_every_launch_is_inside_its_bound(dev, dtype, kv_heads, lora):
    llm, _ = _llama(dev, kv_heads, dtype, lora)
    assert llm.config.rms_norm_eps == LC.EPS and llm.config.hidden_size == 256 and llm.config.vocab_size == 260
    embeds, mask = _prefix(dev, dtype)
    dec = LS.HipLmDecoder(llm)
    seen = {}
    real = dec.descriptor

    def descriptor(B, cache, mask8, position, rope, h, *rest):
        seen.update(cache=cache, mask8=mask8, position=position, rope=rope, h=h)
        return real(B, cache, mask8, position, rope, h, *rest)

    dec.descriptor = descriptor
    tokens = dec.generate(embeds, mask, N_NEW, ignore_eos=True, keep_logits=True)
    torch.cuda.synchronize(dev)
    assert tokens.shape == (3, N_NEW) and dec.last_logits.shape == (3, N_NEW, 260)
    cache, w = seen["cache"], LS.walk(llm)
    assert (seen["position"].cpu() != PREFIX).any()                                     # positions and cache slots differ
    final = cache.clone()
    worst, fars = {}, []
    for j in range(1, N_NEW):
        logits, h = _composed_step(dev, llm, w, tokens[:, j - 1].to(torch.int32), cache, seen["mask8"], seen["position"], j, PREFIX, seen["rope"], worst)
        assert torch.equal(logits, dec.last_logits[:, j]), f"step {j}: mra_lm_step's logits are not its launches' logits"
        assert torch.equal(LS.argmax_ref(dec.last_logits[:, j]), tokens[:, j])
        slot = PREFIX + j - 1
        assert torch.equal(cache[:, :, :, :, slot], final[:, :, :, :, slot])
        # the float64 definition on the same cache and tokens, at every step, under the stated margin of the cases file
        ref, _ = LS.lm_step_ref(llm, tokens[:, j - 1], cache.clone(), seen["mask8"], seen["position"].long() + (j - 1), slot, dtype=dtype,
                                compute=torch.float64, rope=seen["rope"])
        dist = (ref - logits.double()).abs().max().item()
        fars.append((dist / LC.chain_margin(ref, dtype), dist, j))
    assert torch.equal(h, seen["h"])                                                    # the residual rows the last step left
    print(f"{dtype} kv {kv_heads} lora {lora}: {N_NEW - 1} steps; worst |d| / bound per launch {dict((k, round(v, 3)) for k, v in worst.items())}; "
          f"worst |logit - lm_step_ref float64| over the steps {max(fars)[1]:.3g} at step {max(fars)[2]} = {max(fars)[0]:.3g} of the margin "
          f"{LC.CHAIN_ULPS} U (logit scale {dec.last_logits.abs().max().item():.3g})")
    assert max(worst.values()) <= 1.0
    assert len(fars) == N_NEW - 1 and max(fars)[0] <= 1.0


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------------------------------
def _teacher_forced(model, embeds, mask, tokens):
    """fp32 logits [B, N_NEW, V] that predict ``tokens`` from one uncached forward over prefix + tokens."""
    emb = model.get_input_embeddings()(tokens).to(embeds.dtype if model.dtype != torch.float32 else torch.float32)
    x = torch.cat([embeds.to(emb.dtype), emb], 1)
    m = torch.cat([mask, torch.ones_like(tokens)], 1)
    logits = model(inputs_embeds=x, attention_mask=m, return_dict=True).logits
    return logits[:, PREFIX - 1: PREFIX - 1 + N_NEW].float()


@pytest.mark.parametrize("lora", [False, True], ids=["plain", "lora"])
@pytest.mark.parametrize("kv_heads", [4, 2])
def test_hip_step_tokens_are_argmax_up_to_rounding_ties(dev, kv_heads, lora):
    llm, _ = _llama(dev, kv_heads, torch.bfloat16, lora)
    llm32 = copy.deepcopy(llm).float()
    embeds, mask = _prefix(dev, torch.bfloat16)
    kw = dict(inputs_embeds=embeds, attention_mask=mask, max_new_tokens=N_NEW, min_new_tokens=N_NEW, do_sample=False)
    with torch.no_grad():
        stock = llm.generate(**kw)
        step = LS.HipLmDecoder(llm).generate(embeds, mask, N_NEW, ignore_eos=True)
        L32_stock = _teacher_forced(llm32, embeds, mask, stock)
        d_stock = (_teacher_forced(llm, embeds, mask, stock) - L32_stock).abs().max().item()
        gaps = {}
        for name, toks, L32 in (("stock", stock, L32_stock), ("hip_step", step, _teacher_forced(llm32, embeds, mask, step))):
            gaps[name] = (L32.max(2).values - L32.gather(2, toks[:, :, None]).squeeze(2)).max().item()
    print(f"kv heads {kv_heads} lora {lora}: d_stock {d_stock:.4g}; worst fp32 gap to the argmax: stock {gaps['stock']:.4g}, hip_step "
          f"{gaps['hip_step']:.4g} (bar 2 d_stock = {2 * d_stock:.4g}); {int((stock == step).sum())} of {stock.numel()} tokens equal")
    assert d_stock > 0 and step.shape == stock.shape
    assert gaps["hip_step"] <= 2 * d_stock                   # the stock route's own gap is printed, not asserted: with adapters it can exceed the bar


def test_early_stop_and_pad_are_generates(dev):
    """The counting Llama of the CPU test in bf16 (its margins are far above rounding): eos at different steps per sequence."""
    from test_lm_step_cases_cpu import _counting_llama

    llm, E = _counting_llama()
    llm = llm.to(dev).to(torch.bfloat16)
    B, S0, n = 3, 40, 14
    embeds, mask = LC.prefix(B, S0, llm.config.hidden_size)
    for b, start in enumerate((10, 20, 30)):
        embeds[b, -1] = E[start]
    embeds, mask = embeds.to(dev).to(torch.bfloat16), mask.to(dev)
    for pad in (0, None):
        llm.generation_config.eos_token_id, llm.generation_config.pad_token_id = [14, 27, 39], pad
        with torch.no_grad():
            want = llm.generate(inputs_embeds=embeds, attention_mask=mask, max_new_tokens=n, do_sample=False)
        dec = LS.HipLmDecoder(llm)
        dec.check_every = 2
        got = dec.generate(embeds, mask, n, keep_logits=True)                               # V = 61: the kept logits' rows are pitched to 16 bytes
        assert want.shape == (B, 9) and torch.equal(got, want)
        assert dec.last_logits.shape == (B, 9, 61) and torch.equal(LS.argmax_ref(dec.last_logits[2]), want[2])    # row 2 never emits pad
    many = dec.generate(embeds.repeat(4, 1, 1)[:11], mask.repeat(4, 1)[:11], n)              # more than 8 sequences: blocks of 8
    assert torch.equal(many, want.repeat(4, 1)[:11])


def test_generate_llm_hip_step_leaves_the_lm_as_it_was(dev, monkeypatch):
    from mraudio_amd.models.xinstructblip import XInstructBLIP

    with pytest.raises(ValueError, match="hip_step"):
        XInstructBLIP(seed=0, perturb=True, device=dev, llm_hidden_size=LH, op_dtype=torch.bfloat16, lm_decode="fast")
    llm, tok = _tiny_llama(dev)
    model = _model(dev, llm, tok)
    batch = _batch(dev)
    tokens = []
    real = llm.generate
    monkeypatch.setattr(llm, "generate", lambda **kw: tokens.append(real(**kw).clone()) or tokens[-1].clone())
    before = {k: v.clone() for k, v in llm.state_dict().items()}
    impl, training = llm.config._attn_implementation, llm.training
    first = model.generate_llm(batch, max_new_tokens=12)
    model.lm_decode = "hip_step"
    dec_calls = []
    real_gen = LS.HipLmDecoder.generate
    monkeypatch.setattr(LS.HipLmDecoder, "generate", lambda self, *a, **k: dec_calls.append(1) or real_gen(self, *a, **k))
    hip = model.generate_llm(batch, max_new_tokens=12)
    assert len(tokens) == 1 and dec_calls == [1] and len(hip) == len(first)             # the stock generate was not called
    after = llm.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before) and llm.config._attn_implementation == impl and llm.training == training
    model.lm_decode = "stock"
    again = model.generate_llm(batch, max_new_tokens=12)
    assert torch.equal(tokens[0], tokens[1]) and again == first                          # a following stock call: the token bits of the one before
    print(f"generate_llm: hip_step strings equal the stock ones: {hip == first}")
    model.compat_repeat = False
    multi = {**batch, "text_input": [[t, t + " again"] for t in batch["text_input"]]}
    multi_stock = model.generate_multi_llm(multi, max_new_tokens=4)
    model.lm_decode = "hip_step"
    multi_hip = model.generate_multi_llm(multi, max_new_tokens=4)
    assert len(dec_calls) > 1 and [len(x) for x in multi_hip] == [len(x) for x in multi_stock] == [2, 2]


def test_trainer_validates_on_hip_step_decoded_strings(dev, tmp_path):
    from mraudio_amd.eval.mr_eval import eval_submission
    from mraudio_amd.utils.mr_dataset import prepare_sample
    from mraudio_amd.utils.spans import moment_str_to_list, post_process
    from mraudio_amd.utils.trainer import Trainer, default_args

    llm, tok = _tiny_llama(dev)
    model = _model(dev, llm, tok)
    kw = dict(output_dir=str(tmp_path), gpu=0, synthetic=4, dataset="Charades_STA", max_epoch=1)
    with pytest.raises(ValueError, match="hip_step"):
        Trainer(default_args(val_decode="llm", lm_decode="fast", **kw), model=model)
    tr = Trainer(default_args(val_decode="llm", lm_decode="hip_step", **kw), model=model)
    assert model.lm_decode == "hip_step"
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
