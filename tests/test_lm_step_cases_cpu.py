"""The one-token step of the LM's decode without a GPU: ``lm_step_ref`` against transformers' own one-token forward, the fp32 emulation of every
launch form inside its derived bound and the named mutants outside it, every refusal of the C entries and their workspace formula,
``HipLmDecoder``'s refusals, and the greedy loop (eos, pad, early stop) against ``generate`` on the CPU.  tests/lm_step_cases.py holds the
tables, references and bounds."""
import copy
import ctypes as C

import pytest
import torch

import lm_step_cases as LC
from mraudio_amd import _lib
from mraudio_amd.models import lm_step as LS

tf = pytest.importorskip("transformers")
CASES = LC.skinny_cases()


# ---- 1. the definition against the LM's own forward ------------------------------------------------------------------------------------------------
def _own_step(llm, embeds, mask, tok):
    """transformers' one-token forward over a DynamicCache filled by its own prefill: (logits [B, V], the prefill's cache as a tensor, positions)."""
    pos = mask.cumsum(-1) - 1
    pos.masked_fill_(mask == 0, 1)
    out = llm(inputs_embeds=embeds, attention_mask=mask, position_ids=pos, use_cache=True, return_dict=True, logits_to_keep=1)
    pk = out.past_key_values
    kv = torch.stack([torch.stack([l.keys, l.values]) for l in pk.layers]).clone()                 # [L, 2, B, Hkv, S0, D]
    nxt = mask.sum(-1)
    got = llm(input_ids=tok[:, None], attention_mask=torch.cat([mask, torch.ones_like(mask[:, :1])], 1), position_ids=nxt[:, None],
              past_key_values=pk, use_cache=True, return_dict=True)
    return got.logits[:, -1], kv, nxt


@pytest.mark.parametrize("lora", [False, True], ids=["plain", "lora"])
@pytest.mark.parametrize("kv_heads,head_dim", [(4, 64), (2, 64), (4, 128), (2, 128)])
def test_lm_step_ref_is_the_lms_own_one_token_forward(kv_heads, head_dim, lora):
    llm = LC.tiny_llama(kv_heads, head_dim, lora=lora)
    B, S0 = 3, 21
    embeds, mask = LC.prefix(B, S0, llm.config.hidden_size)
    assert (mask[1, :3] == 0).all() and mask[2, S0 // 2] == 0 and mask[2, 0] == 1                      # left padding; holes inside the prefix
    tok = torch.tensor([5, 17, 96])
    with torch.no_grad():
        want, kv, nxt = _own_step(llm, embeds, mask, tok)
    L = kv.shape[0]
    cache = torch.full((L, 2, B, kv_heads, S0 + 4, head_dim), float("nan"))
    cache[:, :, :, :, :S0] = kv
    m = torch.ones(B, S0 + 4, dtype=torch.uint8)
    m[:, :S0] = mask.to(torch.uint8)
    assert (nxt != S0).any()                                                                            # positions and cache slots differ
    got, _ = LS.lm_step_ref(llm, tok, cache, m, nxt, S0, dtype=None, compute=torch.float32)
    d = (got - want).abs().max().item()
    print(f"kv {kv_heads} D {head_dim} lora {lora}: max |logit difference| {d:.3g} (logit scale {want.abs().max().item():.3g})")
    assert d <= 1e-5
    assert torch.isfinite(cache[:, :, :, :, S0]).all() and torch.isnan(cache[:, :, :, :, S0 + 1:]).all()  # only the one slot was written
    if lora:                                                                                            # the adapters matter: B is non-zero
        from mraudio_amd.models.lora import ADAPTER, lora_modules

        bare = copy.deepcopy(llm)
        for mod in lora_modules(bare).values():
            mod.lora_B[ADAPTER].weight.data.zero_()
        c2 = cache.clone()
        off, _ = LS.lm_step_ref(bare, tok, c2, m, nxt, S0, dtype=None, compute=torch.float32)
        assert (off - want).abs().max().item() > 1e-3


# ---- 2. every launch form: emulation inside the bound, mutants outside ---------------------------------------------------------------------------
def test_the_case_table_covers_what_the_issue_lists():
    assert {c["B"] for c in CASES} == {1, 2, 3, 8} and {c["K"] for c in CASES} == {8, 64, 72, 264, 1032}
    assert {r for c in CASES for r in c["R"]} == {0, 3, 8, 16} and {len(c["N"]) for c in CASES if c["epi"] == LC.PLAIN} == {1, 2, 3}
    assert {n for c in CASES if c["epi"] != LC.ROPE for n in c["N"]} == set(LC.NS)
    for epi in (LC.PLAIN, LC.RES, LC.SWIGLU, LC.ROPE):
        assert {c["pitch"] for c in CASES if c["epi"] == epi} == {False, True}
    assert {(c["D"], c["Hq"] // c["Hkv"]) for c in CASES if c["epi"] == LC.ROPE} >= {(64, 1), (64, 2), (64, 4), (128, 1), (128, 2), (128, 4)}
    assert any(c["f32"] for c in CASES) and any(c["norm"] for c in CASES) and any(not c["norm"] for c in CASES)


@pytest.mark.parametrize("dtype", LC.DTYPES, ids=["f16", "bf16"])
def test_fp32_emulation_of_every_form_is_inside_the_bound(dtype):
    worst = {}
    for ci, c in enumerate(CASES):
        r = LC.ratios(ci, dtype, LC.emulate(ci, dtype))
        worst[c["epi"]] = max(worst.get(c["epi"], 0.0), r)
        assert r <= 1.0, (LC.case_id(c), r)
    print(f"{dtype}: worst |emulation - float64| / bound per epilogue (plain, residual, SwiGLU, rotary): {[round(worst[e], 3) for e in range(4)]}")


# the forms a mutant can show in
_WHERE = {"rotate_half_sign": LC.ROPE, "position_from_slot": LC.ROPE, "slot_from_position": LC.ROPE, "lora_scale_dropped": None,
          "lora_after_rotation": LC.ROPE, "residual_dropped": LC.RES, "gain_before_rsqrt": None, "silu_on_up": LC.SWIGLU}


@pytest.mark.parametrize("mutant", sorted(_WHERE))
@pytest.mark.parametrize("dtype", LC.DTYPES, ids=["f16", "bf16"])
def test_named_mutants_are_outside_the_bound(dtype, mutant):
    hit = 0
    for ci, c in enumerate(CASES):
        if _WHERE[mutant] is not None and c["epi"] != _WHERE[mutant]:
            continue
        if mutant.startswith("lora") and not any(c["R"][:2 if c["epi"] == LC.ROPE and mutant == "lora_after_rotation" else 3]):
            continue
        if mutant == "gain_before_rsqrt" and not c["norm"]:
            continue
        got = LC.emulate(ci, dtype, mutant)
        if mutant == "slot_from_position":          # the k / v rows land in another slot: the right slot keeps what it held
            assert got["slot"] != LC.reference(ci, dtype)[1]["slot"]
            hit += 1
            continue
        r = LC.ratios(ci, dtype, got)
        assert r > 1.0, (LC.case_id(c), mutant, r)
        hit += 1
    assert hit >= 2


def test_argmax_order_ties_and_nan():
    for V in LC.HEAD_V:
        z = LC.argmax_case(V)
        got = LS.argmax_ref(z)
        for b in range(z.shape[0]):
            row = z[b]
            want = int(torch.isnan(row).nonzero()[0]) if torch.isnan(row).any() else int((row == row.max()).nonzero()[0])
            assert int(got[b]) == want
        if not torch.isnan(z).any():
            assert torch.equal(got, torch.argmax(z, -1))
        if V >= 63:
            assert not torch.equal(LS.argmax_ref(z, "argmax_tie_highest"), got)       # the planted ties tell the two orders apart
    tok, fin = LS.greedy_ref(torch.tensor([4, 2, 9, 7]), torch.tensor([0, 0, 1, 0]), pad=0, eos=[2, 7])
    assert tok.tolist() == [4, 2, 0, 7] and fin.tolist() == [False, True, True, True]


# ---- 3. the mutants a whole step shows: each misses the pin the definition holds -----------------------------------------------------------------
@pytest.mark.parametrize("mutant", LS.MUTANTS)
def test_every_step_mutant_misses_the_own_forward_pin(mutant):
    llm = LC.tiny_llama(2, 64, lora=True)
    B, S0 = 3, 21
    embeds, mask = LC.prefix(B, S0, llm.config.hidden_size)
    tok = torch.tensor([5, 17, 96])
    with torch.no_grad():
        want, kv, nxt = _own_step(llm, embeds, mask, tok)
    cache = torch.zeros(kv.shape[0], 2, B, 2, S0 + 24, 64)
    cache[:, :, :, :, :S0] = kv
    m = torch.ones(B, S0 + 24, dtype=torch.uint8)
    m[:, :S0] = mask.to(torch.uint8)
    got, _ = LS.lm_step_ref(llm, tok, cache.clone(), m, nxt, S0, dtype=None, compute=torch.float32)
    bad, _ = LS.lm_step_ref(llm, tok, cache.clone(), m, nxt, S0, dtype=None, compute=torch.float32, mutant=mutant)
    d = (bad - want).abs().max().item()
    assert (got - want).abs().max().item() <= 1e-5 < d, (mutant, d)


# ---- 3b. the chain: the worst-case bound is vacuous (evaluated here), the stated margin tells the definition from its mutants ----------------
def _chain_setup(kv_heads, lora, dtype):
    llm = LC.tiny_llama(kv_heads, 64, vocab=260, lora=lora).to(dtype)
    if lora:                                                      # the adapters stay fp32 masters
        from mraudio_amd.models.lora import lora_modules

        for m in lora_modules(llm).values():
            m.lora_A.float(), m.lora_B.float()
    B, S0 = 3, 19
    g = torch.Generator().manual_seed(4)
    cache = (torch.randn(llm.config.num_hidden_layers, 2, B, kv_heads, S0 + 3, 64, generator=g) * 0.5).to(dtype)
    _, mask = LC.prefix(B, S0, 8)
    m = torch.ones(B, S0 + 3, dtype=torch.uint8)
    m[:, :S0] = mask.to(torch.uint8)
    return llm, torch.tensor([5, 17, 96]), cache, m, mask.sum(-1), S0, LS.rope_table(llm, S0 + 8, torch.device("cpu"))


@pytest.mark.parametrize("dtype", LC.DTYPES, ids=["f16", "bf16"])
def test_worst_case_chain_bound_is_vacuous(dtype):
    llm, tok, cache, m, pos, slot, rope = _chain_setup(2, False, dtype)
    trace = []
    ref, bnd = LC.step_with_bound(llm, tok, cache.clone(), m, pos, slot, dtype, rope, trace)
    same, _ = LS.lm_step_ref(llm, tok, cache.clone(), m, pos, slot, dtype=dtype, compute=torch.float64, rope=rope)
    assert torch.equal(same, ref)                                 # the bound-carrying forward IS lm_step_ref in float64
    print(f"{dtype}: relative worst-case bound along the first layer {[(n, float(f'{r:.3g}')) for n, r in trace]}; finite bounds on the logits: "
          f"{int(torch.isfinite(bnd).sum())} of {bnd.numel()}")
    rel = dict(trace)
    assert rel["o product"] > 20 * rel["q"] and rel["second norm"] > 0.15       # a 16-bit ulp at q, tens of it behind |W_o|, no use at the norm
    assert not torch.isfinite(bnd).any() or (bnd.min() > ref.abs().max()).item()      # nothing usable reaches the logits


@pytest.mark.parametrize("lora", [False, True], ids=["plain", "lora"])
@pytest.mark.parametrize("dtype", LC.DTYPES, ids=["f16", "bf16"])
def test_chain_margin_holds_the_fp32_step_and_no_step_mutant(dtype, lora):
    llm, tok, cache, m, pos, slot, rope = _chain_setup(2, lora, dtype)
    ref, _ = LS.lm_step_ref(llm, tok, cache.clone(), m, pos, slot, dtype=dtype, compute=torch.float64, rope=rope)
    bar = LC.chain_margin(ref, dtype)
    got, _ = LS.lm_step_ref(llm, tok, cache.clone(), m, pos, slot, dtype=dtype, compute=torch.float32, rope=rope)
    d = (got.double() - ref).abs().max().item()
    out = {}
    for mutant in LS.MUTANTS:
        if mutant.startswith("lora") and not lora:
            continue
        bad, _ = LS.lm_step_ref(llm, tok, cache.clone(), m, pos, slot, dtype=dtype, compute=torch.float32, mutant=mutant, rope=rope)
        out[mutant] = (bad.double() - ref).abs().max().item() / bar
    print(f"{dtype} lora {lora}: fp32 step {d / bar:.3g} of the margin; mutants {dict((k, round(v, 1)) for k, v in out.items())}")
    assert d <= bar
    assert min(out.values()) > 1.0, out


# ---- 4. the C entries: refusals before any launch, the workspace formula -------------------------------------------------------------------------
def _step_desc():
    """A descriptor every check accepts up to the launch -- with fake (aligned, never followed) addresses: used for refusals only."""
    d = _lib.mra_lm_step_desc()
    d.struct_bytes = C.sizeof(d)
    d.B, d.hidden, d.intermediate, d.Hq, d.Hkv, d.D, d.L, d.V, d.dtype, d.Smax = 3, 256, 512, 4, 2, 64, 1, 260, _lib.MRA_BF16, 40
    d.eps, d.attn_scale = 1e-6, 0.125
    lay = (_lib.mra_lm_layer * 1)()
    fake = 0x10000
    lay[0].norm1 = lay[0].norm2 = lay[0].kcache = lay[0].vcache = fake
    for n, (N, K) in dict(q=(256, 256), k=(128, 256), v=(128, 256), o=(256, 256), gate=(512, 256), up=(512, 256), down=(256, 512)).items():
        lin = getattr(lay[0], n)
        lin.W, lin.ldw, lin.N = fake, K, N
    d.layers = lay
    d.embed = d.final_norm = d.head = d.mask = d.position = d.cos = d.sin = d.tokens_in = d.h = d.logits = d.tokens_out = d.workspace = fake
    d.ld_embed = d.ld_head = 256
    d.k_sb, d.k_sh, d.k_ss = 2 * 40 * 64, 40 * 64, 64
    d.v_sb, d.v_sh, d.v_ss = 2 * 40 * 64, 40 * 64, 64
    d.mask_sb, d.slot, d.rope_ld, d.rope_rows, d.ld_logits = 40, 7, 64, 41, 260
    d.workspace_bytes = LS.step_workspace_bytes(3, 256, 512, 4, 64, 40)
    d._keep = lay
    return d


def _refused(d, word):
    assert _lib.lib().mra_lm_step(C.byref(d), None) == -1
    msg = _lib.lib().mra_last_error().decode()
    assert word in msg, msg


def test_lm_step_refusals_and_workspace_formula():
    lib = _lib.lib()
    for args in ((1, 256, 512, 4, 64, 40), (8, 4096, 11008, 32, 128, 1964), (3, 264, 72, 8, 64, 257), (2, 64, 8, 2, 128, 1)):
        assert lib.mra_lm_step_workspace_bytes(*args) == LS.step_workspace_bytes(*args)
        B, H, I, Hq, D, S = args
        assert LS.step_workspace_bytes(*args) == LC.up256(4 * B * H) + 3 * LC.up256(64 * B) + 2 * LC.up256(2 * B * Hq * D) + LC.up256(2 * B * I) \
            + lib.mra_decode_attention_workspace_bytes(B, Hq, S, D)
    for bad in ((0, 256, 512, 4, 64, 40), (9, 256, 512, 4, 64, 40), (1, 260, 512, 4, 64, 40), (1, 256, 516, 4, 64, 40), (1, 256, 512, 4, 96, 40),
                (1, 256, 512, 4, 64, 0)):
        assert lib.mra_lm_step_workspace_bytes(*bad) == 0
    assert lib.mra_lm_step(None, None) == -1

    def with_(**kw):
        d = _step_desc()
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    _refused(with_(struct_bytes=8), "struct_bytes")
    _refused(with_(B=0), "B must be in 1..8")
    _refused(with_(B=9), "B must be in 1..8")
    _refused(with_(hidden=260), "multiples of 8")
    _refused(with_(intermediate=516), "multiples of 8")
    _refused(with_(D=96), "D must be 64 or 128")
    _refused(with_(Hq=6, Hkv=2), "1, 2, 4 or 8")
    _refused(with_(Hq=4, Hkv=3), "multiple of Hkv")
    _refused(with_(slot=40), "slot")
    _refused(with_(slot=-1), "slot")
    _refused(with_(h=0), "null")
    _refused(with_(workspace=0), "null")
    _refused(with_(head=0x10008), "16-byte aligned")
    _refused(with_(position=0x10002), "4-byte aligned")
    _refused(with_(workspace_bytes=LS.step_workspace_bytes(3, 256, 512, 4, 64, 40) - 1), "workspace too small")
    _refused(with_(eps=float("nan")), "finite")
    _refused(with_(eps=float("inf")), "finite")
    _refused(with_(dtype=_lib.MRA_F32), "dtype")
    _refused(with_(n_eos=9), "n_eos")
    _refused(with_(k_ss=60), "strides")
    _refused(with_(ld_head=250), "ld_head")
    d = _step_desc()
    d._keep[0].q.R = 17
    _refused(d, "R must be in 0..16")
    d = _step_desc()
    d._keep[0].down.R, d._keep[0].down.A = 4, 0
    _refused(d, "null adapter")
    d = _step_desc()
    d._keep[0].k.N = 256
    _refused(d, "N is not the layer's")
    d = _step_desc()
    d._keep[0].o.W = 0x10004
    _refused(d, "16-byte aligned")
    d = _step_desc()
    d._keep[0].kcache = 0
    _refused(d, "null")


def _skinny_desc(epi=LC.PLAIN):
    d = _lib.mra_lm_skinny_desc()
    d.struct_bytes = C.sizeof(d)
    fake = 0x10000
    d.B, d.K, d.dtype, d.epilogue, d.nseg = 2, 64, _lib.MRA_F16, epi, 1
    d.x, d.ldx, d.x_bytes, d.eps = fake, 64, 2 * 2 * 64, 1e-6
    d.seg[0].W, d.seg[0].ldw, d.seg[0].N = fake, 64, 17
    d.w_bytes[0] = 2 * 17 * 64
    d.out[0], d.ldo[0], d.out_bytes[0] = fake, 24, 2 * (24 + 17)
    d.res, d.ldres, d.res_bytes = fake, 24, 2 * (24 + 17)
    return d


def test_debug_lm_skinny_refusals():
    lib = _lib.lib()

    def refused(d, word):
        assert lib.mra_debug_lm_skinny(C.byref(d), None) == -1
        msg = lib.mra_last_error().decode()
        assert word in msg, msg

    def with_(epi=LC.PLAIN, **kw):
        d = _skinny_desc(epi)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    assert lib.mra_debug_lm_skinny(None, None) == -1
    refused(with_(struct_bytes=16), "struct_bytes")
    refused(with_(epilogue=4), "epilogue")
    refused(with_(B=9), "B must be in 1..8")
    refused(with_(K=60), "K must be")
    refused(with_(nseg=4), "nseg")
    refused(with_(x=0), "x must be")
    refused(with_(x=0x10008), "x must be")
    refused(with_(ldx=56), "ldx")
    refused(with_(ldx=68), "ldx")
    refused(with_(x_bytes=2 * 2 * 64 - 2), "x footprint")
    refused(with_(eps=float("nan")), "eps")
    refused(with_(LC.RES, out_f32=1), "fp32 output")
    refused(with_(LC.RES, res=0), "res must be")
    refused(with_(LC.RES, res_bytes=2 * (24 + 17) - 2), "res footprint")
    refused(with_(LC.RES, ldres=16), "ldres")
    refused(with_(LC.SWIGLU), "SwiGLU")
    refused(with_(LC.ROPE), "D must be")
    d = with_()
    d.w_bytes[0] -= 2
    refused(d, "W footprint")
    d = with_()
    d.out_bytes[0] -= 2
    refused(d, "out footprint")
    d = with_()
    d.ldo[0] = 16
    refused(d, "ldo")
    d = with_()
    d.out[0] = 0
    refused(d, "out must be")
    d = with_()
    d.seg[0].R, d.seg[0].A, d.seg[0].Bw = 17, 0x10000, 0x10000
    refused(d, "R must be in 0..16")
    d = with_()
    d.seg[0].R, d.seg[0].A, d.seg[0].Bw = 4, 0x10000, 0x10000
    refused(d, "workspace")
    d.workspace, d.workspace_bytes = 0x10000, LC.skinny_workspace_bytes(2, 64) - 1
    refused(d, "workspace too small")
    # the rotary form: slot beyond the cache, Hq / Hkv, D
    d = with_(LC.ROPE, nseg=3, Hq=4, Hkv=2, D=64, slot=9, rope_rows=8, rope_ld=64, rope_bytes=4 * 8 * 64)
    for s, N in enumerate((256, 128, 128)):
        d.seg[s].W, d.seg[s].ldw, d.seg[s].N, d.w_bytes[s] = 0x10000, 64, N, 2 * N * 64
    d.out[0], d.ldo[0], d.out_bytes[0] = 0x10000, 256, 2 * 2 * 256
    d.position = d.cos = d.sin = d.kcache = d.vcache = 0x10000
    d.k_sb, d.k_sh, d.k_ss = 2 * 9 * 64, 9 * 64, 64
    d.v_sb, d.v_sh, d.v_ss = 2 * 9 * 64, 9 * 64, 64
    d.kcache_bytes = d.vcache_bytes = 2 * 2 * 2 * 9 * 64
    refused(d, "slot beyond the cache")
    d.slot, d.Hq, d.Hkv = 8, 6, 2
    refused(d, "1, 2, 4 or 8")
    d.Hq, d.Hkv, d.rope_bytes = 4, 2, 4 * 8 * 64 - 4
    refused(d, "rotary footprint")
    assert lib.mra_debug_lm_argmax(None, 4, 1, 4, None, None, 0, None, 0, None) == -1
    assert lib.mra_debug_lm_argmax(C.c_void_p(0x10000), 3, 1, 4, C.c_void_p(0x10000), None, 0, None, 0, None) == -1
    assert lib.mra_debug_lm_argmax(C.c_void_p(0x10000), 4, 1, 4, C.c_void_p(0x10000), None, 0, None, 9, None) == -1


# ---- 5. HipLmDecoder's refusals ----------------------------------------------------------------------------------------------------------------------
def test_hip_lm_decoder_refuses_what_is_not_llama_shaped():
    with pytest.raises(_lib.MraError, match="has a bias"):
        LS.HipLmDecoder(LC.tiny_llama(2, 64, attention_bias=True).to(torch.bfloat16))
    with pytest.raises(_lib.MraError, match="has a bias"):
        LS.HipLmDecoder(LC.tiny_llama(2, 64, mlp_bias=True).to(torch.bfloat16))
    with pytest.raises(_lib.MraError, match="hidden_act must be 'silu', found 'gelu'"):
        LS.HipLmDecoder(LC.tiny_llama(2, 64, hidden_act="gelu").to(torch.bfloat16))
    with pytest.raises(_lib.MraError, match="found Linear"):
        LS.HipLmDecoder(torch.nn.Linear(8, 8))
    gpt = tf.GPT2LMHeadModel(tf.GPT2Config(n_layer=1, n_head=2, n_embd=16, vocab_size=32))
    with pytest.raises(_lib.MraError, match="found GPT2LMHeadModel"):
        LS.HipLmDecoder(gpt)
    with pytest.raises(_lib.MraError, match="float16 or bfloat16, found torch.float32"):
        LS.HipLmDecoder(LC.tiny_llama(2, 64))
    mixed = LC.tiny_llama(2, 64).to(torch.bfloat16)
    mixed.model.layers[1].post_attention_layernorm.float()                             # a norm kept in fp32: its gain is not what the kernel reads
    with pytest.raises(_lib.MraError, match="layer 1 norm2 must be torch.bfloat16"):
        LS.HipLmDecoder(mixed)
    mixed = LC.tiny_llama(2, 64).to(torch.bfloat16)
    mixed.model.norm.float()
    with pytest.raises(_lib.MraError, match="model.norm.weight must be torch.bfloat16"):
        LS.HipLmDecoder(mixed)
    mixed = LC.tiny_llama(2, 64).to(torch.bfloat16)
    mixed.model.embed_tokens.float()
    with pytest.raises(_lib.MraError, match="embed_tokens.weight must be torch.bfloat16"):
        LS.HipLmDecoder(mixed)
    with pytest.raises(_lib.MraError, match="head_dim 32"):
        LS.HipLmDecoder(LC.tiny_llama(2, 32).to(torch.bfloat16))
    with pytest.raises(_lib.MraError, match="fp32 masters"):                          # .to() rounds the adapters: refused as such
        LS.HipLmDecoder(LC.tiny_llama(2, 64, lora=True).to(torch.bfloat16))
    llm = LC.tiny_llama(4, 64).to(torch.float16)
    dec = LS.HipLmDecoder(llm)
    w, layers = dec._table()
    first = dec._sig
    assert layers[0].q.W == llm.model.layers[0].self_attn.q_proj.weight.data_ptr() and layers[0].q.R == 0 and layers[1].down.N == 256
    dec._table()
    assert dec._sig is first or dec._sig == first
    LC.add_adapters(llm)
    _, layers = dec._table()                                                          # an adapter appeared: the table is rebuilt
    assert dec._sig != first and layers[0].q.R == 8 and layers[0].q.scale == 2.0
    with pytest.raises(_lib.MraError, match="CUDA"):
        dec.generate(torch.zeros(1, 4, 256, dtype=torch.float16), torch.ones(1, 4, dtype=torch.long), 2)


# ---- 6. the greedy loop against generate ---------------------------------------------------------------------------------------------------------------
def _counting_llama(vocab=61):
    """A tiny Llama rigged to count: o_proj and down_proj are zero, so the residual stream stays the token's embedding row E[v], and lm_head's row
    v + 1 is E[v]: the token after v is v + 1 (mod vocab), whatever the prefix holds.  Attention, rotary and the MLP still run."""
    llm = LC.tiny_llama(2, 64, vocab=vocab)
    E = torch.randn(vocab, llm.config.hidden_size, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        for layer in llm.model.layers:
            layer.self_attn.o_proj.weight.zero_()
            layer.mlp.down_proj.weight.zero_()
        llm.model.norm.weight.fill_(1.0)
        llm.model.embed_tokens.weight.copy_(E)
        llm.lm_head.weight.copy_(torch.roll(E, 1, 0))
    return llm, E


@pytest.mark.parametrize("pad", [0, None], ids=["pad0", "pad_is_eos"])
def test_greedy_loop_is_generates_with_eos_at_different_steps(pad):
    llm, E = _counting_llama()
    B, S0, n = 3, 17, 12
    embeds, mask = LC.prefix(B, S0, llm.config.hidden_size)
    for b, start in enumerate((10, 20, 30)):
        embeds[b, -1] = E[start]
    llm.generation_config.eos_token_id, llm.generation_config.pad_token_id = None, pad
    with torch.no_grad():
        free = llm.generate(inputs_embeds=embeds, attention_mask=mask, max_new_tokens=n, do_sample=False)
    assert free.tolist() == [[start + 1 + j for j in range(n)] for start in (10, 20, 30)]
    eos = [14, 27, 39]                                                                 # the sequences finish at steps 3, 6 and 8
    llm.generation_config.eos_token_id = eos
    with torch.no_grad():
        want = llm.generate(inputs_embeds=embeds, attention_mask=mask, max_new_tokens=n, do_sample=False)
    dec = LS.HipLmDecoder(llm, ref=True)
    dec.check_every = 3
    got = dec.generate(embeds, mask, n)
    print(f"eos ids {eos}, pad {pad}: generate stops after {want.shape[1]} of {n} tokens; rows {want.tolist()}")
    assert want.shape[1] == 9 and got.dtype == torch.int64
    assert torch.equal(got, want)
    fill = 0 if pad == 0 else eos[0]
    assert want[0, 4:].tolist() == [fill] * 5 and want[1, 7:].tolist() == [fill] * 2    # pad behind each sequence's eos
    full = dec.generate(embeds, mask, n, ignore_eos=True)
    assert full.shape == (B, n) and torch.equal(full, free)
    llm.generation_config.eos_token_id = None
    assert torch.equal(dec.generate(embeds, mask, n), free)                            # no eos: every token, as generate
    llm.generation_config.eos_token_id = eos
    many = dec.generate(embeds.repeat(4, 1, 1)[:11], mask.repeat(4, 1)[:11], n)          # more than 8 sequences: blocks of 8
    assert torch.equal(many, want.repeat(4, 1)[:11])


# ---- 7. the public switches -----------------------------------------------------------------------------------------------------------------------------
def test_cli_flags_and_constructor_take_hip_step(capsys):
    from mraudio_amd import evaluate, finetune
    from mraudio_amd.models.xinstructblip import XInstructBLIP

    args = finetune.build_parser().parse_args(["--output-dir", "out", "--dataset", "QVH", "--lm-decode", "hip_step"])
    assert args.lm_decode == "hip_step"
    ep = evaluate.build_parser()
    flags = {a.dest: a for a in ep._actions}
    assert flags["lm_step"].default is False and flags["lm_decode"].default == "stock"
    with pytest.raises(SystemExit) as e:                                                # two flags, one setting: never silently
        evaluate.main(["--output-file", "out.json", "--lm-step", "--lm-decode", "hip"])
    assert e.value.code == 2 and "--lm-step and --lm-decode hip" in capsys.readouterr().err
    assert XInstructBLIP.lm_decode == "stock"                                           # the default is what it was
    with pytest.raises(ValueError, match="'stock', 'hip' or 'hip_step'"):
        XInstructBLIP(seed=0, device="cpu", lm_decode="fast")
