"""No GPU: the case families, float64 references and the derived bound of ``tests/attention_cases.py`` -- what
``tests/test_gpu_encoder_cores.py`` holds the HIP attention cores to -- checked against a plain fp32 / 16-bit emulation of the kernels'
arithmetic and against three deliberately wrong versions of it.  This proves on a machine without a GPU that the GPU test is sensitive
(a kernel that left ONE zero padding key unmasked, or whose softmax scale was 1 % off, could not pass it), that a correct kernel has
room (the emulation's worst ratio is printed), and it guards the reference code itself."""
import math

import pytest
import torch

import attention_cases as AC

HD = 88                       # the ViT-g head dimension
LENGTHS = (2, 122, 257)       # one fragment, a partially valid fragment, ViT-g/224
UNITS = 6


def _ratio(kind, S, dtype, mutant=None, hd=HD):
    q, k, v = AC.make_qkv(kind, UNITS, S, hd, dtype)
    ref, bound, p = AC.attention_ref(q, k, v)
    return AC.worst_ratio(AC.emulate(q, k, v, mutant=mutant), ref, bound), p


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_the_emulated_kernel_arithmetic_stays_within_the_bound_on_every_family(dtype):
    worst = {}
    for S in LENGTHS:
        for kind in AC.families_for(S):
            r, _ = _ratio(kind, S, dtype)
            worst[(kind, S)] = r
            assert r <= 1.0, (kind, S, dtype, r)
    print(f"emulation {dtype}: worst |d| / bound {max(worst.values()):.3f} at {max(worst, key=worst.get)}")


def test_the_families_are_what_their_names_say():
    q, k, v = AC.make_qkv("peaked", UNITS, 257, HD)
    _, _, p = AC.attention_ref(q, k, v)
    med = p.max(-1).values.median().item()
    assert 0.4 <= med <= 0.75, med                                    # "about 0.57 at S = 257"
    _, _, p = AC.attention_ref(*AC.make_qkv("mild", UNITS, 257, HD))
    assert p.max(-1).values.median().item() < 0.05                    # near-uniform rows
    q, k, v = AC.make_qkv("negative", UNITS, 257, HD)
    s = q.double() @ k.double().transpose(-1, -2) / math.sqrt(HD)
    assert s.max().item() < -10.0                                     # every valid score far below a padding key's zero
    for kind in AC.families_for(257):
        if kind.startswith("onehot"):
            t = 256 if kind == "onehot_last" else int(kind.split("@")[1])
            _, _, p = AC.attention_ref(*AC.make_qkv(kind, UNITS, 257, HD))
            assert (p.argmax(-1) == t).all() and p[..., t].min().item() > 0.5, kind
    ref, _, p = AC.attention_ref(*AC.make_qkv("constant", UNITS, 122, HD))
    v = AC.make_qkv("constant", UNITS, 122, HD)[2]
    assert (p - 1.0 / 122).abs().max().item() < 1e-12 and (ref - v.double().mean(1, keepdim=True)).abs().max().item() < 1e-12
    assert AC.families_for(2) == ["mild", "peaked", "negative", "constant", "onehot_last", "onehot@0"]
    assert len(AC.families_for(257)) == len(AC.VIT_FAMILIES)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_every_mutant_exceeds_the_bound_on_its_named_family(dtype):
    for S in LENGTHS:
        # one zero padding key left unmasked: invisible on ``mild`` (that is why ``negative`` exists), far outside on ``negative``
        r, _ = _ratio("negative", S, dtype, "pad1")
        assert r > 1.0, ("pad1", S, r)
        # the last key never seen: in f16 it fails on every family at every length.  The bf16 bound is eight times wider and one key of 257
        # near-equal ones weighs less than it: there the families that carry weight on the last key show it (the kernels are one template
        # over the dtype, and the f16 run of the same families sees the rest)
        for kind in AC.families_for(S) if dtype == torch.float16 else ("mild", "peaked", "onehot_last"):
            r, _ = _ratio(kind, S, dtype, "drop_last")
            assert r > 1.0, ("drop_last", kind, S, r)
    # a softmax scale 1 % off needs sharp rows to show
    r, _ = _ratio("peaked", 257, dtype, "scale")
    assert r > 1.0, ("scale", r)
    r, _ = _ratio("peaked", 122, dtype, "scale")
    assert r > 1.0, ("scale", 122, r)


def test_f16_mutant_margins_at_257():
    """The figures the case families were chosen by (f16, hd = 88, S = 257): ``pad1`` is two orders of magnitude outside on ``negative`` and
    INSIDE on ``mild``; ``scale`` is an order of magnitude outside on ``peaked``."""
    pad_neg, _ = _ratio("negative", 257, torch.float16, "pad1")
    pad_mild, _ = _ratio("mild", 257, torch.float16, "pad1")
    sc_peak, _ = _ratio("peaked", 257, torch.float16, "scale")
    print(f"pad1: {pad_neg:.1f} x bound on negative, {pad_mild:.2f} x on mild; scale: {sc_peak:.1f} x on peaked")
    assert pad_neg > 1.0 and pad_mild < 1.0 and sc_peak > 1.0


def test_beats_families_bias_reference_and_mutants():
    """hd = 64 with the gated relative-position bias: the emulation within the bound for both bias tables and both gate sources, the
    peaked table peaks the rows on its own (mean row maximum of the bias alone > 0.4, the existing whole-encoder test's criterion), and the
    mutants are caught here too."""
    heads = 4
    for P in (8, 24, 136, 264):
        for scale in (1.0, AC.PEAKED_BIAS_SCALE):
            pr = AC.beats_core_params(heads, bias_scale=scale)
            kinds = AC.families_for(P, AC.BEATS_FAMILIES) if scale == 1.0 else ["mild"]
            q, k, v = AC.make_units(kinds, heads, P, 64, torch.float16)
            layer_in = torch.randn(len(kinds), heads, P, 64, generator=torch.Generator().manual_seed(P)).half()
            for src in (q, layer_in):
                ref, bound, p = AC.beats_attention_ref(q, k, v, src, pr["E"], pr["gw"], pr["gb"], pr["ga"])
                bias = AC.beats_gate(src, pr["gw"], pr["gb"], pr["ga"]) * AC.beats_position_bias(pr["E"], P)[None]
                r = AC.worst_ratio(AC.emulate(q, k, v, bias=bias), ref, bound)
                assert r <= 1.0, (P, scale, r)
                for ci, kind in enumerate(kinds):
                    rd = AC.worst_ratio(AC.emulate(q[ci], k[ci], v[ci], bias=bias[ci], mutant="drop_last"), ref[ci], bound[ci])
                    assert rd > 1.0, ("drop_last", kind, P, scale, rd)
                ni = kinds.index("negative") if "negative" in kinds else None
                if ni is not None:
                    rp = AC.worst_ratio(AC.emulate(q[ni], k[ni], v[ni], bias=bias[ni], mutant="pad1"), ref[ni], bound[ni])
                    assert rp > 1.0, ("pad1", P, rp)
            if scale != 1.0 and P >= 136:
                peak = torch.softmax(AC.beats_position_bias(pr["E"], P), -1).max(-1).values.mean().item()
                assert peak > 0.4, (P, peak)
    # the gate and the bucket table are those of the model: one layer's attention through models/beats.py against the reference
    from mraudio_amd.models.beats import BEATs, BEATsConfig
    m = BEATs(BEATsConfig(encoder_layers=1)).eval().init_seeded_(3).double()
    att = m.encoder.layers[0].self_attn
    x = torch.randn(2, 24, 768, generator=torch.Generator().manual_seed(1)).double()
    with torch.no_grad():
        want = att(x, m.encoder.position_bias(24))
        hv = lambda t: t.view(2, 24, 12, 64).transpose(1, 2)
        q, k, v = hv(att.q_proj(x)), hv(att.k_proj(x)), hv(att.v_proj(x))
        s = q @ k.transpose(-1, -2) / 8.0 + AC.beats_gate(q, att.grep_linear.weight, att.grep_linear.bias, att.grep_a.view(-1)) * \
            AC.beats_position_bias(att.relative_attention_bias.weight, 24)[None]
        got = att.out_proj((torch.softmax(s, -1) @ v).transpose(1, 2).reshape(2, 24, 768))
    assert (got - want).abs().max().item() < 1e-6        # the module's softmax runs in fp32


def test_posconv_reference_is_the_models_convolution_and_the_bound_has_room():
    from mraudio_amd.models.beats import BEATs, BEATsConfig
    x, w, b = AC.make_posconv(2, 24)
    assert 3.0 < x.abs().max().item() <= 4.0
    ref, bound = AC.posconv_ref(x, w, b)
    # the same stage through the restatement's module, in float64 on the f16-rounded operands
    m = BEATs(BEATsConfig(encoder_layers=1)).double()
    conv = m.encoder.pos_conv[0]
    with torch.no_grad():
        conv.weight_g.copy_(w.half().double().norm(dim=(0, 1), keepdim=True))
        conv.weight_v.copy_(w.half().double())
        conv.bias.copy_(b.double())
        x16 = x.half().double()
        want = x.double() + torch.nn.functional.gelu(conv(x16.transpose(1, 2))[:, :, :24]).transpose(1, 2)
    assert (ref - want).abs().max().item() < 1e-12
    # a plain fp32 evaluation sits far inside the bound; one tap shifted by a token does not
    x16f, w16f = x.half().float().transpose(1, 2), w.half().float()
    pre = torch.nn.functional.conv1d(x16f, w16f, b, padding=64, groups=16)[..., :24].transpose(1, 2)
    out = x + torch.nn.functional.gelu(pre)
    assert AC.worst_ratio(out, ref, bound) <= 1.0
    shifted = torch.nn.functional.conv1d(x16f, w16f, b, padding=64, groups=16)[..., 1:25].transpose(1, 2)
    assert AC.worst_ratio(x + torch.nn.functional.gelu(shifted), ref, bound) > 1.0
