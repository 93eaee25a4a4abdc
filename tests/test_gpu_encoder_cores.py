"""``-m gpu``: the encoders' attention cores and the BEATs positional convolution, each on its own through the stage entry points
(``mra_debug_vit_attention`` / ``mra_debug_beats_attention`` / ``mra_debug_beats_posconv``: the forwards' own launch code), against float64
references on the same rounded inputs.  EVERY element of every output is held to the derived per-element bound of
``tests/attention_cases.py`` (4 u A + S 2^-24 max|v| for attention, K 2^-24 B + 2^-20 (1 + |pre|) for the convolution); the bound is not
measured and the emulated kernel arithmetic sits at <= 0.36 of it (``tests/test_attention_cases_cpu.py``), so a ratio above 1.0 is a defect.

What the whole-encoder tests cannot see and this file does: one unmasked padding key (``negative``), a softmax scale off by 1 %
(``peaked``), a wrong row sum, a wrong key at a fragment or mask boundary (``onehot@0/15/16/255/256``, ``onehot_last``) -- at all 16 reachable
ViT lengths, both operand dtypes, 16 and 8 heads, the persistent ViT core at three unit counts, and for BEATs at 13 token counts around
the 64-token convolution window, the 128-key softmax chunks and the 256 / 264 switch between the two LDS instantiations.

Canaries: ``qkv`` / ``x`` are slices of a larger allocation whose rows before and after are NaN (a read outside the batch cannot stay
silent); ``ctx`` is NaN-prefilled with guard rows around it: the guards must stay bit for bit, the inside must come out finite (so every
element was written)."""
import ctypes as C
import time

import pytest
import torch

import attention_cases as AC
from mraudio_amd import _lib as L

pytestmark = pytest.mark.gpu

GUARD = 16
VIT_GEOMETRIES = {"16 heads": (1408, 16), "8 heads": (704, 8)}
BEATS_TOKENS = (8, 16, 24, 120, 128, 136, 248, 256, 264, 384, 496, 504, 512)
POSCONV_TOKENS = (8, 24, 56, 64, 72, 128, 200, 256, 496, 512)
DT = {"f16": (torch.float16, L.MRA_F16), "bf16": (torch.bfloat16, L.MRA_BF16)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _stream():
    return L.current_stream()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


class _Handle:
    """A library handle created straight through the C ABI (no parameter container: the cores need few or no parameters)."""

    def __init__(self, prefix, cfg):
        self.prefix, self.h = prefix, C.c_void_p()
        L.check(getattr(L.lib(), prefix + "_create")(C.byref(cfg), C.byref(self.h)), prefix + "_create")

    def load(self, name, t):
        shape = (C.c_int64 * max(t.dim(), 1))(*t.shape)
        L.check(getattr(L.lib(), self.prefix + "_load")(self.h, name.encode(), L.ptr(t), L.mra_dtype(t.dtype), shape, t.dim(), _stream()), name)

    def close(self):
        if self.h:
            getattr(L.lib(), self.prefix + "_destroy")(self.h)
            self.h = C.c_void_p()


def _vit(dim, heads, img, op, depth=1):
    return _Handle("mra_vit", L.mra_vit_cfg(dim, heads, 256, depth, 14, img, 1e-6, op, L.MRA_F32))    # mlp 256: the smallest create accepts


def _beats_cfg(gate, dim=768, heads=12):
    cfg = L.mra_beats_cfg()
    L.lib().mra_beats_cfg_default(C.byref(cfg))
    cfg.dim, cfg.heads, cfg.layers, cfg.ffn, cfg.embed_dim, cfg.gate_from, cfg.conv_pos_groups = dim, heads, 1, 256, 256, gate, max(dim // 48, 1)
    return cfg


def _guarded(inner, fill=float("nan")):
    """``inner`` [rows, width] (CPU) in the middle of a device allocation with GUARD rows of ``fill`` on either side."""
    rows = inner.shape[0]
    buf = torch.full((rows + 2 * GUARD, inner.shape[1]), fill, dtype=inner.dtype, device="cuda:0")
    buf[GUARD:GUARD + rows] = inner.to(buf.device)
    return buf


def _check_output_region(buf, before, rows, what):
    assert torch.equal(_bits(buf[:GUARD]), _bits(before[:GUARD])) and torch.equal(_bits(buf[GUARD + rows:]), _bits(before[GUARD + rows:])), \
        f"{what}: rows outside the output region were written"
    assert torch.isfinite(buf[GUARD:GUARD + rows]).all().item(), f"{what}: non-finite or unwritten output elements"


def _units(kinds, heads, S, hd, dtype):
    """One frame / chunk per entry of ``kinds`` (repeats get their own seed)."""
    parts = [AC.make_qkv(kind, heads, S, hd, dtype, seed=None if kinds.index(kind) == i else 7000 + i) for i, kind in enumerate(kinds)]
    return tuple(torch.stack([p[i] for p in parts]) for i in range(3))


def _run_vit_core(h, q, k, v):
    n, heads, S, hd = q.shape
    qkv = _guarded(AC.pack_vit_qkv(q, k, v))
    ctx = torch.full((n * S + 2 * GUARD, heads * hd), float("nan"), dtype=q.dtype, device=qkv.device)
    qkv0, ctx0 = qkv.clone(), ctx.clone()
    L.check(L.lib().mra_debug_vit_attention(h.h, L.ptr(qkv[GUARD:]), n, L.ptr(ctx[GUARD:]), _stream()), "mra_debug_vit_attention")
    torch.cuda.synchronize()
    assert torch.equal(_bits(qkv), _bits(qkv0)), "the input was written"
    _check_output_region(ctx, ctx0, n * S, "vit ctx")
    return AC.unpack_ctx(ctx[GUARD:GUARD + n * S].cpu(), n, heads)


def _ratios_per_item(out, ref, bound):
    return [AC.worst_ratio(out[i], ref[i], bound[i]) for i in range(out.shape[0])]


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("geom", list(VIT_GEOMETRIES))
def test_vit_attention_core_every_length_against_float64(dev, geom, dt):
    """All 16 reachable lengths S = np^2 + 1 (img = 14 np): S = 257 takes the compile-time-length kernel, every other one the run-time
    masks.  One frame per case family, heads x families workgroups per launch."""
    dim, heads = VIT_GEOMETRIES[geom]
    hd = dim // heads
    dtype, op = DT[dt]
    t0 = time.time()
    worst, failures = (0.0, None), []
    for np_ in range(1, 17):
        S = np_ * np_ + 1
        kinds = AC.families_for(S)
        h = _vit(dim, heads, 14 * np_, op)
        try:
            q, k, v = _units(kinds, heads, S, hd, dtype)
            out = _run_vit_core(h, q, k, v)
        finally:
            h.close()
        ref, bound, _ = AC.attention_ref(q, k, v)
        for kind, r in zip(kinds, _ratios_per_item(out, ref, bound)):
            worst = max(worst, (r, (kind, S)))
            if not r <= 1.0:
                failures.append((kind, S, round(r, 3)))
    print(f"vit_attn_kernel {dt} {geom} (hd {hd}): worst |d| / bound {worst[0]:.3f} at {worst[1]}  [{time.time() - t0:.1f} s]")
    assert not failures, failures


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_vit_persistent_core_is_bit_identical_and_within_the_bound(dev, dt):
    """S = 257 with ``attn_persist`` 1: fewer units than CUs (every workgroup runs one unit and prefetches itself), more units than CUs with
    a unit count that is not a multiple of the grid (some workgroups run two units, some one), and an exact multiple of the grid."""
    dim, heads = VIT_GEOMETRIES["16 heads"]
    hd, S = dim // heads, 257
    dtype, op = DT[dt]
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    frame_counts = (3, cus // heads + 1, 2 * (cus // heads))
    assert 3 * heads < cus < frame_counts[1] * heads and (frame_counts[1] * heads) % cus != 0
    fams = AC.families_for(S)
    h = _vit(dim, heads, 224, op)
    worst = 0.0
    try:
        for n in frame_counts:
            kinds = [fams[i % len(fams)] for i in range(n)]
            q, k, v = _units(kinds, heads, S, hd, dtype)
            plain = _run_vit_core(h, q, k, v)
            L.check(L.lib().mra_vit_set_option(h.h, b"attn_persist", 1), "attn_persist")
            try:
                persist = _run_vit_core(h, q, k, v)
            finally:
                L.check(L.lib().mra_vit_set_option(h.h, b"attn_persist", 0), "attn_persist")
            assert torch.equal(_bits(persist), _bits(plain)), f"{n} frames ({n * heads} units on {cus} CUs): persistent != stand-alone"
            ref, bound, _ = AC.attention_ref(q, k, v)
            rs = _ratios_per_item(persist, ref, bound)
            worst = max(worst, max(rs))
            assert max(rs) <= 1.0, (n, [(kd, round(r, 3)) for kd, r in zip(kinds, rs) if not r <= 1.0])
    finally:
        h.close()
    print(f"vit_attn_persist_kernel {dt}: units {[n * heads for n in frame_counts]} on {cus} CUs, worst |d| / bound {worst:.3f}")


# ---- BEATs -------------------------------------------------------------------------------------------------------------------------
def _load_beats_core(h, pr, dev):
    h.load("encoder.layers.0.self_attn.relative_attention_bias.weight", pr["E"].to(dev))
    h.load("encoder.layers.0.self_attn.grep_linear.weight", pr["gw"].to(dev))
    h.load("encoder.layers.0.self_attn.grep_linear.bias", pr["gb"].to(dev))
    h.load("encoder.layers.0.self_attn.grep_a", pr["ga"].view(1, -1, 1, 1).to(dev))


def _run_beats_core(h, q, k, v, layer_in):
    """layer_in [n, heads, P, 64] or None (GATE_Q): the gate source in the kernel's [n * P, dim] layout."""
    n, heads, P, hd = q.shape
    qkv = _guarded(AC.pack_beats_qkv(q, k, v))
    gsrc = _guarded(layer_in.transpose(1, 2).reshape(n * P, heads * hd)) if layer_in is not None else None
    ctx = torch.full((n * P + 2 * GUARD, heads * hd), float("nan"), dtype=torch.float16, device=qkv.device)
    qkv0, ctx0 = qkv.clone(), ctx.clone()
    L.check(L.lib().mra_debug_beats_attention(h.h, 0, L.ptr(qkv[GUARD:]), L.ptr(gsrc[GUARD:]) if gsrc is not None else None, n, P,
                                              L.ptr(ctx[GUARD:]), _stream()), "mra_debug_beats_attention")
    torch.cuda.synchronize()
    assert torch.equal(_bits(qkv), _bits(qkv0)), "the input was written"
    _check_output_region(ctx, ctx0, n * P, "beats ctx")
    return AC.unpack_ctx(ctx[GUARD:GUARD + n * P].cpu(), n, heads)


def test_beats_small_geometry_is_not_a_valid_handle(dev):
    """dim 256 / 4 heads cannot exist: the positional convolution is built on 48 channels per group and dim must be a multiple of 256 and
    at most 1024, which leaves 768 / 12 as the only geometry ``mra_beats_create`` accepts -- so the core tests below run on it alone."""
    h = C.c_void_p()
    for dim, heads in ((256, 4), (512, 8), (1024, 16)):
        cfg = _beats_cfg(L.MRA_BEATS_GATE_Q, dim, heads)
        assert L.lib().mra_beats_create(C.byref(cfg), C.byref(h)) == -1 and not h


@pytest.mark.parametrize("gate", ["gate_q", "gate_input"])
def test_beats_attention_core_against_float64(dev, gate):
    """13 token counts: below one 16-key fragment, around the 128-key chunks of the online softmax, 256 / 264 (the switch between the
    256- and 512-key LDS instantiations), the maximum 512.  Per count: the families with the N(0, 0.5) bias table, then ``mild`` and ``constant``
    q.k under a table scaled until the bias alone peaks the rows."""
    heads, hd = 12, 64
    gate_input = gate == "gate_input"
    h = _Handle("mra_beats", _beats_cfg(L.MRA_BEATS_GATE_INPUT if gate_input else L.MRA_BEATS_GATE_Q))
    tables = {"table": AC.beats_core_params(heads), "peaked bias": AC.beats_core_params(heads, bias_scale=AC.PEAKED_BIAS_SCALE)}
    t0 = time.time()
    worst, failures = (0.0, None), []
    try:
        for P in BEATS_TOKENS:
            for tname, pr in tables.items():
                kinds = AC.families_for(P, AC.BEATS_FAMILIES) if tname == "table" else ["mild", "constant"]   # constant: the bias alone shapes the rows
                _load_beats_core(h, pr, dev)
                q, k, v = _units(kinds, heads, P, hd, torch.float16)
                layer_in = torch.randn(len(kinds), heads, P, hd, generator=torch.Generator().manual_seed(900 + P)).half() if gate_input else None
                out = _run_beats_core(h, q, k, v, layer_in)
                ref, bound, _ = AC.beats_attention_ref(q, k, v, layer_in if gate_input else q, pr["E"], pr["gw"], pr["gb"], pr["ga"])
                for kind, r in zip(kinds, _ratios_per_item(out, ref, bound)):
                    worst = max(worst, (r, (kind, tname, P)))
                    if not r <= 1.0:
                        failures.append((kind, tname, P, round(r, 3)))
    finally:
        h.close()
    print(f"beats_attn_kernel f16 {gate}: worst |d| / bound {worst[0]:.3f} at {worst[1]}  [{time.time() - t0:.1f} s]")
    assert not failures, failures


def test_beats_posconv_against_float64(dev):
    """Token counts below the 64-row padding of the 128-tap window (mostly padding), at and around it, at whole and ragged 64-token wave
    blocks, and the maximum; one chunk and three."""
    h = _Handle("mra_beats", _beats_cfg(L.MRA_BEATS_GATE_Q))
    worst, failures = (0.0, None), []
    try:
        _, w, b = AC.make_posconv(1, 8)
        h.load("encoder.pos_conv.0.weight", w.to(dev))
        h.load("encoder.pos_conv.0.bias", b.to(dev))
        for P in POSCONV_TOKENS:
            for n in (1, 3):
                x, _, _ = AC.make_posconv(n, P)
                buf = _guarded(x.view(n * P, -1))
                before = buf.clone()
                L.check(L.lib().mra_debug_beats_posconv(h.h, L.ptr(buf[GUARD:]), n, P, _stream()), "mra_debug_beats_posconv")
                torch.cuda.synchronize()
                _check_output_region(buf, before, n * P, "posconv x")
                ref, bound = AC.posconv_ref(x, w, b)
                r = AC.worst_ratio(buf[GUARD:GUARD + n * P].cpu().view(n, P, -1), ref, bound)
                worst = max(worst, (r, (P, n)))
                if not r <= 1.0:
                    failures.append((P, n, round(r, 3)))
    finally:
        h.close()
    print(f"beats_posconv_kernel: worst |d| / bound {worst[0]:.2e} at (P, n) = {worst[1]}")
    assert not failures, failures


def test_stage_entry_points_check_their_arguments(dev):
    lib = L.lib()
    EINVAL, ESTATE = -1, -2
    buf = torch.zeros(1 << 20, dtype=torch.float16, device=dev)
    p, p2, st = L.ptr(buf), L.ptr(buf[1 << 19:]), _stream()       # inputs at p, outputs at p2
    v = _vit(1408, 16, 28, L.MRA_F16)              # no parameter loaded: the core needs none
    try:
        assert lib.mra_debug_vit_attention(None, p, 1, p, st) == EINVAL
        assert lib.mra_debug_vit_attention(v.h, p, -1, p, st) == EINVAL
        assert lib.mra_debug_vit_attention(v.h, None, 1, p, st) == EINVAL and lib.mra_debug_vit_attention(v.h, p, 1, None, st) == EINVAL
        assert lib.mra_debug_vit_attention(v.h, None, 0, None, st) == 0
    finally:
        v.close()
    for gate in (L.MRA_BEATS_GATE_Q, L.MRA_BEATS_GATE_INPUT):
        b = _Handle("mra_beats", _beats_cfg(gate))
        try:
            att = lambda layer, q, g, n, tok, c: lib.mra_debug_beats_attention(b.h, layer, q, g, n, tok, c, st)
            assert lib.mra_debug_beats_attention(None, 0, p, p, 1, 8, p, st) == EINVAL
            assert att(0, p, p, -1, 8, p) == EINVAL
            assert att(-1, p, p, 1, 8, p) == EINVAL and att(1, p, p, 1, 8, p) == EINVAL          # one layer
            assert att(0, p, p, 1, 0, p) == EINVAL and att(0, p, p, 1, 513, p) == EINVAL and att(0, p, p, 1, -8, p) == EINVAL
            assert att(0, None, p, 1, 8, p) == EINVAL and att(0, p, p, 1, 8, None) == EINVAL
            assert att(0, None, None, 0, 8, None) == 0
            assert att(0, p, p, 1, 8, p) == ESTATE                                               # nothing loaded
            assert b"not loaded" in lib.mra_last_error()
            pos = lambda x, n, tok: lib.mra_debug_beats_posconv(b.h, x, n, tok, st)
            assert lib.mra_debug_beats_posconv(None, p, 1, 8, st) == EINVAL
            assert pos(p, -1, 8) == EINVAL and pos(p, 1, 0) == EINVAL and pos(p, 1, 513) == EINVAL and pos(None, 1, 8) == EINVAL
            assert pos(None, 0, 8) == 0
            assert pos(p, 1, 8) == ESTATE
            pr = AC.beats_core_params(12)
            _load_beats_core(b, pr, dev)
            if gate == L.MRA_BEATS_GATE_INPUT:
                assert att(0, p, None, 1, 8, p) == EINVAL                                        # the gate source is read in this mode
            else:
                assert att(0, p, None, 1, 8, p2) == 0                                             # ... and ignored in this one
            assert att(0, p, p, 1, 8, p2) == 0 and pos(p, 1, 8) == ESTATE                         # the convolution's parameters are still missing
            torch.cuda.synchronize()
        finally:
            b.close()


# ---- whole encoders at the edges of their geometry ----------------------------------------------------------------------------------
@pytest.mark.parametrize("img", [14, 28, 56, 168, 210])
def test_vit_whole_encoder_at_other_lengths(dev, img):
    """Depth 1 at S = 2, 5, 17, 145 and 226 against the float64 restatement, at the bars of tests/test_gpu_vit.py."""
    from mraudio_amd.models.eva_vit import EvaViTg, HipEvaViTg

    ref = EvaViTg(img_size=img, depth=1).eval().init_seeded_(50 + img)
    hip = HipEvaViTg(img_size=img, depth=1, device=dev).eval()
    hip.load_state_dict(ref.state_dict())
    x = torch.randn(3, 3, img, img, generator=torch.Generator().manual_seed(img))
    with torch.no_grad():
        want = ref.double()(x.double())
    got = hip(x.to(dev)).cpu().double()
    assert got.shape == want.shape == (3, (img // 14) ** 2 + 1, 1408) and torch.isfinite(got).all()
    d, rel = (got - want).abs().max().item(), ((got - want).norm() / want.norm()).item()
    print(f"vit depth 1, img {img} (S = {want.shape[1]}): max|d| {d:.3e}, rel {rel:.3e}")
    assert d < 2e-2 and rel < 2e-3, (img, d, rel)


@pytest.fixture(scope="module")
def beats12(dev):
    from mraudio_amd.models.beats import BEATs, HipBEATs

    ref = BEATs().eval().init_seeded_(33)
    hip = HipBEATs(ref.cfg, device=dev).eval()
    hip.load_state_dict(ref.state_dict())
    return ref.double(), hip


@pytest.mark.parametrize("frames", [16, 48, 1024])
def test_beats_whole_encoder_at_the_ends_of_its_range(beats12, dev, frames):
    """12 layers at P = 8, 24 and 512 (the maximum) against the restatement in float64, at the bars of tests/test_gpu_beats.py; one
    patch row more than the maximum (1040 frames = 520 tokens) is refused."""
    from mraudio_amd import MraError
    from tools.make_beats_golden import make_fbank

    ref, hip = beats12
    fb = make_fbank(frames, n=2, seed=60 + frames)
    with torch.no_grad():
        want = ref(fb.double())
    y = hip(fb.to(dev)).cpu().double()
    assert y.shape == want.shape == (2, frames // 16 * 8, 768)
    d, rel = (y - want).abs().max().item(), ((y - want).norm() / want.norm()).item()
    print(f"beats 12 layers, {frames} frames (P = {want.shape[1]}): max|d| {d:.3e}, rel {rel:.3e}")
    assert torch.isfinite(y).all() and d <= 3e-2 and rel <= 3e-3, (d, rel)
    if frames == 1024:
        with pytest.raises(MraError):
            hip(make_fbank(1040, n=1).to(dev))        # 520 tokens: above the 512 the attention core holds
