"""The video front end without a GPU: the float64 definition of the crop / resize / flip / ToUint8 / normalise transform
(``mraudio_amd/processors/alpro_processors.py``) against torch's own bicubic ``interpolate``; the derived bound and the fp32 emulation of
``csrc/video_pre.hip`` inside it; mutants of the definition outside it; ``mra_video_crop_table`` against the Python table bit for bit;
the crop-box draw; the host processors; and the host side of the device route with a fake device."""
import ctypes as C
import json
import random

import numpy as np
import pytest
import torch

import video_pre_cases as V
from mraudio_amd import _lib
from mraudio_amd.processors import alpro_processors as P
from mraudio_amd.processors.alpro_processors import (AlproVideoEvalProcessor_Stamps, AlproVideoTrainProcessor_Stamps, crop_resize_table,
                                                     preprocess_frames_ref, random_flip, random_resized_crop_params)

H0, W0 = 40, 52                        # a non-square source; 52 * 3 = 156-byte rows
FRAMES = V.noise_frames(2, H0, W0, seed=5)


# ---- the definition --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [16, 56])                                   # a downscale and an upscale of most boxes
@pytest.mark.parametrize("flip", [False, True])
def test_definition_matches_torch_bicubic_in_float64(size, flip):
    for name, box in V.boxes(H0, W0, size):
        want = V.torch_reference(FRAMES, box, flip, size, V.MEAN_T, V.STD_T)
        got = preprocess_frames_ref(FRAMES, box, flip, size, V.MEAN_T, V.STD_T, quantize="none")
        assert got.dtype == torch.float64 and got.shape == (2, 3, size, size)
        d = (got - want).abs().max().item()
        print(f"size {size}, flip {flip}, {name} {box}: max |definition - torch| {d:.3e}")
        assert d <= 1e-9, (name, box, d)
        assert torch.equal(got, V.variant(FRAMES, box, flip, size, V.MEAN_T, V.STD_T, quantize="none"))     # the helper restates it exactly
        assert torch.equal(preprocess_frames_ref(FRAMES, box, flip, size, quantize="floor"), V.variant(FRAMES, box, flip, size))


def test_identity_is_exact_in_both_quantize_modes():
    sq = V.noise_frames(3, 24, 24, seed=6)
    idx, w = crop_resize_table(24, 0, 24)
    assert np.array_equal(idx[:, 1], np.arange(24)) and np.array_equal(w, np.tile(np.array([0.0, 1.0, 0.0, 0.0]), (24, 1)))
    a = preprocess_frames_ref(sq, None, False, 24, quantize="none")
    b = preprocess_frames_ref(sq, (0, 0, 24, 24), False, 24, quantize="floor")
    m, s = torch.tensor(P.MEAN, dtype=torch.float64).view(1, 3, 1, 1), torch.tensor(P.STD, dtype=torch.float64).view(1, 3, 1, 1)
    assert torch.equal(a, b) and torch.equal(a, (sq.permute(0, 3, 1, 2).to(torch.float64) / 255.0 - m) / s)


def test_table_indices_stay_inside_the_crop_and_bad_arguments_are_refused():
    idx, w = crop_resize_table(7, 11, 32)
    assert idx.shape == (32, 4) and w.shape == (32, 4) and w.dtype == np.float64
    assert idx.min() == 11 and idx.max() == 17 and np.allclose(w.sum(1), 1.0, atol=1e-15)
    for bad in [(0, 0, 8), (4, -1, 8), (4, 0, 0)]:
        with pytest.raises(ValueError):
            crop_resize_table(*bad)
    with pytest.raises(ValueError, match="inside"):
        preprocess_frames_ref(FRAMES, (0, 0, H0 + 1, W0), False, 16)
    with pytest.raises(ValueError, match="quantize"):
        preprocess_frames_ref(FRAMES, None, False, 16, quantize="round")


# ---- the bound and the emulation ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [16, 56])
def test_fp32_emulation_sits_inside_the_derived_bound(size):
    worst = 0.0
    for flip in (False, True):
        for name, box in V.boxes(H0, W0, size):
            want = V.variant(FRAMES, box, flip, size, V.MEAN_T, V.STD_T, quantize="none")
            bound = V.total_bound(FRAMES, box, flip, size, V.MEAN_T, V.STD_T)
            d = (V.emulate(FRAMES, box, flip, size, V.MEAN_T, V.STD_T, quantize="none").to(torch.float64) - want).abs()
            worst = max(worst, (d / bound).max().item())
            assert (d <= bound).all(), (name, box, flip, (d / bound).max().item())
            V.check_floor(V.emulate(FRAMES, box, flip, size, V.MEAN_T, V.STD_T, quantize="floor"), FRAMES, box, flip, size, V.MEAN_T, V.STD_T)
    print(f"size {size}: worst |emulation - float64| / bound {worst:.3f}")
    assert worst > 0.01        # the bound is of the emulation's own order, not a blanket


def test_floor_is_rarely_ambiguous_on_noise_and_exact_at_the_ends():
    box = (3, 4, 33, 43)
    levels = V.allowed_levels(FRAMES, box, False, 32)
    many = ((levels[0] != levels[1]) | (levels[1] != levels[2])).double().mean().item()
    print(f"noise, {box} -> 32: {100 * many:.3f} % of outputs have more than one allowed level")
    assert many <= 0.01
    # values 0 and 255: bytes that are all 0 or 255 overshoot the most, the clamp brings those outputs back to the levels 0 and 255,
    # and every output with ONE allowed level is the fp32 normalisation of it, bit for bit
    binary = V.binary_frames(2, 20, 27, seed=3)
    for box in [(0, 0, 20, 27), (4, 6, 5, 7)]:
        single, want = V.exact_levels(binary, box, True, 32, V.MEAN_T, V.STD_T)
        got = V.emulate(binary, box, True, 32, V.MEAN_T, V.STD_T, quantize="floor")
        h = V.variant(binary, box, True, 32, quantize="none", want_h=True)
        clamped = single & ((h < 0) | (h > 255))
        print(f"bytes 0 / 255, {box}: {100 * single.double().mean().item():.1f} % one level, {100 * clamped.double().mean().item():.1f} % on the clamp")
        assert clamped.double().mean().item() > 0.2 and torch.equal(got[single], want[single])
    black = torch.zeros(1, 20, 27, 3, dtype=torch.uint8)
    single, want = V.exact_levels(black, (3, 4, 13, 18), False, 16)
    assert single.all() and torch.equal(V.emulate(black, (3, 4, 13, 18), False, 16, quantize="floor"), want)
    # a constant 255 is NOT such a case: the fp32 sums land on either side of 255 and floor takes the lower ones to 254; both levels are
    # allowed (the plateau rule of the GPU test, without the cap)
    white = torch.full((1, 20, 27, 3), 255, dtype=torch.uint8)
    ambiguous, _ = V.check_floor(V.emulate(white, (3, 4, 13, 18), False, 32, quantize="floor"), white, (3, 4, 13, 18), False, 32)
    assert ambiguous > 0


# ---- mutants: each sits outside the bound on a stated case -----------------------------------------------------------------
MUTANTS = [
    ("tap clamp at the source edge, not the crop edge", (5, 6, 12, 20), False, 24, {"clamp_to": "source"}),
    ("A = -0.5", (3, 4, 30, 41), False, 24, {"A": -0.5}),
    ("align_corners geometry", (3, 4, 30, 41), False, 24, {"geometry": "align_corners"}),
    ("no half-pixel offset", (3, 4, 30, 41), False, 24, {"geometry": "no_half_pixel"}),
    ("flip before the crop offset", (2, 0, 30, 25), True, 24, {"flip_first": True}),
    ("swapped channel order", (3, 4, 30, 41), False, 24, {"channels": (2, 1, 0)}),
]


@pytest.mark.parametrize("name,box,flip,size,kw", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_mutant_of_the_interpolation_is_outside_the_bound(name, box, flip, size, kw):
    want = V.variant(FRAMES, box, flip, size, V.MEAN_T, V.STD_T, quantize="none")
    bound = V.total_bound(FRAMES, box, flip, size, V.MEAN_T, V.STD_T, f16=True)        # the widest bound any GPU test uses
    d = (V.variant(FRAMES, box, flip, size, V.MEAN_T, V.STD_T, quantize="none", **kw) - want).abs()
    outside = (d > bound).double().mean().item()
    print(f"{name}: {100 * outside:.1f} % of outputs outside the bound, worst {((d / bound).max().item()):.1f} x")
    assert outside > 0.05
    assert ((V.emulate(FRAMES, box, flip, size, V.MEAN_T, V.STD_T, quantize="none").to(torch.float64) - want).abs() <= bound).all()


@pytest.mark.parametrize("mode", ["round", "floor_unclamped"])
def test_mutant_of_the_quantisation_is_outside_the_bound(mode):
    box, size = (4, 6, 9, 11), 32            # an upscale of noise: overshoot below 0 and above 255
    h = V.variant(FRAMES, box, False, size, quantize="none", want_h=True)
    assert h.min().item() < -1.0 and h.max().item() > 256.0
    got = V.variant(FRAMES, box, False, size, V.MEAN_T, V.STD_T, quantize=mode)
    with pytest.raises(AssertionError, match="match no allowed level"):
        V.check_floor(got, FRAMES, box, False, size, V.MEAN_T, V.STD_T, f16=True)


# ---- the C helper ------------------------------------------------------------------------------------------------------
def _c_table(n_src_crop, offset, n_out):
    idx, w = np.zeros((n_out, 4), dtype=np.int16), np.zeros((n_out, 4), dtype=np.float32)
    rc = _lib.lib().mra_video_crop_table(n_src_crop, offset, n_out, idx.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p))
    return rc, idx, w


def test_c_crop_table_equals_the_python_table_bit_for_bit():
    for n_src_crop, offset, n_out in [(224, 0, 224), (201, 13, 224), (7, 11, 32), (1, 5, 16), (40, 0, 16), (33, 1, 32), (1080, 400, 224),
                                      (3, 32764, 8)]:
        rc, idx, w = _c_table(n_src_crop, offset, n_out)
        pi, pw = crop_resize_table(n_src_crop, offset, n_out)
        assert rc == 0
        assert np.array_equal(idx.astype(np.int64), pi), (n_src_crop, offset, n_out)
        assert np.array_equal(w.view(np.uint32), pw.astype(np.float32).view(np.uint32)), (n_src_crop, offset, n_out)


def test_c_entries_refuse_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    for bad in [(0, 0, 8), (4, -1, 8), (4, 0, 0), (-3, 0, 8)]:
        assert _c_table(*bad)[0] == -1 and b"> 0" in lib.mra_last_error()
    assert _c_table(4, 32765, 8)[0] == -1 and b"32767" in lib.mra_last_error()
    assert lib.mra_video_crop_table(4, 0, 8, None, None) == -1 and b"null" in lib.mra_last_error()
    mean, std = (C.c_float * 3)(*P.MEAN), (C.c_float * 3)(*P.STD)
    fwd = lambda *a: lib.mra_video_frames_forward(*a, None)
    one = C.c_void_p(16)           # never dereferenced: every refusal comes before a launch
    assert fwd(None, 0, None, 0, None, None, 0, 224, mean, std, 1, None, _lib.MRA_F16) == 0                    # n_out == 0: a no-op
    assert fwd(one, 8, one, 1, one, one, 1, 224, mean, std, 1, None, _lib.MRA_F16) == -1 and b"null" in lib.mra_last_error()
    assert fwd(None, 0, None, 0, None, None, 0, 20, mean, std, 1, None, _lib.MRA_F16) == -1 and b"multiple of 8" in lib.mra_last_error()
    assert fwd(None, 0, None, 0, None, None, 0, 776, mean, std, 1, None, _lib.MRA_F16) == -1 and b"768" in lib.mra_last_error()
    assert fwd(None, 0, None, 0, None, None, 0, 224, mean, std, 1, None, _lib.MRA_BF16) == -1 and b"out_dtype" in lib.mra_last_error()
    assert fwd(None, 0, None, 0, None, None, 0, 224, mean, std, 2, None, _lib.MRA_F16) == -1 and b"quantize" in lib.mra_last_error()
    assert fwd(None, 0, None, 0, None, None, 0, 224, mean, (C.c_float * 3)(0.2, 0.0, 0.2), 1, None, _lib.MRA_F16) == -1 and b"std" in lib.mra_last_error()
    assert fwd(None, 0, None, 0, None, None, 0, 224, None, std, 1, None, _lib.MRA_F16) == -1
    assert fwd(None, 0, None, -1, None, None, 0, 224, mean, std, 1, None, _lib.MRA_F16) == -1
    assert fwd(one, 8, one, 1, one, one, 1, 224, mean, std, 1, C.c_void_p(24), _lib.MRA_F16) == -1 and b"aligned" in lib.mra_last_error()
    assert lib.mra_debug_video_frames_forward(None, 0, None, 0, None, None, 0, 224, mean, std, 1, None, _lib.MRA_F16, 2, None) == -1
    assert lib.mra_video_frames_bytes(1024, 224, 224, 224, _lib.MRA_F16) == 1024 * (3 * 224 * 224 + 3 * 2 * 224 * 224)
    assert lib.mra_video_frames_bytes(2, 20, 27, 16, _lib.MRA_F32) == 2 * (3 * 20 * 27 + 3 * 4 * 16 * 16)
    assert lib.mra_video_frames_bytes(0, 20, 27, 16, _lib.MRA_F32) == 0.0


# ---- the crop-box draw -------------------------------------------------------------------------------------------------
def test_crop_box_draw_stays_inside_its_ranges_and_is_reproducible():
    H, W, scale, ratio = 40, 52, (0.3, 0.6), (3.0 / 4.0, 4.0 / 3.0)
    rng = random.Random(3)
    seen = set()
    for _ in range(300):
        top, left, h, w = random_resized_crop_params(H, W, scale, ratio, rng)
        seen.add((top, left, h, w))
        assert 0 <= top and top + h <= H and 0 <= left and left + w <= W and h > 0 and w > 0
        # an accepted try (here every draw: the fallback below is the whole 40 x 52 frame, area share 1): w, h are roundings of
        # sqrt(area * ratio), sqrt(area / ratio), so w / h and w h are inside the ranges up to half a pixel on each side
        assert (top, left, h, w) != (0, 0, H, W)
        assert (w - 0.5) / (h + 0.5) <= ratio[1] and (w + 0.5) / (h - 0.5) >= ratio[0]
        assert (w - 0.5) * (h - 0.5) <= scale[1] * H * W and (w + 0.5) * (h + 0.5) >= scale[0] * H * W
    assert len(seen) > 250
    again = random.Random(3)
    assert [random_resized_crop_params(H, W, scale, ratio, again) for _ in range(5)] == \
        [random_resized_crop_params(H, W, scale, ratio, r) for r in [random.Random(3)] for _ in range(5)]
    # no try fits (an area share above 1): the ratio-clamped central crop; the draws are still consumed from the rng
    assert random_resized_crop_params(40, 52, (1.5, 2.0), ratio, random.Random(1)) == (0, 0, 40, 52)
    assert random_resized_crop_params(20, 80, (1.5, 2.0), ratio, random.Random(1)) == (0, 26, 20, 27)      # too wide: h = H, w = round(H * 4 / 3)
    assert random_resized_crop_params(80, 20, (1.5, 2.0), ratio, random.Random(1)) == (26, 0, 27, 20)      # too tall: w = W, h = round(W / (3 / 4))
    flips = [random_flip(random.Random(9)) for _ in range(3)]
    assert flips[0] == flips[1] == flips[2] and isinstance(flips[0], bool)
    rng = random.Random(4)
    share = sum(random_flip(rng) for _ in range(2000)) / 2000.0
    assert abs(share - 0.5) < 0.05


# ---- the host processors -------------------------------------------------------------------------------------------------
def _reader(frames, fps=3.0):
    return lambda vpath, h, w: (frames.numpy(), fps)


def _todays_output(frames, indices, n_frms, mean=None, std=None):
    """An inline copy of the processor as it was: float32, normalise, permute, pad."""
    clip = torch.as_tensor(frames.numpy()[np.asarray(indices)]).permute(3, 0, 1, 2).float()
    m = torch.tensor(mean if mean is not None else (0.48145466, 0.4578275, 0.40821073)).view(3, 1, 1, 1)
    s = torch.tensor(std if std is not None else (0.26862954, 0.26130258, 0.27577711)).view(3, 1, 1, 1)
    out = (clip / 255.0 - m) / s
    pad = n_frms - out.shape[1]
    return torch.cat([out, out[:, -1:].repeat(1, pad, 1, 1)], dim=1) if pad > 0 else out


def test_default_processors_are_unchanged_bit_for_bit():
    video = V.noise_frames(9, 24, 24, seed=8)
    ev = AlproVideoEvalProcessor_Stamps(image_size=24, n_frms=4, reader=_reader(video))
    clip, idx, fps = ev("v")
    assert torch.equal(clip, _todays_output(video, idx, 4)) and clip.dtype == torch.float32 and clip.shape == (3, 4, 24, 24) and fps == 3.0
    short = AlproVideoEvalProcessor_Stamps(image_size=24, n_frms=12, reader=_reader(video), mean=V.MEAN_T, std=V.STD_T)
    clip, idx, _ = short("v")
    assert len(idx) == 9 and torch.equal(clip, _todays_output(video, idx, 12, V.MEAN_T, V.STD_T)) and clip.shape == (3, 12, 24, 24)
    random.seed(11)
    tr = AlproVideoTrainProcessor_Stamps(image_size=24, n_frms=4, reader=_reader(video), min_scale=0.2, max_scale=0.3)
    clip, idx, _ = tr("v")
    assert tr.augment is False and torch.equal(clip, _todays_output(video, idx, 4))
    random.seed(11)
    assert list(idx) == list(P.frame_indices(9, 4, "random"))           # the same draws from the global generator as before


def test_augmenting_train_processor_applies_the_definition():
    video = V.noise_frames(9, 30, 41, seed=9)
    tr = AlproVideoTrainProcessor_Stamps(image_size=24, n_frms=6, reader=_reader(video), min_scale=0.4, max_scale=0.7, augment=True,
                                         rng=random.Random(21), mean=V.MEAN_T, std=V.STD_T)
    clip, idx, _ = tr("v")
    rng = random.Random(21)
    want_idx = P.frame_indices(9, 6, "random", rng)
    box = random_resized_crop_params(30, 41, (0.4, 0.7), rng=rng)
    flip = random_flip(rng)
    assert list(idx) == list(want_idx) and box != (0, 0, 30, 41)          # min_scale / max_scale do something
    want = preprocess_frames_ref(video[np.asarray(want_idx)], box, flip, 24, V.MEAN_T, V.STD_T, "floor")
    assert clip.dtype == torch.float32 and clip.shape == (3, 6, 24, 24)
    assert torch.equal(clip, want.permute(1, 0, 2, 3).to(torch.float32))
    levels = clip.permute(1, 0, 2, 3).double() * torch.tensor(V.STD_T).view(1, 3, 1, 1) + torch.tensor(V.MEAN_T).view(1, 3, 1, 1)
    assert ((levels * 255.0) - (levels * 255.0).round()).abs().max().item() < 1e-3         # "floor": whole uint8 levels
    # quantize="none" keeps the fractional values; a clip shorter than n_frms is padded with its last frame
    tr = AlproVideoTrainProcessor_Stamps(image_size=24, n_frms=12, reader=_reader(video), augment=True, rng=random.Random(22), quantize="none")
    clip, idx, _ = tr("v")
    assert len(idx) == 9 and clip.shape == (3, 12, 24, 24) and torch.equal(clip[:, 9:], clip[:, 8:9].expand(-1, 3, -1, -1))
    with pytest.raises(ValueError, match="quantize"):
        AlproVideoTrainProcessor_Stamps(augment=True, quantize="round")


# ---- the host side of the device route, with a fake device ------------------------------------------------------------------
def test_raw_pads_in_uint8_and_carries_the_augmentation():
    video = V.noise_frames(5, 30, 41, seed=10)
    ev = AlproVideoEvalProcessor_Stamps(image_size=24, n_frms=8, reader=_reader(video), device="cuda:0")
    frames, box, flip, idx, fps = ev.raw("v")
    assert frames.dtype == torch.uint8 and frames.shape == (8, 30, 41, 3) and not frames.is_cuda and frames.is_contiguous()
    assert torch.equal(frames[:5], video[np.asarray(idx)]) and torch.equal(frames[5:], video[-1:].expand(3, -1, -1, -1))
    assert box.dtype == torch.int64 and box.tolist() == [0, 0, 30, 41] and flip == 0 and fps == 3.0
    random.seed(5)
    tr = AlproVideoTrainProcessor_Stamps(image_size=24, n_frms=4, reader=_reader(video), device="cuda:0")
    _, box, flip, _, _ = tr.raw("v")
    assert box.tolist() == [0, 0, 30, 41] and flip == 0 and tr.quantize == "none"
    tr = AlproVideoTrainProcessor_Stamps(image_size=24, n_frms=4, reader=_reader(video), device="cuda:0", augment=True, rng=random.Random(2),
                                         min_scale=0.3, max_scale=0.5)
    _, box, flip, idx, _ = tr.raw("v")
    rng = random.Random(2)
    assert list(idx) == list(P.frame_indices(5, 4, "random", rng))
    assert tuple(box.tolist()) == random_resized_crop_params(30, 41, (0.3, 0.5), rng=rng) and flip == int(random_flip(rng)) and tr.quantize == "floor"
    with pytest.raises(ValueError, match="uint8"):
        AlproVideoEvalProcessor_Stamps(image_size=24, n_frms=4, reader=lambda p, h, w: (video.numpy().astype(np.float32), 3.0), device="cuda:0").raw("v")
    with pytest.raises(ValueError, match="CUDA"):
        AlproVideoEvalProcessor_Stamps(device="cpu")
    with pytest.raises(ValueError, match="multiple of 8"):
        AlproVideoEvalProcessor_Stamps(image_size=20, device="cuda:0")
    with pytest.raises(RuntimeError, match="CUDA device"):
        AlproVideoEvalProcessor_Stamps(image_size=24).flat([video])


def test_encode_takes_video_raw_through_the_processor_and_refuses_without_one():
    from mraudio_amd._lib import MraError
    from mraudio_amd.models.xinstructblip import XInstructBLIP as X

    calls = []

    class FakeProc:
        device, n_frms = torch.device("cuda:0"), 4

        def flat(self, clips, boxes, flips, lo, hi, out_dtype):
            calls.append((len(clips), boxes, flips, lo, hi, out_dtype))
            n = (len(clips) * self.n_frms if hi is None else hi) - (0 if lo is None else lo)
            return torch.arange(n, dtype=torch.float32).view(n, 1, 1, 1).expand(n, 3, 2, 2).to(out_dtype)

    enc = lambda x: x.float().mean(dim=(1, 2, 3)).view(-1, 1, 1)
    stub = lambda proc: type("S", (), {"_device": torch.device("cpu"), "encode_chunk": 3, "video_encoder": staticmethod(enc), "audio_encoder": None,
                                       "video_processor": proc, "audio_processor": None})()
    raw = torch.zeros(2, 4, 5, 6, 3, dtype=torch.uint8)
    box, flip = torch.tensor([[0, 0, 5, 6], [1, 1, 3, 3]]), torch.tensor([0, 1])
    out, _, bs, num = X._encode(stub(FakeProc()), {"video_raw": raw, "video_box": box, "video_flip": flip}, "video", 1, 7)
    assert (bs, num) == (2, 4) and out.shape == (6, 1, 1) and torch.equal(out.view(-1), torch.arange(6.0))      # chunks of 3, in order
    assert calls[-1][0] == 2 and calls[-1][1] is box and calls[-1][2] is flip and calls[-1][3:] == (1, 7, torch.float16)
    out, _, bs, num = X._encode(stub(FakeProc()), {"video_raw": [raw[0], raw[1], raw[0]]}, "video")
    assert (bs, num) == (3, 4) and out.shape == (12, 1, 1) and calls[-1][1] is None and calls[-1][2] is None
    assert X._present(stub(None), {"video_raw": raw}, "video") and not X._present(stub(None), {"video_raw": raw}, "audio")
    for proc in (None, AlproVideoEvalProcessor_Stamps(image_size=24, n_frms=4)):                                  # none, or a host processor
        with pytest.raises(MraError, match="video_processor"):
            X._encode(stub(proc), {"video_raw": raw}, "video")


def test_dataset_emits_raw_keys_for_a_device_processor(tmp_path):
    from mraudio_amd.utils.mr_dataset import MRDataset, collate_fn

    video = V.noise_frames(6, 24, 24, seed=12)
    ann = tmp_path / "ann.jsonl"
    ann.write_text("".join(json.dumps({"qid": i, "query": f"q{i}", "vid": f"v{i}", "duration": 10, "relevant_windows": [[0, 2]]}) + "\n" for i in range(2)))
    dev = AlproVideoTrainProcessor_Stamps(image_size=24, n_frms=8, reader=_reader(video), device="cuda:0", augment=True, rng=random.Random(1),
                                          min_scale=0.3, max_scale=0.5)
    batch = collate_fn([MRDataset(str(tmp_path), str(ann), dev, None)[i] for i in range(2)])
    assert "video" not in batch
    assert batch["video_raw"].shape == (2, 8, 24, 24, 3) and batch["video_raw"].dtype == torch.uint8
    assert batch["video_box"].shape == (2, 4) and batch["video_box"].dtype == torch.int64 and batch["video_flip"].shape == (2,)
    assert len(batch["timestamps"][0]) == 6
    host = AlproVideoEvalProcessor_Stamps(image_size=24, n_frms=8, reader=_reader(video))
    rec = MRDataset(str(tmp_path), str(ann), host, None)[0]
    assert "video_raw" not in rec and rec["video"].shape == (3, 8, 24, 24)
