"""The video front end on the GPU (``mra_video_frames_forward``, ``csrc/video_pre.hip``): the kernel alone against the float64
definition ``preprocess_frames_ref`` under the derived bound of ``tests/video_pre_cases.py`` (every element, both forms of the kernel,
sentinel guards either side of the output), its ``quantize="floor"`` step against the allowed levels, the device processors against the
host processors, and the model end to end from ``video_raw``.

``quantize="floor"``, reading of the issue's cases.  Every element is held to "within the normalisation bound of the normalised form of
an allowed level" (levels: floor(clamp(v64 + e)), e in {-d, 0, +d}).  Noise: at most 1 % of the outputs may have more than one level
(asserted on the float64 reference before the kernel's output is looked at).  A box that on EACH axis is the identity (crop == size) or
one pixel is not noise but a plateau -- every output is one source byte times weights that sum to 1, v64 is a whole number and v64 - d
always reaches the level below -- so it is held to the rule without counting towards the cap, as the constant frames are; the identity on
both axes is held in addition to the stronger identity check (``"floor"`` == ``"none"`` bit for bit == the fp32 normalisation of the
bytes).  Constant frames: the same rule without the cap.
Values 0 and 255: bytes that are all 0 or 255 overshoot the most and the clamp returns them to the levels 0 and 255; every output with
ONE allowed level must then be the fp32 normalisation of that level bit for bit (a constant 255 is not such a case: the fp32 sums land on
either side of 255, measured 16 - 35 % of the pixels at 254 in the CPU emulation, and the plateau rule covers it)."""
import ctypes as C
import random

import pytest
import torch

import video_pre_cases as V
from mraudio_amd import _lib
from mraudio_amd.processors import alpro_processors as P
from mraudio_amd.processors.alpro_processors import AlproVideoEvalProcessor_Stamps, AlproVideoTrainProcessor_Stamps, preprocess_frames_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                        # output elements either side of out, and bytes either side of src (multiples of 16 bytes)
SENTINEL = -12344.0               # representable in f16
QUANT = {"none": 0, "floor": 1}


def _launch(src, rows, idx, w, size, quantize="none", dtype=torch.float32, form=0, src_offset=0, mean=V.MEAN_T, std=V.STD_T):
    """One launch over host arguments: the source sits ``GUARD + src_offset`` bytes into an allocation, the output between two guards
    of SENTINEL.  Returns the [n, 3, size, size] outputs (host) after checking the guards."""
    lib = _lib.lib()
    n, nbytes = int(rows.shape[0]), int(src.numel())
    buf = torch.full((nbytes + 2 * GUARD + src_offset,), 171, dtype=torch.uint8, device=DEV)
    buf[GUARD + src_offset: GUARD + src_offset + nbytes] = src.to(DEV)
    numel = n * 3 * size * size
    dst = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
    rows_d, idx_d, w_d = rows.to(DEV), idx.to(DEV), w.to(DEV)
    args = (C.c_void_p(buf.data_ptr() + GUARD + src_offset), nbytes, _lib.ptr(rows_d), n, _lib.ptr(idx_d), _lib.ptr(w_d), int(idx.shape[0]), size,
            (C.c_float * 3)(*mean), (C.c_float * 3)(*std), QUANT[quantize], C.c_void_p(dst.data_ptr() + GUARD * dst.element_size()), _lib.mra_dtype(dtype))
    if form:
        _lib.check(lib.mra_debug_video_frames_forward(*args, form, _lib.current_stream()), "mra_debug_video_frames_forward")
    else:
        _lib.check(lib.mra_video_frames_forward(*args, _lib.current_stream()), "mra_video_frames_forward")
    torch.cuda.synchronize()
    dst = dst.cpu()
    assert (dst[:GUARD] == SENTINEL).all() and (dst[GUARD + numel:] == SENTINEL).all(), "a write outside out"
    return dst[GUARD: GUARD + numel].view(n, 3, size, size)


def _cases(H, W, size):
    """Every box of the CPU list, flip off and on, as the clips of ONE launch (2 frames each, a table row per clip)."""
    frames = V.noise_frames(2, H, W, seed=H * 100 + size)
    cases = [(name, box, flip) for name, box in V.boxes(H, W, size) for flip in (False, True)]
    return frames, cases


@pytest.mark.parametrize("size", V.SIZES)
@pytest.mark.parametrize("source", V.SOURCES)
def test_kernel_against_float64_under_the_bound(source, size):
    H, W = source
    frames, cases = _cases(H, W, size)
    forms = {f for _, box, _ in cases for f in V.is_staged(box, size)}
    assert forms == ({True, False} if W > size else {True}), "the cases must reach both forms of the kernel wherever a crop can exceed size"
    src, rows, idx, w = V.pack([frames] * len(cases), [c[1] for c in cases], [c[2] for c in cases], size, 2)
    got32 = _launch(src, rows, idx, w, size)
    got16 = _launch(src, rows, idx, w, size, dtype=torch.float16)
    assert torch.isfinite(got32).all()
    for k, (name, box, flip) in enumerate(cases):
        want = V.variant(frames, box, flip, size, V.MEAN_T, V.STD_T, quantize="none")
        for got, f16 in ((got32, False), (got16, True)):
            bound = V.total_bound(frames, box, flip, size, V.MEAN_T, V.STD_T, f16=f16)
            d = (got[2 * k: 2 * k + 2].to(torch.float64) - want).abs()
            worst = (d / bound).max().item()
            print(f"{H} x {W} -> {size}, {name} {box} flip {flip}, {'f16' if f16 else 'f32'}, LDS form per band {V.is_staged(box, size)}: "
                  f"max |d| / bound {worst:.3f}, max |d| {d.max().item():.3e}")
            assert (d <= bound).all(), (name, box, flip, f16, worst)
    # the gather form computes the same chains: the same bits; so does a source that starts one byte later (other alignment of every row)
    assert torch.equal(_launch(src, rows, idx, w, size, form=1), got32)
    assert torch.equal(_launch(src, rows, idx, w, size, src_offset=1), got32)
    assert torch.equal(_launch(src, rows, idx, w, size, dtype=torch.float16, form=1, src_offset=1), got16)


def _step():
    """Three clips of different H x W, boxes and flips, 5 items each; the second and third are shorter and repeat their last frame."""
    clips = [V.noise_frames(5, 20, 27, seed=31), V.noise_frames(3, 33, 40, seed=32), V.noise_frames(1, 16, 16, seed=33)]
    return clips, [(3, 4, 13, 18), (0, 0, 33, 40), (0, 0, 16, 16)], [True, False, False]


def test_clips_of_different_sizes_share_one_launch():
    size, T = 16, 5
    clips, boxes, flips = _step()
    src, rows, idx, w = V.pack(clips, boxes, flips, size, T)
    assert rows.shape[0] == 15 and len(set(rows[:, 0].tolist())) == 9           # 15 outputs over 9 source frames: padding shares a source
    got = _launch(src, rows, idx, w, size)
    for r, (clip, box, flip) in enumerate(zip(clips, boxes, flips)):
        frames = V.expand(clip, T)
        want = V.variant(frames, box, flip, size, V.MEAN_T, V.STD_T, quantize="none")
        bound = V.total_bound(frames, box, flip, size, V.MEAN_T, V.STD_T)
        d = (got[r * T: (r + 1) * T].to(torch.float64) - want).abs()
        print(f"clip {r} {tuple(clip.shape)} box {box} flip {flip}: max |d| / bound {(d / bound).max().item():.3f}")
        assert (d <= bound).all(), r
        s1, r1, i1, w1 = V.pack([clip], [box], [flip], size, T)              # a clip does not depend on its neighbours in the launch
        assert torch.equal(_launch(s1, r1, i1, w1, size), got[r * T: (r + 1) * T]), r
    assert torch.equal(got[7], got[9]) and torch.equal(got[10], got[14]) and not torch.equal(got[6], got[7])   # padded items repeat the last frame
    s2, r2, i2, w2 = V.pack(clips, boxes, flips, size, T, lo=3, hi=12)             # a rank's block: the same rows
    assert r2.shape[0] == 9 and torch.equal(_launch(s2, r2, i2, w2, size), got[3:12])
    assert torch.equal(_launch(src, rows, idx, w, size, src_offset=1), got)
    lib = _lib.lib()
    mean, std = (C.c_float * 3)(*V.MEAN_T), (C.c_float * 3)(*V.STD_T)
    assert lib.mra_video_frames_forward(None, 0, None, 0, None, None, 0, size, mean, std, 0, None, _lib.MRA_F32, None) == 0      # n_out == 0
    assert _launch(src, rows[:0], idx, w, size).shape == (0, 3, size, size)
    # descriptors are clipped inside the kernel: a frame that claims to start past the end of src reads as zeros, nothing faults
    wild = rows.clone()
    wild[0, 0] = src.numel() - 10
    out = _launch(src, wild, idx, w, size)
    assert torch.isfinite(out).all() and torch.equal(out[1:], got[1:])


@pytest.mark.parametrize("size", V.SIZES)
@pytest.mark.parametrize("source", V.SOURCES)
def test_floor_quantisation_takes_an_allowed_level_everywhere(source, size):
    H, W = source
    frames, cases = _cases(H, W, size)
    many = total = 0
    for _, box, flip in cases:               # the cap, on the float64 reference alone, before any kernel output is read
        if V.is_plateau(box, size):          # one source byte per output: held to the rule below, not to the cap (module docstring)
            continue
        levels = V.allowed_levels(frames, box, flip, size)
        many += int(((levels[0] != levels[1]) | (levels[1] != levels[2])).sum())
        total += levels[0].numel()
    print(f"{H} x {W} -> {size}: {many} of {total} outputs ({100.0 * many / total:.3f} %) have more than one allowed level")
    assert many <= 0.01 * total
    src, rows, idx, w = V.pack([frames] * len(cases), [c[1] for c in cases], [c[2] for c in cases], size, 2)
    got32 = _launch(src, rows, idx, w, size, quantize="floor")
    got16 = _launch(src, rows, idx, w, size, quantize="floor", dtype=torch.float16)
    for k, (name, box, flip) in enumerate(cases):
        for got, f16 in ((got32, False), (got16, True)):
            _, worst = V.check_floor(got[2 * k: 2 * k + 2], frames, box, flip, size, V.MEAN_T, V.STD_T, f16=f16)
            print(f"{H} x {W} -> {size}, {name} {box} flip {flip}, {'f16' if f16 else 'f32'}: worst distance to an allowed level / bound {worst:.3f}")
    assert torch.equal(_launch(src, rows, idx, w, size, quantize="floor", form=1), got32)


def test_floor_on_plateaus_extremes_and_the_identity():
    size = 32
    # constant frames: the same rule, no cap (the fp32 sums land on either side of the whole number)
    for value in (1, 128, 254, 255):
        flat = torch.full((1, 33, 40, 3), value, dtype=torch.uint8)
        for box in [(3, 4, 26, 31), (0, 0, 33, 40)]:
            src, rows, idx, w = V.pack([flat], [box], [False], size, 1)
            many, worst = V.check_floor(_launch(src, rows, idx, w, size, quantize="floor"), flat, box, False, size, V.MEAN_T, V.STD_T)
            print(f"constant {value}, {box}: {many} outputs with two allowed levels, worst distance / bound {worst:.3f}")
    # values 0 and 255: every output with one allowed level is the fp32 normalisation of it, bit for bit; most sit on the clamp
    binary = V.binary_frames(2, 33, 40, seed=3)
    for box, flip in [((0, 0, 33, 40), True), ((4, 6, 5, 7), False), ((3, 4, 26, 31), False)]:
        src, rows, idx, w = V.pack([binary], [box], [flip], size, 2)
        got = _launch(src, rows, idx, w, size, quantize="floor")
        V.check_floor(got, binary, box, flip, size, V.MEAN_T, V.STD_T)
        single, want = V.exact_levels(binary, box, flip, size, V.MEAN_T, V.STD_T)
        assert single.double().mean().item() > 0.95 and torch.equal(got[single], want[single]), box
    black = torch.zeros(1, 33, 40, 3, dtype=torch.uint8)
    src, rows, idx, w = V.pack([black], [(3, 4, 26, 31)], [False], size, 1)
    single, want = V.exact_levels(black, (3, 4, 26, 31), False, size, V.MEAN_T, V.STD_T)
    assert single.all() and torch.equal(_launch(src, rows, idx, w, size, quantize="floor"), want)
    # the identity route: "floor" == "none" bit for bit == the fp32 normalisation of the bytes, with the default mean / std the host
    # processor's own output
    sq = V.noise_frames(3, size, size, seed=41)
    src, rows, idx, w = V.pack([sq], [(0, 0, size, size)], [False], size, 3)
    a = _launch(src, rows, idx, w, size, quantize="none", mean=P.MEAN, std=P.STD)
    b = _launch(src, rows, idx, w, size, quantize="floor", mean=P.MEAN, std=P.STD)
    host = P._normalise(sq.permute(3, 0, 1, 2).float(), None, None).permute(1, 0, 2, 3)
    assert torch.equal(a, b) and torch.equal(a, host)
    assert torch.equal(_launch(src, rows, idx, w, size, quantize="floor", mean=P.MEAN, std=P.STD, form=1), a)


def _reader(frames, fps=2.0):
    return lambda vpath, h, w: (frames.numpy(), fps)


def test_device_processors_against_the_host_processors():
    size, T = 32, 6
    # eval, frames decoded at the model's size: the identity; host and device are each within the normalisation bound of float64
    video = V.noise_frames(4, size, size, seed=51)
    host = AlproVideoEvalProcessor_Stamps(image_size=size, n_frms=T, reader=_reader(video))
    dev = AlproVideoEvalProcessor_Stamps(image_size=size, n_frms=T, reader=_reader(video), device=DEV)
    want, idx_h, fps_h = host("v")
    got, idx_d, fps_d = dev("v")
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == want.shape == (3, T, size, size) and list(idx_h) == list(idx_d) and fps_h == fps_d
    bound = 2.0 * V.norm_bound(V.expand(video, T).permute(0, 3, 1, 2).to(torch.float64)).permute(1, 0, 2, 3)
    d = (got.cpu().double() - want.double()).abs()
    print(f"eval processor, device against host: max |d| / bound {(d / bound).max().item():.3f}")
    assert (d <= bound).all()
    # train with the augmentation, a fixed rng, frames of another size: the host applies the float64 definition
    video = V.noise_frames(9, 33, 40, seed=52)
    kw = dict(image_size=size, n_frms=T, reader=_reader(video), min_scale=0.4, max_scale=0.8, augment=True, mean=V.MEAN_T, std=V.STD_T)
    want, idx_h, _ = AlproVideoTrainProcessor_Stamps(rng=random.Random(7), **kw)("v")
    dev = AlproVideoTrainProcessor_Stamps(rng=random.Random(7), device=DEV, **kw)
    frames, box, flip, idx_d, _ = dev.raw("v")
    dev.rng = random.Random(7)
    got, _, _ = dev("v")
    assert list(idx_h) == list(idx_d) and tuple(box.tolist()) != (0, 0, 33, 40)
    many, worst = V.check_floor(got.cpu().permute(1, 0, 2, 3), frames, tuple(box.tolist()), bool(flip), size, V.MEAN_T, V.STD_T)
    differs = ((got.cpu() - want).abs() > 1e-4).sum().item()          # another LEVEL than the host took (a level is 1 / (255 std) ~ 0.02 apart)
    print(f"train processor, box {box.tolist()} flip {flip}: worst distance to an allowed level / bound {worst:.3f}; {many} outputs with two allowed "
          f"levels, {differs} where device and host took different ones")
    assert differs <= many
    # "none" against the float64 host output under the kernel's bound (+ the host's own rounding to fp32)
    kw["quantize"] = "none"
    want, _, _ = AlproVideoTrainProcessor_Stamps(rng=random.Random(8), **kw)("v")
    dev = AlproVideoTrainProcessor_Stamps(rng=random.Random(8), device=DEV, **kw)
    frames, box, flip, _, _ = dev.raw("v")
    dev.rng = random.Random(8)
    got, _, _ = dev("v")
    bound = V.total_bound(frames, tuple(box.tolist()), bool(flip), size, V.MEAN_T, V.STD_T).permute(1, 0, 2, 3) + V.U * want.double().abs()
    d = (got.cpu().double() - want.double()).abs()
    print(f"train processor, quantize none: max |d| / bound {(d / bound).max().item():.3f}")
    assert (d <= bound).all()
    # flat / batch: sample-major items, a rank's block, clips of different sizes as a list, f16 by default
    clips = [frames, V.noise_frames(2, 20, 27, seed=53)]
    boxes, flips = [box.tolist(), [2, 3, 15, 20]], [flip, 1]
    full = dev.flat(clips, boxes, flips)
    assert full.dtype == torch.float16 and full.shape == (2 * T, 3, size, size)
    assert torch.equal(dev.flat(clips, boxes, flips, 4, 9), full[4:9]) and dev.flat(clips, boxes, flips, 5, 5).shape == (0, 3, size, size)
    batch = dev.batch(clips, boxes, flips)
    assert batch.shape == (2, 3, T, size, size) and batch.permute(0, 2, 1, 3, 4).is_contiguous()          # a view of the sample-major frames
    assert torch.equal(batch.permute(0, 2, 1, 3, 4).reshape(2 * T, 3, size, size), full)
    assert torch.equal(full[T + 1], full[2 * T - 1])                      # the short clip repeats its last frame
    assert torch.equal(dev.flat(clips, boxes, flips, out_dtype=torch.float32)[:T].permute(1, 0, 2, 3), got)
    with pytest.raises(ValueError, match="inside"):
        dev.flat(clips, [[0, 0, 34, 40], boxes[1]], flips)


def test_end_to_end_from_video_raw_against_the_host_pixels():
    from mraudio_amd.models.eva_vit import HipEvaViTg
    from mraudio_amd.models.xinstructblip import XInstructBLIP

    B, T, S = 2, 3, 224
    hip = HipEvaViTg(depth=2, device=DEV).eval().init_seeded_(3)
    proc = AlproVideoTrainProcessor_Stamps(image_size=S, n_frms=T, device=DEV, augment=True)
    model = XInstructBLIP(seed=0, perturb=True, device=DEV, modalities=["video"], video_encoder=hip, video_processor=proc)
    raw = V.noise_frames(B * T, S, S, seed=61).view(B, T, S, S, 3)
    raw = (raw.float() * 0.5 + raw.float().roll(1, 2) * 0.25 + raw.float().roll(1, 3) * 0.25).to(torch.uint8)     # some spatial correlation
    boxes, flips = torch.tensor([[0, 0, S, S], [9, 17, 201, 190]]), torch.tensor([0, 1])
    host = torch.stack([preprocess_frames_ref(raw[b], boxes[b].tolist(), bool(flips[b]), S, quantize="floor").permute(1, 0, 2, 3) for b in range(B)])
    base = {"text_input": ["Query: a dog runs.\nRelevant windows: ", "Query: the door closes.\nRelevant windows: "],
            "timestamps": [[0, 2, 4], [1, 3, 5]], "duration": [6, 6]}
    model.encode_chunk = 4                     # 6 frames -> chunks of 4 + 2
    a = model.encode_fuse({**base, "video_raw": raw, "video_box": boxes, "video_flip": flips})
    b = model.encode_fuse({**base, "video": host.to(torch.float16)})
    torch.cuda.synchronize()
    scale = b["fused"].abs().max().item()
    d = (a["fused"] - b["fused"]).abs().max().item()
    print(f"end to end, video_raw against the host processor's pixels in f16: max |d fused logit| {d:.3e} on a scale of {scale:.3f}")
    assert a["fused"].shape == (B * T,) and d <= 2e-3 * scale          # the parity bar of tests/test_gpu_vit.py
    assert torch.equal(a["spans"], b["spans"])
