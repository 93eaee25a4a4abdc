"""Cases, references and bounds shared by ``test_video_pre_cpu.py`` and ``test_gpu_video_pre.py`` (the video front end:
``mraudio_amd/processors/alpro_processors.py`` and ``csrc/video_pre.hip``).

References.  ``torch_reference``: torch's own ``interpolate(crop, size, "bicubic", align_corners=False)`` in float64, the flip, the
normalisation -- what the definition ``preprocess_frames_ref`` is pinned to.  ``variant``: the definition restated with every choice
a parameter, so that each mutant of the CPU tests is one argument away from it.  ``emulate``: the kernel's arithmetic in fp32 (tables
rounded to fp32 once; vertical then horizontal fma chain, ascending taps, from 0; clamp and floor; two divisions).

The bound (all in units of u = 2^-24, the fp32 unit roundoff; S = sum |w_y| |w_x| |p| over the 16 taps, in float64):
  interpolation   d = (8 + 2 + 1) u S: eight fma roundings on the path of a tap (four vertical, four horizontal), the two weights'
                  roundings to fp32, and one u for the second-order terms and the float64 reference's own error;
  normalisation   out = ((h / 255) - m) / s with fp32 m, s: n(h) = u ((|h| / 255 + |m|) / s + 4 |out|) -- the first division's rounding
                  and the rounding of m, both divided by s; the subtraction's, the second division's and s's own rounding, each
                  relative to out; one more |out| for second-order terms;
  total           d / (255 s) + n(h); an f16 output adds one f16 rounding, 2^-11 (|out| + total) + 2^-25 (the subnormal spacing).
"""
import numpy as np
import torch
import torch.nn.functional as F

from mraudio_amd.processors.alpro_processors import MEAN, STD, crop_resize_table

U = 2.0 ** -24
INTERP_ROUNDINGS = 8 + 2 + 1
MEAN_T = (0.45, 0.5, 0.4)          # a second mean / std, so that a swapped channel shows in the normalisation too
STD_T = (0.25, 0.3, 0.2)

# (H, W) of the sources and the output sizes of the GPU tests; 27 * 3 = 81-byte rows exercise the unaligned loads
SOURCES = ((20, 27), (33, 40))
SIZES = (16, 32)
BAND, RAW_ROWS = 8, 12             # csrc/video_pre.hip: output rows per workgroup, source rows its LDS form stages


def noise_frames(T, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (T, H, W, 3), generator=g, dtype=torch.uint8)


def boxes(H, W, size):
    """(name, (top, left, height, width)): interior, touching each edge, one pixel high, up- and downscale, both sides of the kernel's
    two thresholds (crop width == size / size + 1, where the gather form takes over), the whole frame."""
    out = [("interior", (3, 4, H - 7, W - 9)),
           ("top edge", (0, 5, H // 2, W // 2)),
           ("bottom edge", (H - H // 2, 2, H // 2, W // 3)),
           ("left edge", (2, 0, H // 2 + 1, W // 2 + 1)),
           ("right edge", (1, W - W // 2, H // 3, W // 2)),
           ("one pixel high", (H // 2, 3, 1, W - 6)),
           ("one pixel wide", (2, W // 2, H - 4, 1)),
           ("upscale", (4, 6, 5, 7)),
           ("whole frame", (0, 0, H, W))]
    if W >= size + 1:
        out += [("crop width == size", (1, W - size, min(H - 1, size), size)), ("crop width == size + 1", (0, 0, min(H, size), size + 1))]
    # narrow crops (the width never decides) whose bands span about RAW_ROWS source rows: at size 16 a band of a 22-row crop spans 12
    # source rows, the most the LDS form stages, and one of a 23-row crop 13
    for name, s in (("rows at the staged span", 1.375), ("rows just beyond the staged span", 1.4375), ("rows beyond the staged span", 2.0)):
        if round(s * size) <= H:
            out.append((name, (H - round(s * size), 1, round(s * size), size // 2 + 1)))
    return out


def is_staged(box, size):
    """The kernel's rule for its LDS form, per band of 8 output rows: [form of band 0, form of band 1, ...]."""
    top, left, bh, bw = box
    iy, _ = crop_resize_table(bh, top, size)
    return [bw <= size and int(iy[r0 + BAND - 1, 3] - iy[r0, 0]) + 1 <= RAW_ROWS for r0 in range(0, size, BAND)]


def is_plateau(box, size):
    """On each axis the crop is the identity or one pixel: every output is ONE source byte times weights that sum to 1."""
    return box[2] in (1, size) and box[3] in (1, size)


def _norm(h, mean, std):
    m = torch.tensor(MEAN if mean is None else mean, dtype=torch.float64).view(1, 3, 1, 1)
    s = torch.tensor(STD if std is None else std, dtype=torch.float64).view(1, 3, 1, 1)
    return (h / 255.0 - m) / s


def torch_reference(frames, box, flip, size, mean=None, std=None):
    """torch's bicubic on the cropped clip, float64: [T, 3, size, size], normalised, quantize "none"."""
    top, left, bh, bw = box
    x = frames.to(torch.float64).permute(0, 3, 1, 2)[:, :, top: top + bh, left: left + bw]
    h = F.interpolate(x, size=(size, size), mode="bicubic", align_corners=False)
    if flip:
        h = h.flip(3)
    return _norm(h, mean, std)


def table(n_src_crop, offset, n_out, n_src, A=-0.75, geometry="half_pixel", clamp_to="crop"):
    """``crop_resize_table`` with its choices as parameters (the defaults are the definition's)."""
    if geometry == "half_pixel":
        x = (n_src_crop / n_out) * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5
    elif geometry == "no_half_pixel":
        x = (n_src_crop / n_out) * np.arange(n_out, dtype=np.float64)
    elif geometry == "align_corners":
        x = np.arange(n_out, dtype=np.float64) * ((n_src_crop - 1) / max(n_out - 1, 1))
    else:
        raise ValueError(geometry)
    fl = np.floor(x)
    t = x - fl
    x0, x1, x2, x3 = t + 1.0, t, 1.0 - t, 2.0 - t
    w = np.stack([((A * x0 - 5.0 * A) * x0 + 8.0 * A) * x0 - 4.0 * A, ((A + 2.0) * x1 - (A + 3.0)) * x1 * x1 + 1.0,
                  ((A + 2.0) * x2 - (A + 3.0)) * x2 * x2 + 1.0, ((A * x3 - 5.0 * A) * x3 + 8.0 * A) * x3 - 4.0 * A], axis=1)
    taps = fl.astype(np.int64)[:, None] - 1 + np.arange(4)[None, :]
    if clamp_to == "crop":
        idx = np.clip(taps, 0, n_src_crop - 1) + offset
    else:                     # the mutant: taps run on into the source frame around the crop
        idx = np.clip(taps + offset, 0, n_src - 1)
    return idx, w


def variant(frames, box, flip, size, mean=None, std=None, quantize="floor", A=-0.75, geometry="half_pixel", clamp_to="crop",
            flip_first=False, channels=(0, 1, 2), want_h=False):
    """The definition, float64, every choice a parameter.  ``flip_first``: the frame is mirrored BEFORE the crop offset is applied;
    ``quantize``: "none", "floor" (the definition), "round", "floor_unclamped"."""
    x = frames.to(torch.float64)[..., list(channels)]
    H, W = x.shape[1], x.shape[2]
    top, left, bh, bw = box
    if flip and flip_first:
        x = x.flip(2)
    iy, wy = table(bh, top, size, H, A, geometry, clamp_to)
    ix, wx = table(bw, left, size, W, A, geometry, clamp_to)
    v = sum(torch.from_numpy(wy[:, j]).view(1, size, 1, 1) * x[:, torch.from_numpy(iy[:, j])] for j in range(4))
    h = sum(torch.from_numpy(wx[:, k]).view(1, 1, size, 1) * v[:, :, torch.from_numpy(ix[:, k])] for k in range(4))
    if flip and not flip_first:
        h = h.flip(2)
    if quantize == "floor":
        h = h.clamp(0.0, 255.0).floor()
    elif quantize == "round":
        h = h.clamp(0.0, 255.0).round()
    elif quantize == "floor_unclamped":
        h = h.floor()
    elif quantize != "none":
        raise ValueError(quantize)
    h = h.permute(0, 3, 1, 2)
    return h if want_h else _norm(h, mean, std)


def abs_sum(frames, box, flip, size):
    """S = sum |w_y| |w_x| |p| per output, [T, 3, size, size] float64."""
    x = frames.to(torch.float64)
    top, left, bh, bw = box
    iy, wy = crop_resize_table(bh, top, size)
    ix, wx = crop_resize_table(bw, left, size)
    v = sum(torch.from_numpy(np.abs(wy[:, j])).view(1, size, 1, 1) * x[:, torch.from_numpy(iy[:, j])] for j in range(4))
    s = sum(torch.from_numpy(np.abs(wx[:, k])).view(1, 1, size, 1) * v[:, :, torch.from_numpy(ix[:, k])] for k in range(4))
    if flip:
        s = s.flip(2)
    return s.permute(0, 3, 1, 2)


def interp_bound(frames, box, flip, size):
    """d: the fp32 interpolation's distance from the float64 one, in pixel units (0 .. 255)."""
    return INTERP_ROUNDINGS * U * abs_sum(frames, box, flip, size)


def norm_bound(h, mean=None, std=None):
    """n(h): the fp32 normalisation's distance from the float64 normalisation of the same h [T, 3, S, S]."""
    m = torch.tensor(MEAN if mean is None else mean, dtype=torch.float64).view(1, 3, 1, 1)
    s = torch.tensor(STD if std is None else std, dtype=torch.float64).view(1, 3, 1, 1)
    return U * ((h.abs() / 255.0 + m.abs()) / s + 4.0 * _norm(h, mean, std).abs())


def f16_bound(out, total):
    return 2.0 ** -11 * (out.abs() + total) + 2.0 ** -25


def total_bound(frames, box, flip, size, mean=None, std=None, f16=False):
    """The kernel (quantize "none") against ``variant(..., quantize="none")``: per element."""
    s = torch.tensor(STD if std is None else std, dtype=torch.float64).view(1, 3, 1, 1)
    h = variant(frames, box, flip, size, quantize="none", want_h=True)
    total = interp_bound(frames, box, flip, size) / (255.0 * s) + norm_bound(h, mean, std)
    return total + f16_bound(_norm(h, mean, std), total) if f16 else total


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate(frames, box, flip, size, mean=None, std=None, quantize="floor"):
    """The kernel's arithmetic on the CPU, fp32: [T, 3, size, size] float32 (torch)."""
    x = frames.numpy().astype(np.float32)
    top, left, bh, bw = box
    iy, wy = crop_resize_table(bh, top, size)
    ix, wx = crop_resize_table(bw, left, size)
    wy, wx = wy.astype(np.float32), wx.astype(np.float32)
    v = np.zeros((x.shape[0], size, x.shape[2], 3), dtype=np.float32)
    for j in range(4):
        v = _fma32(wy[:, j].reshape(1, size, 1, 1), x[:, iy[:, j]], v)
    h = np.zeros((x.shape[0], size, size, 3), dtype=np.float32)
    for k in range(4):
        h = _fma32(wx[:, k].reshape(1, 1, size, 1), v[:, :, ix[:, k]], h)
    if flip:
        h = h[:, :, ::-1]
    if quantize == "floor":
        h = np.floor(np.minimum(np.maximum(h, np.float32(0.0)), np.float32(255.0)))
    m = np.asarray(MEAN if mean is None else mean, dtype=np.float32).reshape(1, 1, 1, 3)
    s = np.asarray(STD if std is None else std, dtype=np.float32).reshape(1, 1, 1, 3)
    out = (h / np.float32(255.0) - m) / s
    assert out.dtype == np.float32
    return torch.from_numpy(np.ascontiguousarray(out.transpose(0, 3, 1, 2)))


def allowed_levels(frames, box, flip, size):
    """quantize "floor": the levels an output may take, floor(clamp(v64 + e)) for e in {-d, 0, +d}: [3][T, 3, S, S] float64."""
    h = variant(frames, box, flip, size, quantize="none", want_h=True)
    d = interp_bound(frames, box, flip, size)
    return [(h + e).clamp(0.0, 255.0).floor() for e in (-d, torch.zeros_like(d), d)]


def check_floor(got, frames, box, flip, size, mean=None, std=None, f16=False):
    """Every element of ``got`` (the kernel under quantize "floor") is within the normalisation bound of the normalised form of one
    allowed level.  Returns (number of elements with more than one allowed level, worst distance / bound)."""
    levels = allowed_levels(frames, box, flip, size)
    ok = torch.zeros(got.shape, dtype=torch.bool)
    worst = torch.full(got.shape, float("inf"), dtype=torch.float64)
    for lv in levels:
        want = _norm(lv, mean, std)
        b = norm_bound(lv, mean, std)
        if f16:
            b = b + f16_bound(want, b)
        dist = (got.to(torch.float64) - want).abs()
        ok |= dist <= b
        worst = torch.minimum(worst, dist / b)
    assert ok.all(), f"{int((~ok).sum())} of {ok.numel()} outputs match no allowed level; worst distance / bound {worst.max().item():.3f}"
    return int(((levels[0] != levels[1]) | (levels[1] != levels[2])).sum()), worst.max().item()


def binary_frames(T, H, W, seed):
    """Every byte 0 or 255: the strongest overshoot, so most outputs sit on the clamp."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 2, (T, H, W, 3), generator=g, dtype=torch.uint8) * 255).to(torch.uint8)


def exact_levels(frames, box, flip, size, mean=None, std=None):
    """quantize "floor": (mask of the outputs with ONE allowed level, the fp32 normalisation of that level).  There the kernel's h is
    that whole number whatever its roundings, and two IEEE divisions of it leave no freedom: an fp32 output must equal it bit for bit."""
    levels = allowed_levels(frames, box, flip, size)
    single = (levels[0] == levels[1]) & (levels[1] == levels[2])
    m = torch.tensor(MEAN if mean is None else mean, dtype=torch.float32).view(1, 3, 1, 1)
    s = torch.tensor(STD if std is None else std, dtype=torch.float32).view(1, 3, 1, 1)
    return single, (levels[1].to(torch.float32) / 255.0 - m) / s


def pack(clips, boxes_, flips, size, n_frms, lo=None, hi=None):
    """The arguments of one ``mra_video_frames_forward`` over items [lo, hi) of the sample-major ``len(clips) * n_frms`` frames, as the
    device processor builds them, with the Python table rounded to fp32: (src uint8 [bytes], rows int64 [n, 5], tap_idx int16
    [n_tab, 2, size, 4], tap_w fp32 [n_tab, 2, size, 4]).  A clip shorter than n_frms repeats its last frame (rows share the source)."""
    B = len(clips)
    lo, hi = (0 if lo is None else lo), (B * n_frms if hi is None else hi)
    parts, rows, idx_t, w_t, base = [], [], [], [], 0
    for r in range(B):
        clip = clips[r]
        n_src, H, W = clip.shape[0], clip.shape[1], clip.shape[2]
        top, left, bh, bw = boxes_[r]
        iy, wy = crop_resize_table(bh, top, size)
        ix, wx = crop_resize_table(bw, left, size)
        idx_t.append(torch.from_numpy(np.stack([iy, ix])).to(torch.int16))
        w_t.append(torch.from_numpy(np.stack([wy, wx]).astype(np.float32)))
        parts.append(clip.reshape(-1))
        for i in range(n_frms):
            if lo <= r * n_frms + i < hi:
                rows.append((base + min(i, n_src - 1) * H * W * 3, H, W, r, int(flips[r])))
        base += clip.numel()
    return torch.cat(parts), torch.tensor(rows, dtype=torch.int64).reshape(-1, 5), torch.stack(idx_t), torch.stack(w_t)


def expand(clip, n_frms):
    """The n_frms source frames behind a clip's items (last frame repeated)."""
    return clip[[min(i, clip.shape[0] - 1) for i in range(n_frms)]]
