"""Video processors with the reference's signatures (``processors/alpro_processors.py:14-85``).

Video decoding (decord) and the LAVIS Alpro transforms are outside the hot path (SURVEY.md section 2,
row 10); what the path consumes from them is integer: the sampled frame indices and, through
``utils/mr_dataset.py:44``, the per-position timestamps.  Those are restated here exactly.  The
decoder is pluggable: ``reader(vpath, height, width) -> (frames uint8/float [T, H, W, C], fps)``.

The pixel side of the transforms -- LAVIS ``AlproVideoTrainProcessor.transform``: a random resized crop of the whole clip
(bicubic), a random horizontal flip of the whole clip, ``ToUint8``, ``/ 255``, ``Normalize`` -- is defined here in float64
(``crop_resize_table``, ``preprocess_frames_ref``) and run on the GPU by ``csrc/video_pre.hip`` (``mra_video_frames_forward``)
for processors built with ``device=``.  The crop-resize arithmetic is pinned: LAVIS' crop is
``torch.nn.functional.interpolate(clip[..., i:i+h, j:j+w], size, mode="bicubic", align_corners=False)``, and
``tests/test_video_pre_cpu.py`` holds the definition to it.  Unpinned: the crop-box draw (``random_resized_crop_params`` restates
torchvision's published ``RandomResizedCrop.get_params``; torchvision is not part of this build) and decord's decode-time resize to
``image_size``, which stays inside the pluggable ``reader``.  ``ToUint8`` in the reference is a bare cast, undefined for the
overshoot bicubic produces (about -36 .. 299 on noise); this build clamps to [0, 255] first, then floors.
"""
from __future__ import annotations

import math
import random as rnd
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)
CUBIC_A = -0.75                     # torch's bicubic coefficient
QUANTIZE = {"none": 0, "floor": 1}  # MRA_VIDEO_QUANT_* of include/mra.h


def frame_indices(vlen: int, n_frms: int, sampling: str = "uniform", rng: Optional[rnd.Random] = None):
    """Reference ``load_video`` (``:19-33``): ``n = min(n_frms, vlen)``; uniform =
    ``np.linspace(0, vlen, n, endpoint=False).astype(int)``; random = one frame per interval of
    ``np.linspace(0, vlen, n + 1).astype(int)`` (``low`` itself when the interval is empty)."""
    n = min(n_frms, vlen)
    if sampling == "uniform":
        return np.linspace(start=0, stop=vlen, num=n, endpoint=False).astype(int)
    if sampling == "random":
        r = rng or rnd
        iv = np.linspace(start=0, stop=vlen, num=n + 1).astype(int)
        return [int(lo) if lo == hi else r.choice(range(int(lo), int(hi))) for lo, hi in zip(iv[:-1], iv[1:])]
    raise NotImplementedError(f"Sampling strategy '{sampling}' is not implemented.")


def timestamps_from_indices(indices: Sequence[int], fps: float) -> List[int]:
    """``utils/mr_dataset.py:44``: ``[round(idx / fps) for idx in indices]`` (Python banker's rounding)."""
    return [round(int(i) / fps) for i in indices]


def _normalise(frames: torch.Tensor, mean, std) -> torch.Tensor:
    m = torch.tensor(mean if mean is not None else MEAN).view(3, 1, 1, 1)
    s = torch.tensor(std if std is not None else STD).view(3, 1, 1, 1)
    return (frames / 255.0 - m) / s


# ---- the pixel transform: definition (float64) -------------------------------------------------------------------------
def crop_resize_table(n_src_crop: int, offset: int, n_out: int) -> Tuple[np.ndarray, np.ndarray]:
    """One axis of torch's bicubic ``interpolate(..., align_corners=False)`` from a crop of ``n_src_crop`` pixels that starts at
    ``offset`` of the source frame to ``n_out`` pixels: ``(idx int64 [n_out, 4], w float64 [n_out, 4])``.  Output ``o`` sits at source
    coordinate ``x = (n_src_crop / n_out)(o + 0.5) - 0.5`` of the crop; its taps are ``floor(x) - 1 .. floor(x) + 2`` with the cubic
    convolution weights of coefficient A = -0.75 at ``t = x - floor(x)``.  ``idx`` is absolute in the source frame and clamped to the
    CROP, ``[offset, offset + n_src_crop)``: ``interpolate`` only ever sees the cropped tensor.  ``mra_video_crop_table`` builds the
    same table (weights rounded to fp32 once)."""
    if n_src_crop <= 0 or n_out <= 0 or offset < 0:
        raise ValueError("crop_resize_table: n_src_crop and n_out must be > 0 and offset >= 0")
    A = CUBIC_A
    scale = float(n_src_crop) / float(n_out)
    x = scale * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5
    fl = np.floor(x)
    t = x - fl
    x0, x1, x2, x3 = t + 1.0, t, 1.0 - t, 2.0 - t
    w = np.stack([((A * x0 - 5.0 * A) * x0 + 8.0 * A) * x0 - 4.0 * A,
                  ((A + 2.0) * x1 - (A + 3.0)) * x1 * x1 + 1.0,
                  ((A + 2.0) * x2 - (A + 3.0)) * x2 * x2 + 1.0,
                  ((A * x3 - 5.0 * A) * x3 + 8.0 * A) * x3 - 4.0 * A], axis=1)
    idx = np.clip(fl.astype(np.int64)[:, None] - 1 + np.arange(4, dtype=np.int64)[None, :], 0, n_src_crop - 1) + int(offset)
    return idx, w


def whole_frame_box(H: int, W: int) -> Tuple[int, int, int, int]:
    return (0, 0, int(H), int(W))


def preprocess_frames_ref(frames_u8, box=None, flip: bool = False, size: int = 224, mean=None, std=None,
                          quantize: str = "floor") -> torch.Tensor:
    """The float64 definition of the pixel transform: ``frames_u8 [T, H, W, 3]`` -> ``[T, 3, size, size]``.  ``box = (top, left,
    height, width)`` (None: the whole frame).  In order: the vertical then the horizontal 4-tap sums of ``crop_resize_table``; the flip,
    a reversal of the output x axis AFTER the resize, as the reference orders it; for ``quantize="floor"`` the reference's ``ToUint8`` as
    ``floor(clamp(v, 0, 255))`` (``"none"`` skips it); ``(v / 255 - mean_c) / std_c``.  With the whole frame as the box, no flip and
    ``size == H == W`` the weights are exactly 0 / 1 and this is the normalisation of the bytes, in both quantize modes."""
    if quantize not in QUANTIZE:
        raise ValueError(f"quantize: 'floor' or 'none', got {quantize!r}")
    x = torch.as_tensor(np.asarray(frames_u8)).to(torch.float64)
    if x.dim() != 4 or x.shape[-1] != 3:
        raise ValueError(f"frames: [T, H, W, 3], got {list(x.shape)}")
    H, W = int(x.shape[1]), int(x.shape[2])
    top, left, bh, bw = whole_frame_box(H, W) if box is None else (int(b) for b in box)
    if not (0 <= top and 0 < bh and top + bh <= H and 0 <= left and 0 < bw and left + bw <= W):
        raise ValueError(f"box {(top, left, bh, bw)} does not lie inside the {H} x {W} frame")
    iy, wy = crop_resize_table(bh, top, size)
    ix, wx = crop_resize_table(bw, left, size)
    wy_t, wx_t = torch.from_numpy(wy), torch.from_numpy(wx)
    v = torch.zeros(x.shape[0], size, W, 3, dtype=torch.float64)
    for j in range(4):
        v = v + wy_t[:, j].view(1, size, 1, 1) * x[:, torch.from_numpy(iy[:, j])]
    h = torch.zeros(x.shape[0], size, size, 3, dtype=torch.float64)
    for k in range(4):
        h = h + wx_t[:, k].view(1, 1, size, 1) * v[:, :, torch.from_numpy(ix[:, k])]
    if flip:
        h = h.flip(2)
    if quantize == "floor":
        h = h.clamp(0.0, 255.0).floor()
    m = torch.tensor(mean if mean is not None else MEAN, dtype=torch.float64).view(1, 3, 1, 1)
    s = torch.tensor(std if std is not None else STD, dtype=torch.float64).view(1, 3, 1, 1)
    return (h.permute(0, 3, 1, 2) / 255.0 - m) / s


def random_resized_crop_params(H: int, W: int, scale: Sequence[float], ratio: Sequence[float] = (3.0 / 4.0, 4.0 / 3.0),
                               rng: Optional[rnd.Random] = None) -> Tuple[int, int, int, int]:
    """torchvision's published ``RandomResizedCrop.get_params``, restated (unpinned: torchvision is not part of this build, and its draws
    come from torch's generator, these from ``rng``): ten tries of a uniform area share in ``scale`` and a log-uniform aspect ratio in
    ``ratio``, ``w = round(sqrt(area * ratio))``, ``h = round(sqrt(area / ratio))``, accepted when the box fits, then a uniform
    position; otherwise the ratio-clamped central crop.  Returns ``(top, left, height, width)``."""
    r = rng or rnd
    area = H * W
    log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
    for _ in range(10):
        target = area * r.uniform(scale[0], scale[1])
        aspect = math.exp(r.uniform(log_ratio[0], log_ratio[1]))
        w = int(round(math.sqrt(target * aspect)))
        h = int(round(math.sqrt(target / aspect)))
        if 0 < w <= W and 0 < h <= H:
            return r.randint(0, H - h), r.randint(0, W - w), h, w
    in_ratio = float(W) / float(H)
    if in_ratio < min(ratio):
        w = W
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = H
        w = int(round(h * max(ratio)))
    else:
        w, h = W, H
    return (H - h) // 2, (W - w) // 2, h, w


def random_flip(rng: Optional[rnd.Random] = None) -> bool:
    """The reference's ``RandomHorizontalFlipVideo``: p = 0.5, one draw per clip."""
    return (rng or rnd).random() < 0.5


class _StampsProcessor:
    sampling = "uniform"
    quantize = "none"      # the eval transform's ToUint8 acts on decoded bytes: nothing to quantize

    def __init__(self, image_size=224, mean=None, std=None, n_frms=60, full_video=True, reader: Optional[Callable] = None, device=None):
        self.image_size, self.mean, self.std, self.n_frms, self.full_video = image_size, mean, std, n_frms, full_video
        self.reader = reader
        # a CUDA device selects the device route: the decoded bytes go up as they are and csrc/video_pre.hip crops, resizes, flips and
        # normalises them (raw / flat / batch; __call__ returns the clip on the device).  None: the host processor, unchanged.
        self.device = torch.device(device) if device is not None else None
        if self.device is not None:
            if self.device.type != "cuda":
                raise ValueError("device: None (the host processor) or a CUDA device (the HIP front end)")
            if int(image_size) % 8 != 0:
                raise ValueError("the HIP front end needs image_size to be a multiple of 8")
        self._tables = {}

    def _read(self, vpath):
        if self.reader is None:
            raise RuntimeError("no video reader configured (decord is not part of this build); pass reader=")
        frames, fps = self.reader(vpath, self.image_size, self.image_size)
        vlen = int(frames.shape[0])
        indices = frame_indices(vlen, self.n_frms, self.sampling, getattr(self, "rng", None))
        return np.asarray(frames)[np.asarray(indices)], indices, fps

    def _draw(self, H: int, W: int) -> Tuple[Tuple[int, int, int, int], bool]:
        """The clip's crop box and flip: the whole frame, unflipped, unless a train processor augments."""
        return whole_frame_box(H, W), False

    def __call__(self, vpath) -> Tuple[torch.Tensor, object, float]:
        if self.device is not None:
            frames, box, flip, indices, fps = self.raw(vpath)
            return self.batch([frames], [box], [flip], out_dtype=torch.float32)[0], indices, fps
        sel, indices, fps = self._read(vpath)
        transformed = self._host(sel)
        pad = self.n_frms - transformed.shape[1]
        if pad > 0:  # repeat the last frame (reference :79-83)
            transformed = torch.cat([transformed, transformed[:, -1:].repeat(1, pad, 1, 1)], dim=1)
        return transformed, indices, fps

    def _host(self, sel) -> torch.Tensor:
        clip = torch.as_tensor(sel).permute(3, 0, 1, 2).float()  # (C, T, H, W)
        return _normalise(clip, self.mean, self.std)

    # ---- the device route ----------------------------------------------------------------------------------------------
    def raw(self, vpath):
        """What the device route needs of one clip, all on the host: ``(frames uint8 [n_frms, H, W, 3], box int64 [4] = (top, left,
        height, width), flip 0 / 1, indices, fps)``.  The sampled frames are padded to ``n_frms`` by repeating the last one, in uint8;
        box is the whole frame and flip 0 unless a train processor augments."""
        sel, indices, fps = self._read(vpath)
        frames = torch.as_tensor(sel)
        if frames.dtype != torch.uint8:
            raise ValueError(f"the device route takes the decoder's uint8 frames, the reader returned {frames.dtype}")
        if frames.dim() != 4 or frames.shape[-1] != 3:
            raise ValueError(f"frames: [T, H, W, 3], got {list(frames.shape)}")
        pad = self.n_frms - int(frames.shape[0])
        if pad > 0:
            frames = torch.cat([frames, frames[-1:].repeat(pad, 1, 1, 1)], dim=0)
        box, flip = self._draw(int(frames.shape[1]), int(frames.shape[2]))
        return frames.contiguous(), torch.tensor(box, dtype=torch.int64), int(flip), indices, fps

    def _table(self, H: int, W: int, box) -> Tuple[torch.Tensor, torch.Tensor]:
        """``[2][size][4]`` tap indices (int16) and weights (fp32) of one crop box, y then x, from ``mra_video_crop_table``."""
        top, left, bh, bw = (int(b) for b in box)
        if not (0 <= top and 0 < bh and top + bh <= H and 0 <= left and 0 < bw and left + bw <= W):
            raise ValueError(f"box {(top, left, bh, bw)} does not lie inside the {H} x {W} frame")
        key = (top, left, bh, bw)
        hit = self._tables.get(key)
        if hit is None:
            lib, S = self._lib, int(self.image_size)
            idx, w = torch.empty(2, S, 4, dtype=torch.int16), torch.empty(2, S, 4, dtype=torch.float32)
            lib.check(lib.lib().mra_video_crop_table(bh, top, S, lib.ptr(idx[0]), lib.ptr(w[0])), "mra_video_crop_table")
            lib.check(lib.lib().mra_video_crop_table(bw, left, S, lib.ptr(idx[1]), lib.ptr(w[1])), "mra_video_crop_table")
            if len(self._tables) >= 64:
                self._tables.clear()
            hit = self._tables[key] = (idx, w)
        return hit

    def flat(self, clips, boxes=None, flips=None, lo: Optional[int] = None, hi: Optional[int] = None,
             out_dtype: torch.dtype = torch.float16) -> torch.Tensor:
        """Items ``[lo, hi)`` of the sample-major ``B * n_frms`` frames of ``clips`` (``[B, T, H, W, 3]`` uint8, or a list of ``[T_b, H_b,
        W_b, 3]``; a clip shorter than ``n_frms`` repeats its last frame) as ``[hi - lo, 3, S, S]`` on the device, what the encoder
        reads: only the source frames those items need are uploaded, as bytes, and ONE launch crops, resizes, flips and normalises them.
        ``boxes`` (per clip ``(top, left, height, width)``, None: whole frames) and ``flips`` (per clip) are the clip-wide augmentation."""
        if self.device is None:
            raise RuntimeError("flat() / batch() run on the HIP front end: construct the processor with a CUDA device")
        import ctypes as C

        from .. import _lib
        self._lib = lib = _lib
        if out_dtype not in (torch.float32, torch.float16):
            raise ValueError("out_dtype: torch.float32 or torch.float16")
        clips = list(clips.unbind(0)) if isinstance(clips, torch.Tensor) else [torch.as_tensor(c) for c in clips]
        T, S, B = int(self.n_frms), int(self.image_size), len(clips)
        lo, hi = (0 if lo is None else int(lo)), (B * T if hi is None else int(hi))
        if not 0 <= lo <= max(hi, lo) <= B * T:
            raise ValueError(f"items [{lo}, {hi}) outside the {B} x {T} frames of the step")
        out = torch.empty(max(hi - lo, 0), 3, S, S, dtype=out_dtype, device=self.device)
        if hi <= lo:
            return out
        used = range(lo // T, (hi - 1) // T + 1)          # only the clips that own an item of the block are touched
        parts, rows, idx_t, w_t, base = [], [], [], [], 0
        for n, r in enumerate(used):
            clip = clips[r]
            if clip.dtype != torch.uint8 or clip.dim() != 4 or clip.shape[-1] != 3 or clip.shape[0] < 1:
                raise ValueError(f"a clip is uint8 [T, H, W, 3], got {clip.dtype} {list(clip.shape)}")
            n_src, H, W = int(clip.shape[0]), int(clip.shape[1]), int(clip.shape[2])
            box = whole_frame_box(H, W) if boxes is None else [int(b) for b in boxes[r]]
            flip = 0 if flips is None else int(bool(flips[r]))
            idx, w = self._table(H, W, box)
            idx_t.append(idx)
            w_t.append(w)
            first, last = max(lo - r * T, 0), min(hi - r * T, T) - 1       # the clip's items of the block
            f0, f1 = min(first, n_src - 1), min(last, n_src - 1)           # ... and the source frames under them
            parts.append((base, clip[f0: f1 + 1]))
            for i in range(first, last + 1):
                rows.append((base + (min(i, n_src - 1) - f0) * H * W * 3, H, W, n, flip))
            base += (f1 - f0 + 1) * H * W * 3
        mean = (C.c_float * 3)(*(self.mean if self.mean is not None else MEAN))
        std = (C.c_float * 3)(*(self.std if self.std is not None else STD))
        with torch.cuda.device(self.device):
            src = torch.empty(base, dtype=torch.uint8, device=self.device)
            for at, part in parts:
                src[at: at + part.numel()].copy_(part.reshape(-1), non_blocking=True)
            rows_d = torch.tensor(rows, dtype=torch.int64).to(self.device)
            idx_d, w_d = torch.stack(idx_t).to(self.device), torch.stack(w_t).to(self.device)
            lib.check(lib.lib().mra_video_frames_forward(lib.ptr(src), base, lib.ptr(rows_d), len(rows), lib.ptr(idx_d), lib.ptr(w_d), len(idx_t), S,
                                                         mean, std, QUANTIZE[self.quantize], lib.ptr(out), lib.mra_dtype(out_dtype),
                                                         lib.current_stream()), "mra_video_frames_forward")
        return out

    def batch(self, clips, boxes=None, flips=None, out_dtype: torch.dtype = torch.float16) -> torch.Tensor:
        """All clips of a step in one launch: ``[B, 3, n_frms, S, S]`` on the device, a view of ``flat``'s sample-major frames."""
        S = int(self.image_size)
        return self.flat(clips, boxes, flips, out_dtype=out_dtype).view(len(clips), int(self.n_frms), 3, S, S).permute(0, 2, 1, 3, 4)


class AlproVideoEvalProcessor_Stamps(_StampsProcessor):
    """Reference ``:64-85``: uniform sampling, returns ``(frames [C,T,H,W] float32, indices, fps)``."""
    sampling = "uniform"


class AlproVideoTrainProcessor_Stamps(_StampsProcessor):
    """Reference ``:40-62``: one random frame per interval.  ``augment=True`` (opt-in) applies the reference's training transform: one
    random resized crop (area share in ``[min_scale, max_scale]``, bicubic) and one random horizontal flip per clip, then ``ToUint8``
    (``quantize="floor"``; ``"none"`` skips it), ``/ 255`` and the normalisation -- on the host in float64 (``preprocess_frames_ref``), or
    on the device with ``device=``.  ``rng`` (a ``random.Random``) makes the frame sampling and the draws reproducible.  Without
    ``augment`` the output is what it always was: the normalised decoded frames."""
    sampling = "random"

    def __init__(self, image_size=224, mean=None, std=None, min_scale=0.9, max_scale=1.0, n_frms=60, full_video=True, reader=None,
                 augment: bool = False, rng: Optional[rnd.Random] = None, quantize: str = "floor", device=None):
        super().__init__(image_size=image_size, mean=mean, std=std, n_frms=n_frms, full_video=full_video, reader=reader, device=device)
        self.min_scale, self.max_scale = min_scale, max_scale
        if quantize not in QUANTIZE:
            raise ValueError(f"quantize: 'floor' or 'none', got {quantize!r}")
        self.augment, self.rng = bool(augment), rng
        self.quantize = quantize if self.augment else "none"

    def _draw(self, H: int, W: int):
        if not self.augment:
            return super()._draw(H, W)
        box = random_resized_crop_params(H, W, (self.min_scale, self.max_scale), rng=self.rng)
        return box, random_flip(self.rng)

    def _host(self, sel) -> torch.Tensor:
        if not self.augment:
            return super()._host(sel)
        box, flip = self._draw(int(sel.shape[1]), int(sel.shape[2]))
        out = preprocess_frames_ref(sel, box, flip, int(self.image_size), self.mean, self.std, self.quantize)
        return out.permute(1, 0, 2, 3).to(torch.float32)      # (C, T, S, S)
