"""Audio processor with the call signature the reference uses (``evaluate.py:24``, ``utils/trainer.py:46``):
``BeatsAudioProcessor(model_name, sampling_rate, n_frames, is_eval, frame_length)(path) -> Tensor[T, F, 128]``
-- T temporal positions of F = ``frame_length`` filterbank frames with 128 mel bins, the input the BEATs encoder
(row A1) patches into 16 x 16 tokens (512 x 128 -> 256 tokens per position).

The reference takes this class from the third-party ``salesforce-lavis`` package (unpinned, absent offline), which in
turn calls ``torchaudio.compliance.kaldi.fbank`` (absent too).  What is restated here is the PUBLISHED algorithm of that
call with the arguments BEATs uses (``num_mel_bins=128, sample_frequency=16000, frame_length=25, frame_shift=10``;
Kaldi defaults otherwise: no dither, DC-offset removal, 0.97 pre-emphasis, povey window, 512-point FFT, power
spectrum, mel banks from 20 Hz to Nyquist, log with a float-epsilon floor, ``snip_edges``) followed by BEATs'
normalisation ``(x - 15.41663) / (2 * 6.55582)``.  Neither package can be imported here and the reference holds no
audio fixtures: **parity unpinned**; ``tests/test_audio_processor.py`` checks the implementation against a direct
(DFT-by-definition) restatement and against analytic properties.  Decoding the audio track of an ``.mp4`` is IO outside
the path: pass ``reader(path) -> (waveform float tensor [samples] in [-1, 1], sample_rate)``.

``BeatsAudioProcessor(device=None)`` is this host arithmetic in float64 and stays the definition.  With a CUDA ``device`` the
same filterbank is computed on the GPU by ``mra_fbank_forward`` (``csrc/fbank.hip``: fp32 throughout, one launch for all
temporal positions of all clips) and stays there for the encoder; ``tests/test_gpu_fbank.py`` holds it to the host processor.

Resampling.  ``resample="linear"`` (the default, unchanged) interpolates linearly on the host: it does not band-limit, so at 48 kHz
everything between 8 and 24 kHz folds into the band BEATs sees.  ``resample="sinc"`` is what LAVIS' processor does, torchaudio's
windowed-sinc ``resample`` (Hann window, ``lowpass_filter_width=6``, ``rolloff=0.99``), restated from the published algorithm in
two independent forms -- ``resample_sinc`` (dense, float64: the definition) and ``resample_table`` (the sparse per-phase taps the
kernel uses); torchaudio itself is absent, so **parity unpinned** here too (``tests/test_resample_cpu.py`` holds the two forms to
each other and to the behaviour on pure tones).  On a device processor ``"sinc"`` runs on the GPU (``mra_resample_forward``,
``csrc/resample.hip``): waveforms go up at their native rate and channel count and the 16 kHz buffer stays on the device.
"""
from __future__ import annotations

import math
import numbers
from typing import Callable, List, Optional, Sequence, Tuple

import torch

FBANK_MEAN, FBANK_STD = 15.41663, 6.55582      # BEATs' dataset statistics (its preprocess())


def _mel(f):
    return 1127.0 * math.log(1.0 + f / 700.0)


def mel_banks(num_bins: int, padded_window: int, sample_rate: float, low_freq: float = 20.0, high_freq: float = 0.0) -> torch.Tensor:
    """Kaldi's triangular mel filters: ``[num_bins, padded_window // 2]`` (the Nyquist bin carries no weight)."""
    nyquist = 0.5 * sample_rate
    if high_freq <= 0.0:
        high_freq += nyquist
    n_fft_bins = padded_window // 2
    fft_bin_width = sample_rate / padded_window
    mel_lo, mel_hi = _mel(low_freq), _mel(high_freq)
    delta = (mel_hi - mel_lo) / (num_bins + 1)
    b = torch.arange(num_bins, dtype=torch.float64).unsqueeze(1)
    left, center, right = mel_lo + b * delta, mel_lo + (b + 1.0) * delta, mel_lo + (b + 2.0) * delta
    mel = 1127.0 * torch.log(1.0 + fft_bin_width * torch.arange(n_fft_bins, dtype=torch.float64) / 700.0).unsqueeze(0)
    up, down = (mel - left) / (center - left), (right - mel) / (right - center)
    return torch.clamp(torch.minimum(up, down), min=0.0)


def kaldi_fbank(waveform: torch.Tensor, num_mel_bins: int = 128, sample_frequency: float = 16000.0, frame_length: float = 25.0,
                frame_shift: float = 10.0, preemphasis: float = 0.97, low_freq: float = 20.0, high_freq: float = 0.0) -> torch.Tensor:
    """Log mel filterbank energies ``[frames, num_mel_bins]`` of a mono waveform ``[samples]`` (Kaldi ``compute-fbank-feats``
    conventions as exposed by ``torchaudio.compliance.kaldi.fbank`` with its defaults)."""
    x = waveform.reshape(-1).to(torch.float64)
    win = int(sample_frequency * frame_length * 0.001)
    shift = int(sample_frequency * frame_shift * 0.001)
    padded = 1 << (win - 1).bit_length()                      # round_to_power_of_two
    if x.numel() < win:
        return torch.zeros(0, num_mel_bins)
    n_frames = 1 + (x.numel() - win) // shift                 # snip_edges
    frames = x.unfold(0, win, shift)[:n_frames].clone()       # [frames, win]
    frames = frames - frames.mean(dim=1, keepdim=True)        # remove_dc_offset
    if preemphasis != 0.0:                                    # x[i] -= c * x[i - 1], the first sample against itself
        prev = torch.cat([frames[:, :1], frames[:, :-1]], dim=1)
        frames = frames - preemphasis * prev
    n = torch.arange(win, dtype=torch.float64)
    window = (0.5 - 0.5 * torch.cos(2.0 * math.pi * n / (win - 1))) ** 0.85      # povey
    frames = frames * window
    spec = torch.fft.rfft(frames, n=padded, dim=1)
    power = spec.real ** 2 + spec.imag ** 2                   # [frames, padded / 2 + 1]
    banks = mel_banks(num_mel_bins, padded, sample_frequency, low_freq, high_freq)
    energies = power[:, : padded // 2] @ banks.t()
    return torch.log(torch.clamp(energies, min=torch.finfo(torch.float32).eps)).to(torch.float32)

RESAMPLE_LPW, RESAMPLE_ROLLOFF = 6, 0.99       # torchaudio.functional.resample's defaults (sinc_interp_hann)


def _reduced_rates(rate_in: int, rate_out: int) -> Tuple[int, int]:
    rate_in, rate_out = int(rate_in), int(rate_out)
    if rate_in <= 0 or rate_out <= 0:
        raise ValueError(f"sample rates must be > 0, got {rate_in} -> {rate_out}")
    g = math.gcd(rate_in, rate_out)
    return rate_in // g, rate_out // g


def resample_out_samples(rate_in: int, rate_out: int, n_in: int) -> int:
    """``ceil(new * n_in / orig)``: the length ``resample_sinc`` gives ``n_in`` samples."""
    orig, new = _reduced_rates(rate_in, rate_out)
    return -(-new * int(n_in) // orig)


def _windowed_sinc(t: torch.Tensor, lpw: int, scale: float) -> torch.Tensor:
    """``sinc(pi t) cos^2(pi t / (2 lpw)) scale`` with ``t`` clamped to ``[-lpw, lpw]`` (the Hann window ends there: zero beyond)."""
    t = t.clamp(-lpw, lpw)
    window = torch.cos(t * math.pi / lpw / 2.0) ** 2
    a = t * math.pi
    return torch.where(a == 0, torch.ones_like(a), torch.sin(a) / a) * window * scale


def _mono64(wave) -> torch.Tensor:
    x = torch.as_tensor(wave).to(torch.float64)
    if x.dim() == 2:
        return x.mean(dim=0)
    if x.dim() != 1:
        raise ValueError(f"a waveform is [samples] or [channels, samples], got {list(x.shape)}")
    return x


def resample_sinc(wave, rate_in: int, rate_out: int, lowpass_filter_width: int = RESAMPLE_LPW, rolloff: float = RESAMPLE_ROLLOFF) -> torch.Tensor:
    """Band-limited resampling, float64 ``[ceil(new * n / orig)]``: the published windowed-sinc algorithm of
    ``torchaudio.functional.resample`` in its DENSE form -- one kernel row of ``2 width + orig`` taps per output phase, the input
    zero-padded by ``(width, width + orig)`` and correlated at stride ``orig``.  ``wave`` is ``[n]``, or ``[C, n]`` with the channels
    averaged first; equal rates return the (mono) input unchanged.  This is the definition the sparse form and the GPU are held to."""
    x = _mono64(wave)
    orig, new = _reduced_rates(rate_in, rate_out)
    if orig == new:
        return x
    lpw = int(lowpass_filter_width)
    base = min(orig, new) * float(rolloff)
    width = math.ceil(lpw * orig / base)
    k = torch.arange(-width, width + orig, dtype=torch.float64)
    i = torch.arange(new, dtype=torch.float64)
    c = _windowed_sinc((-i[:, None] / new + k[None, :] / orig) * base, lpw, base / orig)       # [new, 2 width + orig]
    n = x.numel()
    padded = torch.nn.functional.pad(x, (width, width + orig))
    y = torch.nn.functional.conv1d(padded.view(1, 1, -1), c.unsqueeze(1), stride=orig)[0]      # [new, n // orig + 1]
    return y.t().reshape(-1)[: -(-new * n // orig)]


def resample_table(rate_in: int, rate_out: int, lowpass_filter_width: int = RESAMPLE_LPW, rolloff: float = RESAMPLE_ROLLOFF):
    """The SPARSE form of ``resample_sinc``, the one ``csrc/resample.hip`` builds: ``(orig, new, first [new] int64, coef [new, K]
    float64, taps [new] int64)``.  Output sample ``j * new + i`` is ``sum_k coef[i][k] x[j * orig + first[i] + k]`` over
    ``k < taps[i]`` (rows are zero-padded to ``K = max taps``): only the input samples within ``lpw * orig / base`` of the phase's
    centre ``j * orig + i * orig / new`` carry weight, the window being zero beyond.  Equal rates: the identity."""
    orig, new = _reduced_rates(rate_in, rate_out)
    if orig == new:
        return 1, 1, torch.zeros(1, dtype=torch.int64), torch.ones(1, 1, dtype=torch.float64), torch.ones(1, dtype=torch.int64)
    lpw = int(lowpass_filter_width)
    base = min(orig, new) * float(rolloff)
    reach = lpw * orig / base
    first, rows = [], []
    for i in range(new):
        centre = i * orig / new
        k0, k1 = math.ceil(centre - reach), math.floor(centre + reach)
        k = torch.arange(k0, k1 + 1, dtype=torch.float64)
        first.append(k0)
        rows.append(_windowed_sinc((-float(i) / new + k / orig) * base, lpw, base / orig))
    coef = torch.zeros(new, max(r.numel() for r in rows), dtype=torch.float64)
    for i, r in enumerate(rows):
        coef[i, : r.numel()] = r
    return orig, new, torch.tensor(first, dtype=torch.int64), coef, torch.tensor([r.numel() for r in rows], dtype=torch.int64)


class BeatsAudioProcessor:
    def __init__(self, model_name: str = "iter3", sampling_rate: int = 16000, n_frames: int = 2, is_eval: bool = False,
                 frame_length: int = 512, reader: Optional[Callable[[str], Tuple[torch.Tensor, int]]] = None,
                 device=None, out_dtype: torch.dtype = torch.float32, resample: str = "linear"):
        if resample not in ("linear", "sinc"):
            raise ValueError(f"resample: 'linear' (host interpolation, no anti-alias filter) or 'sinc' (band-limited), got {resample!r}")
        self.resample = resample
        self._resamplers = {}                  # input rate -> mra_resample handle (device processor with resample="sinc")
        self.model_name, self.sampling_rate, self.n_frames, self.is_eval, self.frame_length = model_name, sampling_rate, n_frames, is_eval, frame_length
        self.reader = reader
        self.device = torch.device(device) if device is not None else None
        self.out_dtype = out_dtype
        self._handle = None
        if self.device is not None:
            if self.device.type != "cuda":
                raise ValueError("device: None (the float64 host processor) or a CUDA device (the HIP front end)")
            if int(sampling_rate) != 16000:
                raise ValueError("the HIP front end is built for BEATs' 16 kHz input")
            if out_dtype not in (torch.float32, torch.float16):
                raise ValueError("out_dtype: torch.float32 or torch.float16")

    def __del__(self):
        try:
            for h in self._resamplers.values():
                self._lib.lib().mra_resample_destroy(h)
            self._resamplers = {}
            if self._handle:
                self._lib.lib().mra_fbank_destroy(self._handle)
                self._handle = None
        except Exception:
            pass

    def _fbank(self):
        """The ``mra_fbank`` handle of this processor's device (tables built and uploaded on first use)."""
        if self._handle is None:
            import ctypes as C

            from .. import _lib
            self._lib = _lib
            h = C.c_void_p()
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().mra_fbank_create(C.byref(h)), "mra_fbank_create")
            self._handle = h
        return self._handle

    def _resampler(self, rate: int):
        """The ``mra_resample`` handle of one input rate (tap table built and uploaded on first use, kept for the processor's life)."""
        h = self._resamplers.get(rate)
        if h is None:
            import ctypes as C

            self._fbank()
            h = C.c_void_p()
            with torch.cuda.device(self.device):
                self._lib.check(self._lib.lib().mra_resample_create(int(rate), int(self.sampling_rate), C.byref(h)), "mra_resample_create")
            self._resamplers[rate] = h
        return h

    def _rates(self, rates, n: int) -> Optional[List[int]]:
        """``rates`` as one int per clip; None when every clip is already at ``sampling_rate`` (today's path, no extra launch)."""
        if rates is None:
            return None
        if self.resample != "sinc":
            raise ValueError('rates= needs a processor built with resample="sinc" (the device resampler)')
        if isinstance(rates, torch.Tensor):
            rates = rates.tolist()
        rates = [int(rates)] * n if isinstance(rates, numbers.Integral) else [int(r) for r in rates]
        if len(rates) != n:
            raise ValueError(f"rates: an int or one int per clip ({n}), got {len(rates)}")
        if any(r <= 0 for r in rates):
            raise ValueError(f"rates must be > 0, got {rates}")
        return None if all(r == self.sampling_rate for r in rates) else rates

    def segments(self, n_samples: int) -> List[Tuple[int, int]]:
        """(first sample, number of samples) of the ``n_frames`` temporal positions: equal windows over the clip."""
        edges = torch.linspace(0, n_samples, self.n_frames + 1).long().tolist()
        return [(a, b - a) for a, b in zip(edges[:-1], edges[1:])]

    def flat(self, waves: Sequence[torch.Tensor], lo: Optional[int] = None, hi: Optional[int] = None,
             out_dtype: Optional[torch.dtype] = None, rates=None) -> torch.Tensor:
        """Items ``[lo, hi)`` of the sample-major ``B * n_frames`` positions of ``waves`` (16 kHz mono, [-1, 1]) as
        ``[hi - lo, frame_length, 128]`` on the device: one concatenated sample buffer, one segment table, ONE launch.
        ``rates`` (an int or one int per clip; needs ``resample="sinc"``): a clip at another rate goes up as it is, ``[n]`` or
        ``[C, n]``, and one ``mra_resample_forward`` per distinct rate writes its band-limited 16 kHz mono samples into that buffer."""
        if self.device is None:
            raise RuntimeError("flat() / batch() run on the HIP front end: construct the processor with a CUDA device")
        rates = self._rates(rates, len(waves))
        if rates is not None:
            return self._flat_resampled(waves, rates, lo, hi, out_dtype)
        h = self._fbank()
        lib = self._lib
        T = self.n_frames
        lo, hi = (0 if lo is None else int(lo)), (len(waves) * T if hi is None else int(hi))
        dt = self.out_dtype if out_dtype is None else out_dtype
        out = torch.empty(max(hi - lo, 0), self.frame_length, 128, dtype=dt, device=self.device)
        if hi <= lo:
            return out
        clips = range(lo // T, (hi - 1) // T + 1)          # only the clips that own an item of the block are uploaded
        parts, segs, base = [], [], 0
        for r in clips:
            w = torch.as_tensor(waves[r]).reshape(-1)
            parts.append(w.to(device=self.device, dtype=torch.float32))
            for i, (a, n) in enumerate(self.segments(w.numel())):
                if lo <= r * T + i < hi:
                    segs.append((base + a, n))
            base += w.numel()
        wave = torch.cat(parts) if len(parts) > 1 else parts[0].contiguous()
        if wave.numel() == 0:
            wave = torch.zeros(1, dtype=torch.float32, device=self.device)
        seg_t = torch.tensor(segs, dtype=torch.int64).to(self.device)
        with torch.cuda.device(self.device):
            lib.check(lib.lib().mra_fbank_forward(h, lib.ptr(wave), base, lib.ptr(seg_t), len(segs), self.frame_length, lib.ptr(out),
                                                  lib.mra_dtype(dt), lib.current_stream()), "mra_fbank_forward")
        return out

    def _flat_resampled(self, waves, rates: List[int], lo, hi, out_dtype) -> torch.Tensor:
        """``flat`` with clips at other rates: the step's 16 kHz buffer is filled on the device, by a copy for the clips already at
        16 kHz and by one resampling launch per distinct input rate for the others, and read by the filterbank launch in place."""
        h = self._fbank()
        lib = self._lib
        T, sr = self.n_frames, self.sampling_rate
        lo, hi = (0 if lo is None else int(lo)), (len(waves) * T if hi is None else int(hi))
        dt = self.out_dtype if out_dtype is None else out_dtype
        out = torch.empty(max(hi - lo, 0), self.frame_length, 128, dtype=dt, device=self.device)
        if hi <= lo:
            return out
        segs, base, same, groups = [], 0, [], {}
        for r in range(lo // T, (hi - 1) // T + 1):       # only the clips that own an item of the block are uploaded
            w = torch.as_tensor(waves[r])
            if rates[r] == sr:
                w = w.reshape(-1)
                n16 = w.numel()
                same.append((base, w))
            else:
                if w.dim() not in (1, 2):
                    raise ValueError(f"a waveform is [samples] or [channels, samples], got {list(w.shape)}")
                w = w.reshape(-1, w.shape[-1])
                n16 = int(lib.lib().mra_resample_out_samples(rates[r], sr, w.shape[1]))
                groups.setdefault(rates[r], []).append((base, n16, w))
            for i, (a, n) in enumerate(self.segments(n16)):
                if lo <= r * T + i < hi:
                    segs.append((base + a, n))
            base += n16
        wave = torch.empty(max(base, 1), dtype=torch.float32, device=self.device)
        if base == 0:
            wave.zero_()
        for at, w in same:
            wave[at: at + w.numel()].copy_(w)
        with torch.cuda.device(self.device):
            for rate, clips in groups.items():
                parts, rows, first, block = [], [], 0, 0
                for at, n16, w in clips:
                    parts.append(w.reshape(-1).to(device=self.device, dtype=torch.float32))
                    rows.append((first, w.shape[1], w.shape[0], at, n16, block))
                    first += w.numel()
                    block += -(-n16 // 1024)                # the kernel's workgroups own 1024 output samples
                raw = torch.cat(parts) if len(parts) > 1 else parts[0].contiguous()
                if raw.numel() == 0:
                    raw = torch.zeros(1, dtype=torch.float32, device=self.device)
                row_t = torch.tensor(rows, dtype=torch.int64).to(self.device)
                lib.check(lib.lib().mra_resample_forward(self._resampler(rate), lib.ptr(raw), first, lib.ptr(row_t), len(rows), lib.ptr(wave),
                                                         base, lib.current_stream()), "mra_resample_forward")
            seg_t = torch.tensor(segs, dtype=torch.int64).to(self.device)
            lib.check(lib.lib().mra_fbank_forward(h, lib.ptr(wave), base, lib.ptr(seg_t), len(segs), self.frame_length, lib.ptr(out),
                                                  lib.mra_dtype(dt), lib.current_stream()), "mra_fbank_forward")
        return out

    def batch(self, waves: Sequence[torch.Tensor], out_dtype: Optional[torch.dtype] = None, rates=None) -> torch.Tensor:
        """All clips of a step in one launch: ``[B, n_frames, frame_length, 128]`` on the device (``rates``: see ``flat``)."""
        return self.flat(waves, out_dtype=out_dtype, rates=rates).view(len(waves), self.n_frames, self.frame_length, 128)

    def resample_flops(self, rate: int, total_out: int) -> float:
        return float(self._lib.lib().mra_resample_flops(self._resampler(int(rate)), int(total_out)))

    def flops(self, n_seg: int) -> float:
        h = self._fbank()
        return float(self._lib.lib().mra_fbank_flops(h, int(n_seg), int(self.frame_length)))

    def _resample(self, wav: torch.Tensor, sr: int) -> torch.Tensor:
        if sr == self.sampling_rate:
            return wav
        n_out = int(round(wav.numel() * self.sampling_rate / sr))             # linear interpolation; IO-side convenience
        return torch.nn.functional.interpolate(wav.view(1, 1, -1), size=n_out, mode="linear", align_corners=False).view(-1)

    def features(self, segment: torch.Tensor) -> torch.Tensor:
        """One temporal position: ``[frame_length, 128]`` normalised filterbank frames (zero-padded or cut at the end)."""
        fb = kaldi_fbank(segment * (1 << 15), num_mel_bins=128, sample_frequency=self.sampling_rate)
        fb = (fb - FBANK_MEAN) / (2.0 * FBANK_STD)
        out = torch.zeros(self.frame_length, 128)
        k = min(self.frame_length, fb.shape[0])
        out[:k] = fb[:k]
        return out

    def __call__(self, path) -> torch.Tensor:
        if self.reader is None:
            raise RuntimeError("no audio reader configured (decoding is not part of this build); pass reader=")
        wav, sr = self.reader(path)
        if self.resample == "sinc":
            wav = torch.as_tensor(wav, dtype=torch.float32)
            if int(sr) == self.sampling_rate and wav.dim() == 2:
                wav = wav.mean(dim=0)      # nothing to resample: only the downmix is left
            if self.device is not None:  # uploaded at its own rate and channel count; resampled and filtered on the device
                return self.batch([wav], rates=[int(sr)])[0]
            wav = resample_sinc(wav, int(sr), self.sampling_rate)
        else:
            wav = self._resample(torch.as_tensor(wav, dtype=torch.float32).reshape(-1), int(sr))
        if self.device is not None:      # the waveform is uploaded once; the filterbank is computed and stays on the device
            return self.batch([wav])[0]
        # n_frames equal windows over the clip, one per temporal position (the video processor samples its frames the same way)
        edges = torch.linspace(0, wav.numel(), self.n_frames + 1).long().tolist()
        return torch.stack([self.features(wav[a:b]) for a, b in zip(edges[:-1], edges[1:])])
