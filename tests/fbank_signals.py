"""Shared by tests/test_fbank_host.py and tests/test_gpu_fbank.py (not a test module): the seeded test signals of the filterbank
front end, the parity bar, and an fp32 restatement of the arithmetic ``csrc/fbank.hip`` is built in (the FOLDED form: DC removal,
pre-emphasis and window composed into the transform table in float64 and rounded to fp32 once; the product reads raw samples)."""
import math

import torch

from mraudio_amd.processors.audio_processors import FBANK_MEAN, FBANK_STD, mel_banks

SR = 16000
# Derived, not measured: BEATs rounds this input to f16 for its patch GEMM, the normalised values lie mostly in [-2, 2], and
# 2^-11 is half an f16 ulp in [1, 2): an error below it is smaller than the rounding the consumer applies anyway.
BAR = 2.0 ** -11


def signals(seconds: float = 5.0):
    """name -> waveform fp32 [seconds * 16 kHz] in [-1, 1]; every one has a noise floor (see the docstring of the GPU test)."""
    n = int(seconds * SR)
    t = torch.arange(n, dtype=torch.float64) / SR
    g = torch.Generator().manual_seed(20240607)
    noise = lambda: torch.randn(n, generator=g, dtype=torch.float64)
    env = 0.05 + 0.95 * (0.5 - 0.5 * torch.cos(2 * math.pi * 3.0 * t))
    out = {
        "white noise at 0.1": 0.1 * noise(),
        "syllable-like + DC offset": env * (0.03 * noise() + 0.01 * torch.sin(2 * math.pi * 180.0 * t)) + 0.015,
        "440 Hz tone + noise at -60 dB": 0.25 * torch.sin(2 * math.pi * 440.0 * t) + 0.25e-3 * noise(),
        "chirp 100-7100 Hz + noise at -50 dB": 0.2 * torch.sin(2 * math.pi * (100.0 * t + 0.5 * (7000.0 / seconds) * t * t)) + 0.2 * 10 ** -2.5 * noise(),
        "white noise at 1e-4": 1e-4 * noise(),
    }
    return {k: v.clamp(-1.0, 1.0).to(torch.float32) for k, v in out.items()}


def folded_table() -> torch.Tensor:
    """float64 [400, 512]: (I - 11^T / 400) . P_0.97 . diag(povey) . [cos | -sin] of bins 0..255, acting on a ROW of raw samples."""
    win, nfft = 400, 512
    n = torch.arange(win, dtype=torch.float64)
    w = (0.5 - 0.5 * torch.cos(2.0 * math.pi * n / (win - 1))) ** 0.85
    ang = 2.0 * math.pi * ((n.long()[:, None] * torch.arange(nfft // 2)[None, :]) % nfft).to(torch.float64) / nfft
    T = torch.cat([torch.cos(ang), -torch.sin(ang)], dim=1) * w[:, None]
    M = T.clone()
    M[0] *= 0.03                      # y[0] = x[0] - 0.97 x[0]
    M[:-1] -= 0.97 * T[1:]            # x[n] feeds y[n + 1] with -0.97
    return M - M.mean(dim=0, keepdim=True)


def emulate_folded(segment: torch.Tensor, frame_length: int) -> torch.Tensor:
    """The kernel's arithmetic in plain fp32 torch: fp32 frames of raw samples x 2^15, fp32 table product, fp32 power and mel sums."""
    x = segment.reshape(-1).to(torch.float32) * 32768.0
    out = torch.zeros(frame_length, 128)
    if x.numel() < 400:
        return out
    frames = x.unfold(0, 400, 160)[:frame_length]
    spec = frames @ folded_table().to(torch.float32)
    power = spec[:, :256] ** 2 + spec[:, 256:] ** 2
    e = power @ mel_banks(128, 512, float(SR)).to(torch.float32).t()
    fb = torch.log(torch.clamp(e, min=torch.finfo(torch.float32).eps))
    out[: fb.shape[0]] = (fb - FBANK_MEAN) / (2.0 * FBANK_STD)
    return out
