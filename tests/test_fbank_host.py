"""Audio front end (``mra_fbank_*``, ``csrc/fbank.hip``), the part that needs no GPU: argument checks of the C ABI, the host
processor unchanged by the new ``device`` argument, and the CPU check that the parity bar of ``tests/test_gpu_fbank.py`` is
reachable by fp32 arithmetic in the form the kernel is built in (folded table, see ``tests/fbank_signals.py``)."""
import ctypes as C

import pytest
import torch

from fbank_signals import BAR, emulate_folded, signals
from mraudio_amd import _lib
from mraudio_amd.processors.audio_processors import FBANK_MEAN, FBANK_STD, BeatsAudioProcessor, kaldi_fbank


def test_fbank_bad_arguments_are_rejected_before_touching_the_gpu():
    lib = _lib.lib()
    assert lib.mra_fbank_create(None) == -1
    assert b"null" in lib.mra_last_error()
    buf = (C.c_float * 4)()
    seg = (C.c_int64 * 2)(0, 4)
    assert lib.mra_fbank_forward(None, buf, 4, seg, 1, 8, buf, _lib.MRA_F32, None) == -1
    assert b"null handle" in lib.mra_last_error()
    for bad in (_lib.MRA_BF16, 7, -1):
        assert lib.mra_fbank_forward(None, buf, 4, seg, 1, 8, buf, bad, None) == -1
        assert b"out_dtype" in lib.mra_last_error()
    assert lib.mra_fbank_flops(None, 4, 512) == 0.0
    lib.mra_fbank_destroy(None)      # a null handle is a no-op


def test_host_processor_is_unchanged_by_the_device_argument():
    g = torch.Generator().manual_seed(3)
    wave = (torch.randn(16000 * 3, generator=g) * 0.2).clamp(-1, 1)
    proc = BeatsAudioProcessor(n_frames=4, frame_length=96, reader=lambda p: (wave, 16000))
    assert proc.device is None
    got = proc("clip")
    assert got.dtype == torch.float32 and got.device.type == "cpu" and got.shape == (4, 96, 128)
    edges = torch.linspace(0, wave.numel(), 5).long().tolist()
    for i, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        fb = (kaldi_fbank(wave[a:b] * (1 << 15), num_mel_bins=128, sample_frequency=16000) - FBANK_MEAN) / (2.0 * FBANK_STD)
        want = torch.zeros(96, 128)
        k = min(96, fb.shape[0])
        want[:k] = fb[:k]
        assert torch.equal(got[i], want)
        assert proc.segments(wave.numel())[i] == (a, b - a)
    with pytest.raises(ValueError):
        BeatsAudioProcessor(device="cpu")
    with pytest.raises(RuntimeError):
        proc.batch([wave])


def test_fp32_emulation_of_the_folded_form_is_inside_the_bar():
    """If this fails the bar is not reachable by fp32 in this form; if it passes and the GPU test fails, the kernel is wrong."""
    host = BeatsAudioProcessor(n_frames=1, frame_length=512)
    for name, w in signals().items():
        want = host.features(w)
        got = emulate_folded(w, 512)
        d = (got - want).abs().max().item()
        print(f"fp32 folded emulation, {name}: max|d| {d:.3e} (bar {BAR:.3e})")
        assert d <= BAR, (name, d)
    z = emulate_folded(torch.zeros(16000), 512)
    assert torch.equal(z[:98], host.features(torch.zeros(16000))[:98])
