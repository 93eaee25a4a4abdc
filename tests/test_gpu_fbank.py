"""Audio front end on the GPU (``mra_fbank_forward``, ``csrc/fbank.hip``) through ``BeatsAudioProcessor(device="cuda")``, held to
the float64 host processor ``BeatsAudioProcessor()``.

Bar: max |d| <= 2^-11 = 4.9e-4 in the normalised units of the output, NO element left out.  Derived, not measured: BEATs rounds
this input to f16 for its patch GEMM, the normalised values lie mostly in [-2, 2], and 2^-11 is half an f16 ulp in [1, 2).  The
signals all carry a noise floor; a noiseless pure tone is not among them because its far bands sit > 100 dB under the peak, where
fp32 itself is not within this bar of float64 (the kernel is fp32 by design: folded table, ``tests/fbank_signals.py``)."""
import ctypes as C
import math

import pytest
import torch

from fbank_signals import BAR, signals
from mraudio_amd import _lib
from mraudio_amd.processors.audio_processors import FBANK_MEAN, FBANK_STD, BeatsAudioProcessor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _pair(n_frames, frame_length, wave, **kw):
    host = BeatsAudioProcessor(n_frames=n_frames, frame_length=frame_length, reader=lambda p: (wave, 16000))
    gpu = BeatsAudioProcessor(n_frames=n_frames, frame_length=frame_length, reader=lambda p: (wave, 16000), device=DEV, **kw)
    return host, gpu


@pytest.mark.parametrize("n_frames", [1, 4, 32])
def test_parity_with_the_host_processor(n_frames):
    frame_length = {1: 512, 4: 160, 32: 16}[n_frames]     # 5 s: 498 frames in one position, 123 in each of 4, 14 in each of 32
    for name, w in signals().items():
        host, gpu = _pair(n_frames, frame_length, w)
        want = host("clip")
        got = gpu("clip")
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == want.shape == (n_frames, frame_length, 128)
        got = got.cpu()
        assert torch.isfinite(got).all()
        d = (got - want).abs().max().item()
        print(f"fbank parity, T = {n_frames}, {name}: max|d| {d:.3e} (bar {BAR:.3e})")
        assert d <= BAR, (name, n_frames, d)
        assert torch.equal(got == 0, want == 0)           # the zero tails are the same rows, exactly 0.0


def test_all_zero_samples_give_the_floor():
    host, gpu = _pair(2, 64, torch.zeros(16000))
    got = gpu("clip").cpu()
    floor = torch.tensor((math.log(torch.finfo(torch.float32).eps) - FBANK_MEAN) / (2.0 * FBANK_STD), dtype=torch.float32)
    ulp = 2.0 ** -22                                         # one fp32 ulp at |floor| = 2.39
    nfr = 1 + (8000 - 400) // 160
    assert (got[:, :nfr] - floor).abs().max().item() <= ulp
    assert (got[:, nfr:] == 0).all()
    assert (got - host("clip")).abs().max().item() <= ulp


def test_short_long_and_sub_window_positions():
    w = signals(2.0)["white noise at 0.1"]
    # shorter than frame_length frames: zero tail, exactly 0.0, across a workgroup's 128-frame boundary
    host, gpu = _pair(1, 512, w)
    want, got = host("c"), gpu("c").cpu()
    nfr = 1 + (w.numel() - 400) // 160
    assert nfr == 198 and (got[0, nfr:] == 0).all() and (got[0, :nfr] != 0).any(dim=1).all()
    assert (got - want).abs().max().item() <= BAR
    # longer: cut at frame_length (not a multiple of the workgroup's 128 frames)
    host, gpu = _pair(1, 150, w)
    want, got = host("c"), gpu("c").cpu()
    assert got.shape == (1, 150, 128) and (got - want).abs().max().item() <= BAR and (got[0, -1] != 0).any()
    # shorter than one window: no frame at all
    host, gpu = _pair(4, 32, w[:1500])
    want, got = host("c"), gpu("c").cpu()
    assert (want == 0).all() and (got == 0).all()


def test_f16_output_is_the_fp32_output_rounded_once():
    w = signals(2.0)["syllable-like + DC offset"]
    _, g32 = _pair(2, 128, w)
    _, g16 = _pair(2, 128, w, out_dtype=torch.float16)
    a, b = g32("c"), g16("c")
    assert b.dtype == torch.float16 and b.is_cuda
    assert torch.equal(a.to(torch.float16), b)


def test_batch_equals_the_single_calls():
    s = signals(3.0)
    waves = [s["white noise at 0.1"][:40000], s["syllable-like + DC offset"][:16001], s["440 Hz tone + noise at -60 dB"][:47999],
             s["white noise at 1e-4"][:1000]]
    gpu = BeatsAudioProcessor(n_frames=4, frame_length=96, device=DEV)
    both = gpu.batch(waves)
    assert both.shape == (4, 4, 96, 128) and both.is_cuda
    for i, w in enumerate(waves):
        assert torch.equal(both[i], gpu.batch([w])[0]), i
    # a block of items of the sample-major order (the clip-sharded path) is the same rows
    assert torch.equal(gpu.flat(waves, 3, 11), both.view(16, 96, 128)[3:11])


def test_a_segment_that_claims_too_many_samples_is_clipped():
    """An argument check of the kernel's bound, nothing is provoked: the claimed samples lie INSIDE the same allocation (allocated
    longer than total_samples, the tail filled with NaN), and no NaN may reach the output."""
    lib = _lib.lib()
    total, extra, F = 8000, 4000, 64
    w = signals(1.0)["white noise at 0.1"][:total]
    buf = torch.full((total + extra,), float("nan"), device=DEV)
    buf[:total] = w.to(DEV)
    segs = torch.tensor([[0, 4000], [4000, 4000 + extra], [-100, 2100], [total + 50, 500]], dtype=torch.int64, device=DEV)
    out = torch.full((4, F, 128), float("nan"), device=DEV)
    h = C.c_void_p()
    _lib.check(lib.mra_fbank_create(C.byref(h)), "mra_fbank_create")
    try:
        _lib.check(lib.mra_fbank_forward(h, _lib.ptr(buf), total, _lib.ptr(segs), 4, F, _lib.ptr(out), _lib.MRA_F32, _lib.current_stream()), "forward")
        torch.cuda.synchronize()
        assert lib.mra_fbank_forward(h, _lib.ptr(buf), total, _lib.ptr(segs), 0, F, None, _lib.MRA_F32, None) == 0      # n_seg == 0: a no-op
        assert lib.mra_fbank_forward(h, _lib.ptr(buf), total, _lib.ptr(segs), -1, F, _lib.ptr(out), _lib.MRA_F32, None) == -1
        assert lib.mra_fbank_flops(h, 1024, 512) > 2.0 * 400 * 512 * 1024 * 512
    finally:
        lib.mra_fbank_destroy(h)
    out = out.cpu()
    assert torch.isfinite(out).all()
    host = BeatsAudioProcessor(n_frames=1, frame_length=F)
    assert (out[0] - host.features(w[:4000])).abs().max().item() <= BAR
    assert (out[1] - host.features(w[4000:])).abs().max().item() <= BAR       # clipped to the 4000 samples that exist
    assert (out[2] - host.features(w[:2000])).abs().max().item() <= BAR       # a negative start is clipped to sample 0
    assert (out[3] == 0).all()                                                # entirely outside: no frame


def test_end_to_end_waveforms_against_host_filterbanks():
    from mraudio_amd.models.xinstructblip import XInstructBLIP

    s = signals(4.0)
    waves = [s["syllable-like + DC offset"], s["white noise at 0.1"][:50000]]
    T, F = 4, 96
    proc = BeatsAudioProcessor(n_frames=T, frame_length=F, device=DEV)
    model = XInstructBLIP(seed=0, perturb=True, device=DEV, modalities=["audio"], audio_encoder="beats", audio_processor=proc)
    host = BeatsAudioProcessor(n_frames=T, frame_length=F)
    fb = torch.stack([torch.stack([host.features(w[a:a + n]) for a, n in host.segments(w.numel())]) for w in waves])
    base = {"text_input": ["Query: a dog barks.\nRelevant windows: ", "Query: someone speaks.\nRelevant windows: "],
            "timestamps": [[0, 1, 2, 3]] * 2, "duration": [4, 4]}
    a = model.encode_fuse({**base, "audio_wave": waves})
    b = model.encode_fuse({**base, "audio": fb})
    torch.cuda.synchronize()
    d = (a["fused"] - b["fused"]).abs().max().item()
    print(f"end to end, waveform against host filterbank: max|d fused logit| {d:.3e}")
    assert a["fused"].shape == (2 * T,) and d <= 1e-3
    assert torch.equal(a["spans"], b["spans"])
