"""Band-limited resampling on the GPU (``mra_resample_forward``, ``csrc/resample.hip``): the kernel alone against the float64
definition ``resample_sinc`` under the derived bound of ``tests/resample_cases.py`` (every element, sentinel guards either side of
the output), the device ``BeatsAudioProcessor(resample="sinc")`` against the host route, and the model end to end."""
import ctypes as C

import pytest
import torch

from fbank_signals import BAR
from resample_cases import RATE_OUT, RATES, emulate, launches, pack, reference
from mraudio_amd import _lib
from mraudio_amd.processors.audio_processors import BeatsAudioProcessor, resample_sinc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                       # floats either side of both buffers (a multiple of 4: the input keeps its 16-byte alignment)
SENTINEL = -12345.0


def _launch(handle, wave, rows, total_out, in_offset=GUARD):
    """One ``mra_resample_forward`` over host arguments: the input sits ``in_offset`` floats into an allocation filled with NaN,
    the output between two guards of SENTINEL.  Returns the ``total_out`` outputs (host) after checking the guards."""
    lib = _lib.lib()
    total_in = wave.numel()
    src = torch.full((total_in + in_offset + GUARD,), float("nan"), device=DEV)
    src[in_offset: in_offset + total_in] = wave.to(DEV)
    dst = torch.full((total_out + 2 * GUARD,), SENTINEL, device=DEV)
    rows_d = rows.to(DEV)
    _lib.check(lib.mra_resample_forward(handle, C.c_void_p(src.data_ptr() + 4 * in_offset), total_in, _lib.ptr(rows_d), rows.shape[0],
                                        C.c_void_p(dst.data_ptr() + 4 * GUARD), total_out, _lib.current_stream()), "mra_resample_forward")
    torch.cuda.synchronize()
    dst = dst.cpu()
    assert (dst[:GUARD] == SENTINEL).all() and (dst[GUARD + total_out:] == SENTINEL).all(), "a write outside [0, total_out)"
    return dst[GUARD: GUARD + total_out]


@pytest.mark.parametrize("rate", RATES)
def test_kernel_against_float64_under_the_bound(rate):
    lib = _lib.lib()
    h = C.c_void_p()
    with torch.cuda.device(DEV):
        _lib.check(lib.mra_resample_create(rate, RATE_OUT, C.byref(h)), "mra_resample_create")
    try:
        for name, clips in launches(rate).items():
            wave, rows, total = pack(clips, rate)
            got = _launch(h, wave, rows, total)
            assert torch.isfinite(got).all(), (rate, name)          # no NaN of the input guards was read
            for w, (_, _, _, at, n_out, _) in zip(clips, rows.tolist()):
                want, bound = reference(w, rate)
                d = (got[at: at + n_out].to(torch.float64) - want).abs()
                worst = (d / bound.clamp_min(1e-300)).max().item() if n_out else 0.0
                print(f"{rate}, {name}, clip of {tuple(w.shape)}: max |d| / bound {worst:.3f}, max |d| {d.max().item() if n_out else 0.0:.3e}")
                assert (d <= bound).all(), (rate, name, worst)
            if len(clips) > 1:
                for w, (_, _, _, at, n_out, _) in zip(clips, rows.tolist()):    # a clip does not depend on its neighbours
                    w1, r1, t1 = pack([w], rate)
                    assert torch.equal(_launch(h, w1, r1, t1), got[at: at + n_out]), (rate, tuple(w.shape))
                # an input that is not 16-byte aligned takes the scalar loads: the same bits
                assert torch.equal(_launch(h, wave, rows, total, in_offset=GUARD + 1), got)
        assert lib.mra_resample_forward(h, None, 0, None, 0, None, 0, None) == 0          # n_clip == 0: a no-op
        assert lib.mra_resample_forward(h, None, 4, None, -1, None, 4, None) == -1
        assert lib.mra_resample_flops(h, 1000) > 0.0
    finally:
        lib.mra_resample_destroy(h)


def _step_waves():
    """Three clips of a step at their own rates: 48 kHz stereo, 44.1 kHz mono, 16 kHz mono; all carry a noise floor."""
    g = torch.Generator().manual_seed(77)
    t = lambda n, sr: torch.arange(n, dtype=torch.float64) / sr
    a = 0.1 * torch.randn(2, 96000, generator=g, dtype=torch.float64)
    a[0] += 0.2 * torch.sin(2 * torch.pi * 440.0 * t(96000, 48000))
    a[1] += 0.2 * torch.sin(2 * torch.pi * 11000.0 * t(96000, 48000))          # above the 8 kHz band: must not fold into it
    b = 0.05 * torch.randn(70001, generator=g, dtype=torch.float64) + 0.2 * torch.sin(2 * torch.pi * 3000.0 * t(70001, 44100))
    c = 0.1 * torch.randn(30000, generator=g, dtype=torch.float64)
    return [w.clamp(-1, 1).to(torch.float32) for w in (a, b, c)], [48000, 44100, 16000]


def test_device_processor_against_the_host_route():
    waves, rates = _step_waves()
    T, F = 2, 100
    host = BeatsAudioProcessor(n_frames=T, frame_length=F)
    feats = lambda y: torch.stack([host.features(y[a: a + n]) for a, n in host.segments(y.numel())])
    want, share = [], 0.0
    for w, r in zip(waves, rates):
        y = resample_sinc(w, r, RATE_OUT)
        want.append(feats(y))
        if r != RATE_OUT:     # the resampler's own share of the error: its fp32 arithmetic (CPU emulation) through the float64 filterbank
            wave, rows, total = pack([w.reshape(-1, w.shape[-1])], r)
            share = max(share, (feats(emulate(wave, rows, total, r).to(torch.float64)) - want[-1]).abs().max().item())
    want = torch.stack(want)
    bar = BAR + 2.0 * share
    gpu = BeatsAudioProcessor(n_frames=T, frame_length=F, device=DEV, resample="sinc")
    got = gpu.batch(waves, rates=rates)
    assert got.is_cuda and got.shape == want.shape == (3, T, F, 128)
    d = (got.cpu() - want).abs().max().item()
    print(f"device sinc processor against the host route: max|d| {d:.3e}; bar {bar:.3e} = filterbank {BAR:.3e} + 2 x resampler share {share:.3e}")
    assert d <= bar
    assert torch.equal(got.cpu() == 0, want == 0)
    # items [lo, hi) of the sample-major order are the same rows; __call__ takes the reader's waveform as it is
    assert torch.equal(gpu.flat(waves, 1, 5, rates=rates), got.view(3 * T, F, 128)[1:5])
    one = BeatsAudioProcessor(n_frames=T, frame_length=F, device=DEV, resample="sinc", reader=lambda p: (waves[0], 48000))
    assert torch.equal(one("clip"), got[0])
    # without other rates nothing changes: no extra launch, the same bits as a processor built as before
    plain = BeatsAudioProcessor(n_frames=T, frame_length=F, device=DEV)
    mono = [waves[2], waves[1][:20000]]
    base = plain.batch(mono)
    assert torch.equal(gpu.batch(mono), base) and torch.equal(gpu.batch(mono, rates=16000), base)
    with pytest.raises(ValueError, match='resample="sinc"'):
        plain.batch(waves, rates=rates)


def test_end_to_end_native_rate_waveforms_against_host_sinc_filterbanks():
    from mraudio_amd.models.xinstructblip import XInstructBLIP

    g = torch.Generator().manual_seed(78)
    n = 4 * 48000
    t = torch.arange(n, dtype=torch.float64) / 48000
    env = 0.05 + 0.95 * (0.5 - 0.5 * torch.cos(2 * torch.pi * 3.0 * t))
    waves = [(env * 0.05 * torch.randn(2, n, generator=g, dtype=torch.float64) + 0.015).to(torch.float32),
             (0.1 * torch.randn(2, 150000, generator=g, dtype=torch.float64)).to(torch.float32)]
    T, F = 4, 96
    proc = BeatsAudioProcessor(n_frames=T, frame_length=F, device=DEV, resample="sinc")
    model = XInstructBLIP(seed=0, perturb=True, device=DEV, modalities=["audio"], audio_encoder="beats", audio_processor=proc)
    host = BeatsAudioProcessor(n_frames=T, frame_length=F)
    ys = [resample_sinc(w, 48000, RATE_OUT) for w in waves]
    fb = torch.stack([torch.stack([host.features(y[a: a + k]) for a, k in host.segments(y.numel())]) for y in ys])
    base = {"text_input": ["Query: a dog barks.\nRelevant windows: ", "Query: someone speaks.\nRelevant windows: "],
            "timestamps": [[0, 1, 2, 3]] * 2, "duration": [4, 4]}
    a = model.encode_fuse({**base, "audio_wave": waves, "audio_wave_rate": 48000})
    b = model.encode_fuse({**base, "audio": fb})
    torch.cuda.synchronize()
    d = (a["fused"] - b["fused"]).abs().max().item()
    print(f"end to end, 48 kHz stereo waveform against host sinc filterbank: max|d fused logit| {d:.3e}")
    assert a["fused"].shape == (2 * T,) and d <= 1e-3
    assert torch.equal(a["spans"], b["spans"])
