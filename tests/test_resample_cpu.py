"""Band-limited resampling (``resample_sinc`` / ``resample_table``, ``mra_resample_*``, ``csrc/resample.hip``), the part that needs
no GPU: the dense definition against the sparse per-phase form the kernel uses, the behaviour on pure tones (and the aliasing of the
linear route, the reason the feature exists), the fp32 emulation of the kernel inside the derived bound of
``tests/resample_cases.py`` with every named mutant outside it, the host processor, and the argument checks of the C ABI.
torchaudio is absent: parity with it is unpinned; what is pinned is the published algorithm in two independent forms."""
import ctypes as C
import math

import pytest
import torch

from resample_cases import MUTANTS, RATE_OUT, RATES, emulate, launches, pack, reference
from mraudio_amd import _lib
from mraudio_amd.processors.audio_processors import BeatsAudioProcessor, resample_out_samples, resample_sinc, resample_table


def _sparse(x, rate):
    """``resample_table`` evaluated in float64: every output as the dot product of its phase's non-zero taps."""
    orig, new, first, coef, taps = resample_table(rate, RATE_OUT)
    n = x.numel()
    m = torch.arange(resample_out_samples(rate, RATE_OUT, n))
    i, j = m % new, m // new
    idx = (j * orig + first[i])[:, None] + torch.arange(coef.shape[1])[None, :]
    ok = (idx >= 0) & (idx < n)
    return (torch.where(ok, x[idx.clamp(0, n - 1)], torch.zeros((), dtype=torch.float64)) * coef[i]).sum(dim=1), taps


@pytest.mark.parametrize("rate", RATES)
def test_dense_and_sparse_forms_agree(rate):
    g = torch.Generator().manual_seed(rate)
    x = torch.randn(20011, generator=g, dtype=torch.float64)
    dense = resample_sinc(x, rate, RATE_OUT)
    sparse, taps = _sparse(x, rate)
    orig, new = rate // math.gcd(rate, RATE_OUT), RATE_OUT // math.gcd(rate, RATE_OUT)
    assert dense.dtype == torch.float64 and dense.shape == sparse.shape == (-(-new * x.numel() // orig),)
    d = (dense - sparse).abs().max().item()
    print(f"{rate} -> {RATE_OUT}: dense against sparse max|d| {d:.3e}, non-zero taps per phase <= {int(taps.max())}")
    assert d <= 1e-11 * x.abs().max().item()
    assert int(taps.max()) == {48000: 37, 44100: 34, 32000: 25, 22050: 17, 8000: 13}[rate]
    # [C, n] is the channel mean resampled
    st = torch.randn(3, 4001, generator=g, dtype=torch.float64)
    assert torch.equal(resample_sinc(st, rate, RATE_OUT), resample_sinc(st.mean(dim=0), rate, RATE_OUT))


def test_equal_rates_return_the_input_and_lengths_follow_the_formula():
    x = torch.randn(1234, dtype=torch.float64)
    assert torch.equal(resample_sinc(x, 16000, 16000), x)
    assert torch.equal(resample_sinc(x.float(), 32000, 32000), x.float().double())
    for rate in RATES:
        for n in (0, 1, 2, 10, 441, 4410):
            assert resample_sinc(torch.zeros(n), rate, RATE_OUT).numel() == resample_out_samples(rate, RATE_OUT, n)
    with pytest.raises(ValueError):
        resample_sinc(x, 0, 16000)


def _gain(y, cut):
    return (y[cut:-cut].pow(2).mean().sqrt() * math.sqrt(2.0)).item()      # RMS gain of a unit-amplitude tone, edges cut


@pytest.mark.parametrize("rate", [48000, 44100])
def test_tones_sinc_band_limits_and_linear_aliases(rate):
    t = torch.arange(rate // 2, dtype=torch.float64) / rate                 # half a second
    tone = lambda f: torch.sin(2.0 * math.pi * f * t)
    lin = BeatsAudioProcessor()
    g1, g11 = _gain(resample_sinc(tone(1000.0), rate, RATE_OUT), 400), _gain(resample_sinc(tone(11000.0), rate, RATE_OUT), 400)
    l11 = _gain(lin._resample(tone(11000.0).float(), rate).double(), 400)
    print(f"{rate} Hz: sinc gain at 1 kHz {g1:.4f}, at 11 kHz {g11:.4f}; linear at 11 kHz {l11:.4f}")
    assert abs(g1 - 1.0) <= 1e-3
    assert g11 <= 0.01
    assert l11 >= 0.5                                                      # linear interpolation folds 11 kHz into the band


@pytest.mark.parametrize("rate", RATES)
def test_fp32_emulation_of_the_kernel_is_inside_the_bound(rate):
    """If this fails the bound is not reachable by the kernel's arithmetic; if it passes and the GPU test fails, the kernel is wrong."""
    for name, clips in launches(rate).items():
        wave, rows, total = pack(clips, rate)
        got = emulate(wave, rows, total, rate).to(torch.float64)
        for w, (_, _, _, at, n_out, _) in zip(clips, rows.tolist()):
            want, bound = reference(w, rate)
            assert want.numel() == n_out
            d = (got[at: at + n_out] - want).abs()
            worst = (d / bound.clamp_min(1e-300)).max().item() if n_out else 0.0
            print(f"{rate}, {name}, clip of {tuple(w.shape)}: max |d| / bound {worst:.3f}")
            assert (d <= bound).all(), (rate, name, worst)


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_mutant_lands_outside_the_bound(mutant):
    """The bound is tight enough to see each of these mistakes somewhere in the case table (a phase shift needs more than one
    phase, a channel sum a stereo clip, a neighbour's samples a neighbour: not every launch can show every one)."""
    outside = 0
    for rate in RATES:
        for name, clips in launches(rate).items():
            wave, rows, total = pack(clips, rate)
            got = emulate(wave, rows, total, rate, mutant=mutant).to(torch.float64)
            for w, (_, _, _, at, n_out, _) in zip(clips, rows.tolist()):
                want, bound = reference(w, rate)
                outside += int(((got[at: at + n_out] - want).abs() > bound).sum())
    print(f"{mutant}: {outside} outputs outside the bound")
    assert outside > 0


def test_host_processor_modes():
    g = torch.Generator().manual_seed(5)
    wave = (torch.randn(2, 48000, generator=g) * 0.2).clamp(-1, 1)           # one second, stereo, 48 kHz
    proc = BeatsAudioProcessor(n_frames=2, frame_length=64, reader=lambda p: (wave, 48000), resample="sinc")
    got = proc("clip")
    y = resample_sinc(wave, 48000, 16000)
    assert y.numel() == 16000
    want = torch.stack([proc.features(y[a: a + n]) for a, n in proc.segments(y.numel())])
    assert got.shape == (2, 64, 128) and torch.equal(got, want)
    # the default is today's route, bit for bit: linear interpolation of the flattened waveform on the host
    mono = wave[0]
    default = BeatsAudioProcessor(n_frames=2, frame_length=64, reader=lambda p: (mono, 48000))
    assert default.resample == "linear"
    n_out = int(round(mono.numel() * 16000 / 48000))
    lin = torch.nn.functional.interpolate(mono.view(1, 1, -1), size=n_out, mode="linear", align_corners=False).view(-1)
    edges = torch.linspace(0, lin.numel(), 3).long().tolist()
    assert torch.equal(default("clip"), torch.stack([default.features(lin[a:b]) for a, b in zip(edges[:-1], edges[1:])]))
    with pytest.raises(ValueError):
        BeatsAudioProcessor(resample="cubic")


def test_abi_without_compute():
    lib = _lib.lib()
    for rate in (8000, 11025, 22050, 44100, 48000, 96000, 16000):
        g = math.gcd(rate, 16000)
        orig, new = rate // g, 16000 // g
        for n in (0, 1, 2, 3, 440, 441, 442, 479999, 480000, 2 ** 40 + 1):
            assert lib.mra_resample_out_samples(rate, 16000, n) == -(-new * n // orig), (rate, n)
    assert lib.mra_resample_out_samples(0, 16000, 100) == 0 and lib.mra_resample_out_samples(48000, -1, 100) == 0
    assert lib.mra_resample_out_samples(48000, 16000, -5) == 0
    h = C.c_void_p()
    assert lib.mra_resample_create(0, 16000, C.byref(h)) == -1 and not h.value
    assert b"> 0" in lib.mra_last_error()
    assert lib.mra_resample_create(48000, 16000, None) == -1
    assert b"null" in lib.mra_last_error()
    assert lib.mra_resample_create(48000, 47999, C.byref(h)) == -1 and not h.value      # 47 999 phases
    assert b"limit is 1024" in lib.mra_last_error()
    assert lib.mra_resample_create(2000000, 16000, C.byref(h)) == -1 and not h.value     # 1 501 taps per phase
    assert b"limit is 256" in lib.mra_last_error()
    buf = (C.c_float * 8)()
    rows = (C.c_int64 * 6)(0, 4, 1, 0, 2, 0)
    assert lib.mra_resample_forward(None, buf, 4, rows, 1, buf, 2, None) == -1
    assert b"null handle" in lib.mra_last_error()
    assert lib.mra_resample_flops(None, 100) == 0.0
    lib.mra_resample_destroy(None)      # a null handle is a no-op
