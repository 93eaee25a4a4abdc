"""Shared by tests/test_resample_cpu.py and tests/test_gpu_resample.py (not a test module): the case table of the resampling
kernel (``csrc/resample.hip``), its float64 reference, the derived error bound, and an fp32 restatement of the kernel's arithmetic
(fp32 table, ascending fma chain over the taps, channel sum times 1 / C) with the named mutants the bound has to reject.

Bound (derived, not measured).  An output is K fp32 fma steps over K non-zero taps whose coefficients were rounded to fp32 once:
``|y - y64| <= (K + 2) 2^-24 sum_k |c_k x_k|`` (K roundings of the running sum, each at most 2^-24 of a partial sum that never
exceeds ``sum |c x|``, one for the coefficients, one spare for the second-order terms), ``y64`` being the float64 DENSE definition
``resample_sinc`` on the fp32 input.  A C-channel downmix adds ``(C + 1) 2^-24 mean_c |x_c|`` per input sample (C - 1 additions, the
reciprocal and the product), which reaches the output through ``sum_k |c_k|`` of it."""
import torch

from mraudio_amd.processors.audio_processors import resample_out_samples, resample_sinc, resample_table

RATE_OUT = 16000
RATES = (48000, 44100, 32000, 22050, 8000)
BLOCK = 1024                     # output samples per workgroup of the kernel
U = 2.0 ** -24
MUTANTS = ("phase row off by one", "centre not advanced by orig", "scale base / orig missing", "last tap dropped",
           "channels summed", "neighbour's samples read")


def length_for(rate: int, n_out: int) -> int:
    """The shortest clip whose output has at least ``n_out`` samples (8 kHz doubles: its lengths are even)."""
    n = n_out * rate // RATE_OUT
    while resample_out_samples(rate, RATE_OUT, n) < n_out:
        n += 1
    while n > 0 and resample_out_samples(rate, RATE_OUT, n - 1) >= n_out:
        n -= 1
    return n


def launches(rate: int):
    """name -> list of clips ``[C, n]`` fp32 of ONE launch at ``rate``.  Lengths 0, 1, 10 (shorter than half the filter), one block
    of outputs and one block -+ 1, 2.5 blocks; unit-variance noise; one clip whose last 64 samples are 1.0 (a wrong zero extension
    at the edge shows); and one launch of three clips of different lengths with 1 / 2 / 1 channels."""
    g = torch.Generator().manual_seed(1000 + rate)
    noise = lambda c, n: torch.randn(c, n, generator=g, dtype=torch.float32)
    out = {}
    for n_out in (BLOCK - 1, BLOCK, BLOCK + 1, BLOCK * 5 // 2):
        out[f"{n_out} outputs"] = [noise(1, length_for(rate, n_out))]
    for n in (0, 1, 10):
        out[f"{n} samples"] = [noise(1, n)]
    tail = noise(1, length_for(rate, BLOCK + 40))
    tail[:, -64:] = 1.0
    out["last 64 samples 1.0"] = [tail]
    out["three clips, 1 / 2 / 1 channels"] = [noise(1, length_for(rate, BLOCK + 300)), noise(2, length_for(rate, BLOCK * 2 + 7)), noise(1, 777)]
    return out


def pack(clips, rate: int, guard: int = 0):
    """The launch's arguments as the processor builds them: the concatenated planes, the int64 clip rows {first input sample,
    samples per channel, channels, first output sample, output samples, first workgroup}, and the total output length.  ``guard``
    output samples are left free in front of the first clip (and are to be allocated behind the last)."""
    rows, first, at, block = [], 0, guard, 0
    for w in clips:
        n16 = resample_out_samples(rate, RATE_OUT, w.shape[1])
        rows.append([first, w.shape[1], w.shape[0], at, n16, block])
        first += w.numel()
        at += n16
        block += -(-n16 // BLOCK)
    return torch.cat([w.reshape(-1) for w in clips]), torch.tensor(rows, dtype=torch.int64).reshape(-1, 6), at + guard


def reference(w: torch.Tensor, rate: int):
    """float64 definition of one clip ``[C, n]`` and the bound of every output: ``(y64 [n_out], bound [n_out])``."""
    y = resample_sinc(w, rate, RATE_OUT)
    orig, new, first, coef, taps = resample_table(rate, RATE_OUT)
    c32 = coef.to(torch.float32).to(torch.float64)
    C, n = w.shape
    x = w.to(torch.float64)
    mono_abs = x.mean(dim=0).abs()                     # |downmixed sample|
    down = (C + 1) * U * x.abs().mean(dim=0) if C > 1 else torch.zeros(n, dtype=torch.float64)
    m = torch.arange(y.numel())
    i, j = m % new, m // new
    idx = (j * orig + first[i])[:, None] + torch.arange(coef.shape[1])[None, :]
    ok = (idx >= 0) & (idx < n)
    take = lambda v: torch.where(ok, v[idx.clamp(0, max(n - 1, 0))], torch.zeros((), dtype=torch.float64)) if n else torch.zeros(idx.shape, dtype=torch.float64)
    ca = c32[i].abs()
    k = (c32[i] != 0).sum(dim=1).to(torch.float64)
    bound = (k + 2.0) * U * (ca * take(mono_abs)).sum(dim=1) + (ca * take(down)).sum(dim=1)
    return y, bound


def emulate(wave: torch.Tensor, rows: torch.Tensor, total_out: int, rate: int, mutant=None) -> torch.Tensor:
    """The kernel's arithmetic in fp32 on the launch's own arguments: ``out [total_out]`` (zero where no clip writes).  The fma is
    formed as the float64 sum of the exact float64 product rounded to fp32 (it can differ from a true fma by the last bit on a
    tie of the intermediate rounding, 2^-53 relative: nothing to the bound).  ``mutant``: one of ``MUTANTS``."""
    assert mutant is None or mutant in MUTANTS
    orig, new, first, coef, taps = resample_table(rate, RATE_OUT)
    if mutant == "scale base / orig missing":
        coef = coef / (min(orig, new) * 0.99 / orig)
    c32 = coef.to(torch.float32)
    if mutant == "last tap dropped":
        c32[torch.arange(new), taps - 1] = 0.0
    K = c32.shape[1]
    out = torch.zeros(total_out, dtype=torch.float32)
    total_in = wave.numel()
    for first_in, n, C, at, n_out, _ in rows.tolist():
        if n_out == 0:
            continue
        m = torch.arange(n_out)
        i, j = m % new, m // new
        step = orig - 1 if mutant == "centre not advanced by orig" else orig
        idx = (j * step + first[i])[:, None] + torch.arange(K)[None, :]          # clip-relative input sample of every tap
        inside = (idx >= 0) & (idx < n)
        x = torch.zeros(idx.shape, dtype=torch.float32)
        for c in range(C):                                                       # the downmix: channel sum in order, times 1 / C
            a = first_in + c * n + idx
            if mutant == "neighbour's samples read":
                ok = (a >= 0) & (a < total_in)
            else:
                ok = inside
            v = torch.where(ok, wave[a.clamp(0, max(total_in - 1, 0))], torch.zeros(())) if total_in else torch.zeros(idx.shape)
            x = v if c == 0 else x + v
        if C > 1 and mutant != "channels summed":
            x = x * torch.tensor(1.0, dtype=torch.float32).div(float(C))
        ci = c32[(i + 1) % new] if mutant == "phase row off by one" else c32[i]
        acc = torch.zeros(n_out, dtype=torch.float32)
        for k in range(K):                                                       # ascending fma chain
            acc = (acc.to(torch.float64) + ci[:, k].to(torch.float64) * x[:, k].to(torch.float64)).to(torch.float32)
        out[at: at + n_out] = acc
    return out
