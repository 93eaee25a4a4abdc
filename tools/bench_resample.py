"""Times the band-limited resampler (``mra_resample_forward``, csrc/resample.hip) at a step's size -- 32 clips x 10 s stereo at 48 kHz
and at 44.1 kHz -- prints one JSON line and writes it to ``--out`` (default profiles/resample_line.json).  One box, one session;
device events around the calls, median of ``--reps`` ALTERNATING repetitions after a warm-up.  Per input rate:
  resample_ms / gb_s     the resampling launch alone and its rate on the algorithmic bytes 4 (C n_in + n_out) per clip
  fbank_ms / both_ms     the filterbank launch alone on the 16 kHz buffer against resampling + filterbank back to back
  step_*_ms              the whole step from host waveforms, host clock around a device synchronise: the device route (upload at the
                         native rate, resample, filterbank) against the host linear route (channel mean + ``_resample`` on 16 threads,
                         upload at 16 kHz, filterbank)
  host_sinc_ms           ``resample_sinc`` (float64, 16 threads) over the same clips, median of 3
For rocprofv3:
    rocprofv3 --kernel-trace --stats -d prof_resample -- python3 tools/bench_resample.py --reps 3 --no-host"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mraudio_amd.processors.audio_processors import BeatsAudioProcessor, resample_out_samples, resample_sinc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--clips", type=int, default=32)
ap.add_argument("--seconds", type=float, default=10.0)
ap.add_argument("--rates", default="48000,44100")
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_line.json"))
a = ap.parse_args()
dev = torch.device("cuda:0")
torch.set_num_threads(16)
T, F, CH = 2, 512, 2


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


res = {"metric": "resample_front_end", "clips": a.clips, "seconds": a.seconds, "channels": CH, "host_threads": torch.get_num_threads(),
       "reps": a.reps, "peak_hbm_tb_s": 8.0}
for rate in [int(v) for v in a.rates.split(",")]:
    g = torch.Generator().manual_seed(rate)
    n_in = int(a.seconds * rate)
    waves = [(torch.randn(CH, n_in, generator=g) * 0.1).clamp(-1, 1) for _ in range(a.clips)]
    proc = BeatsAudioProcessor(n_frames=T, frame_length=F, device=dev, out_dtype=torch.float16, resample="sinc")
    plain = BeatsAudioProcessor(n_frames=T, frame_length=F, device=dev, out_dtype=torch.float16)
    host = BeatsAudioProcessor(n_frames=T, frame_length=F)
    hf, hr, lib = proc._fbank(), proc._resampler(rate), proc._lib
    n16 = resample_out_samples(rate, 16000, n_in)
    raw = torch.cat([w.reshape(-1) for w in waves]).to(dev)
    rows = torch.tensor([[i * CH * n_in, n_in, CH, i * n16, n16, i * (-(-n16 // 1024))] for i in range(a.clips)], dtype=torch.int64).to(dev)
    wave16 = torch.zeros(a.clips * n16, dtype=torch.float32, device=dev)
    segs = torch.tensor([(i * n16 + s, n) for i in range(a.clips) for s, n in proc.segments(n16)], dtype=torch.int64).to(dev)
    out = torch.empty(a.clips * T, F, 128, dtype=torch.float16, device=dev)

    def resample():
        lib.check(lib.lib().mra_resample_forward(hr, lib.ptr(raw), raw.numel(), lib.ptr(rows), a.clips, lib.ptr(wave16), wave16.numel(),
                                                 lib.current_stream()), "mra_resample_forward")

    def fbank():
        lib.check(lib.lib().mra_fbank_forward(hf, lib.ptr(wave16), wave16.numel(), lib.ptr(segs), a.clips * T, F, lib.ptr(out), lib.MRA_F16,
                                              lib.current_stream()), "mra_fbank_forward")

    def both():
        resample()
        fbank()

    def step_device():
        proc.batch(waves, rates=rate)

    def step_host_linear():
        plain.batch([host._resample(w.mean(dim=0), rate) for w in waves])

    for _ in range(a.warmup):
        both()
        step_device()
    t = {"resample": [], "fbank": [], "both": [], "step_device": [], "step_host_linear": []}
    for _ in range(a.reps):                      # alternating, same session
        t["resample"].append(event_ms(resample))
        t["fbank"].append(event_ms(fbank))
        t["both"].append(event_ms(both))
        t["step_device"].append(wall_ms(step_device))
        if not a.no_host:
            t["step_host_linear"].append(wall_ms(step_host_linear))
    nbytes = 4.0 * a.clips * (CH * n_in + n16)
    ms = median(t["resample"])
    r = {"resample_ms": round(ms, 4), "resample_ms_best": round(min(t["resample"]), 4), "algorithmic_mb": round(nbytes / 1e6, 1),
         "gb_s": round(nbytes / ms / 1e6, 1), "gflop": round(proc.resample_flops(rate, a.clips * n16) / 1e9, 3),
         "fbank_ms": round(median(t["fbank"]), 4), "both_ms": round(median(t["both"]), 4), "step_device_ms": round(median(t["step_device"]), 3)}
    if not a.no_host:
        r["step_host_linear_ms"] = round(median(t["step_host_linear"]), 3)
        hs = []
        for _ in range(3):
            t0 = time.perf_counter()
            for w in waves:
                resample_sinc(w, rate, 16000)
            hs.append((time.perf_counter() - t0) * 1e3)
        r["host_sinc_ms"] = round(median(hs), 1)
    res[str(rate)] = r
    del raw, wave16, out, proc, plain
    torch.cuda.empty_cache()
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
