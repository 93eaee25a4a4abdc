"""Times the audio front end (``mra_fbank_forward``, csrc/fbank.hip: waveform -> normalised filterbank) at the step's size and prints
one JSON line: the HIP time at 1024 segments x 5.12 s (frame_length 512; 32 clips x 32 positions) and 32 x 9.92 s (992), device
events around the call, median and best after a warm-up; the float64 host processor on the same input (16 threads, median of 3 on a
BOUNDED SAMPLE of segments, scaled up to the full count: stated as such in the line); and, unless ``--no-beats``, the front end +
``mra_beats_forward`` back to back against the BEATs encode alone, alternating in one session.
For rocprofv3:
    rocprofv3 --kernel-trace --stats -d prof_fbank -- python3 tools/bench_fbank.py --reps 3 --no-host --no-beats"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mraudio_amd.processors.audio_processors import BeatsAudioProcessor  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--host-segments", type=int, default=8, help="segments the host processor is timed on (scaled up to the full count)")
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--no-beats", action="store_true")
ap.add_argument("--shapes", default="1024x512,32x992", help="comma-separated SEGMENTSxFRAME_LENGTH")
a = ap.parse_args()
dev = torch.device("cuda:0")
torch.set_num_threads(16)


def timed(fn, reps=None, warmup=None):
    for _ in range(a.warmup if warmup is None else warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps or a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], ms[0]


res = {"metric": "fbank_front_end", "peak_f32_mfma_tflops": 157.3, "host_threads": torch.get_num_threads()}
for n_seg, F in [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]:
    per = (F - 1) * 160 + 400 + 80          # samples per segment: exactly F frames (5.12 s / 9.92 s of audio and the window's overhang)
    g = torch.Generator().manual_seed(1)
    wave_h = (torch.randn(n_seg * per, generator=g) * 0.1).clamp(-1, 1)
    proc = BeatsAudioProcessor(n_frames=n_seg, frame_length=F, device=dev, out_dtype=torch.float16)
    h = proc._fbank()
    lib = proc._lib
    wave = wave_h.to(dev)
    segs = torch.tensor(proc.segments(wave_h.numel()), dtype=torch.int64).to(dev)
    out = torch.empty(n_seg, F, 128, dtype=torch.float16, device=dev)

    def front():
        lib.check(lib.lib().mra_fbank_forward(h, lib.ptr(wave), wave.numel(), lib.ptr(segs), n_seg, F, lib.ptr(out), lib.MRA_F16, lib.current_stream()),
                  "mra_fbank_forward")

    med, best = timed(front)
    flops = proc.flops(n_seg)
    r = {"ms": round(med, 3), "ms_best": round(best, 3), "gflop": round(flops / 1e9, 1), "tflops": round(flops / med / 1e9, 1),
         "frac_peak": round(flops / med / 1e9 / 157.3, 3), "samples_mb": round(wave.numel() * 4 / 1e6, 1)}
    if not a.no_host:
        host = BeatsAudioProcessor(n_frames=n_seg, frame_length=F)
        k = min(a.host_segments, n_seg)
        s0, n = host.segments(wave_h.numel())[0]
        host.features(wave_h[s0: s0 + n])       # warm-up: thread pool, FFT plan
        hs = []
        for _ in range(3):
            t0 = time.perf_counter()
            for s0, n in host.segments(wave_h.numel())[:k]:
                host.features(wave_h[s0: s0 + n])
            hs.append((time.perf_counter() - t0) * 1e3)
        hs.sort()
        r.update({"host_ms_scaled": round(hs[1] * n_seg / k, 1), "host_segments_timed": k, "host_ms_per_segment": round(hs[1] / k, 3),
                  "speedup_vs_host": round(hs[1] * n_seg / k / med, 1)})
    if not a.no_beats:
        from mraudio_amd.models.beats import HipBEATs
        enc = HipBEATs(device=dev).eval().init_seeded_(0)
        front()
        fb = out.clone()

        def both():
            front()
            enc(out)

        timed(both, reps=1, warmup=1)
        pairs = [(timed(lambda: enc(fb), reps=1, warmup=0)[0], timed(both, reps=1, warmup=0)[0]) for _ in range(max(5, a.reps))]   # alternating, same session
        alone, joint = sorted(p[0] for p in pairs), sorted(p[1] for p in pairs)
        r.update({"beats_alone_ms": round(alone[len(alone) // 2], 3), "fbank_plus_beats_ms": round(joint[len(joint) // 2], 3)})
        del enc, fb
    res[f"{n_seg}x{F}"] = r
    del wave, out
    torch.cuda.empty_cache()
print(json.dumps(res))
