"""Times the BEATs audio encode stage (row A1 / N4, the audio half) on the HIP extension and, beside it, the fp32 torch restatement
run under fp16 autocast on the same GPU (stock PyTorch: rocBLAS / hipBLASLt GEMMs, cuDNN-free conv1d); prints one JSON line.
Shapes: 1024 chunks x 512 frames (the reference step's audio, 32 clips x 32 positions; S = 256 tokens) and 32 x 992 frames (S = 496).
For rocprofv3:
    rocprofv3 --kernel-trace --stats -d prof_beats -- python3 tools/bench_beats.py --reps 2 --no-torch"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mraudio_amd.models.beats import BEATs, HipBEATs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=4)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--no-torch", action="store_true", help="HIP encoder only (profiler runs)")
ap.add_argument("--shapes", default="1024x512,32x992", help="comma-separated NxFRAMES")
a = ap.parse_args()
dev = torch.device("cuda:0")
shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]


def timed(fn, x):
    with torch.no_grad():
        for _ in range(a.warmup):
            fn(x)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(x)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], ms[0]


hip = HipBEATs(device=dev).eval().init_seeded_(0)
ref = None
if not a.no_torch:
    ref = BEATs().eval().init_seeded_(0).to(dev)

    def torch_fp16(x):
        with torch.autocast("cuda", dtype=torch.float16):
            return ref(x)

res = {"metric": "beats_encode", "peak_f16_tflops": 2500.0}
for n, frames in shapes:
    x = torch.randn(n, frames, 128, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    flops = hip.flops(n, frames)
    key = f"{n}x{frames}"
    med, best = timed(hip, x)
    r = {"ms": round(med, 3), "ms_best": round(best, 3), "tflops": round(flops / med / 1e9, 1), "gflop": round(flops / 1e9, 1),
         "frac_peak": round(flops / med / 1e9 / 2500.0, 3)}
    if ref is not None:
        tmed, tbest = timed(torch_fp16, x)
        r.update({"torch_fp16_ms": round(tmed, 3), "torch_fp16_tflops": round(flops / tmed / 1e9, 1), "speedup": round(tmed / med, 2)})
    res[key] = r
    del x
    torch.cuda.empty_cache()
print(json.dumps(res))
