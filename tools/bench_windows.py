"""Times the ranked-window head (``mra_windows_from_logits``, csrc/windows.hip) and writes one JSON line (``--output``, default
``profiles/windows_line.json``; also printed): per shape ``(videos, clips, top_k, max_len)`` the median and best of repeated launches
between device events after a warm-up, the ``mra_span_from_logits`` launch at the same ``(videos, clips)``, the brute-force host
reference of ``tests/window_cases.py`` (timed on ONE video, one run, and scaled to the video count: stated as such in the line), and
each device time as a fraction of the headline step (``--step-ms``, README).  Logits are the ``two_peak`` family of the tests."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import window_cases as W  # noqa: E402
from mraudio_amd import scorer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--shapes", default="32x32x10x0,32x256x10x0,256x256x10x0,1x4096x10x0,32x4096x10x64", help="comma-separated VIDEOSxCLIPSxTOP_KxMAX_LEN")
ap.add_argument("--nms-thd", type=float, default=0.25)
ap.add_argument("--alpha", type=float, default=0.5)
ap.add_argument("--step-ms", type=float, nargs=2, default=[6.40, 6.72], help="the headline step's range the fractions refer to")
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "windows_line.json"))
a = ap.parse_args()


def timed(fn):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], ms[0]


res = {"metric": "window_proposals", "nms_thd": a.nms_thd, "alpha": a.alpha, "reps": a.reps, "step_ms": a.step_ms,
       "note": "ms = median of reps launches between device events (launch overhead included); host_ms_scaled = one video on the host x videos"}
for V, T, top_k, max_len in [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]:
    x_h = W.make_batch("two_peak", T, V, seed=5)
    x = torch.from_numpy(x_h).cuda().reshape(-1)
    med, best = timed(lambda: scorer.windows_from_logits(x, V, T, a.alpha, top_k, a.nms_thd, max_len))
    span_med, span_best = timed(lambda: scorer.spans_from_logits(x, V, T, a.alpha))
    cap = T if max_len == 0 else min(max_len, T)
    r = {"ms": round(med, 4), "ms_best": round(best, 4), "span_ms": round(span_med, 4), "span_ms_best": round(span_best, 4),
         "windows_per_video": T * cap - cap * (cap - 1) // 2, "counts_mean": round(float(scorer.windows_from_logits(x, V, T, a.alpha, top_k, a.nms_thd, max_len)[2].float().mean()), 2),
         "frac_of_step": [round(med / a.step_ms[1], 4), round(med / a.step_ms[0], 4)]}
    if not a.no_host:
        t0 = time.perf_counter()
        W.windows_ref(x_h[:1], 1, T, a.alpha, top_k, a.nms_thd, max_len)
        one = (time.perf_counter() - t0) * 1e3
        r.update({"host_ms_one_video": round(one, 2), "host_ms_scaled": round(one * V, 1)})
    res[f"{V}x{T}x{top_k}x{max_len}"] = r
line = json.dumps(res)
print(line)
if a.output:
    os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
    with open(a.output, "w") as fh:
        fh.write(line + "\n")
