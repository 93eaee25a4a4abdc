"""Times the video front end (``mra_video_frames_forward``, csrc/video_pre.hip) at the benchmark's size -- 32 clips x 32 frames of
224 x 224 uint8 -> [1024, 3, 224, 224] f16 -- prints one JSON line and writes it to ``--out`` (default
profiles/video_frontend_line.json).  One box, one session; median of ``--reps`` ALTERNATING repetitions after a warm-up.
  identity / crop90      the launch alone (device events around ``--inner`` launches), whole-frame box and a 0.9-area crop with a flip, in
                         the kernel's LDS form (what the product entry runs here) and its plain-gather form (mra_debug_video_frames_forward,
                         form 1): ms, GB/s on mra_video_frames_bytes, and the share of the HBM bound (those bytes at 8 TB/s; the
                         arithmetic, ~30 flops per output element at the fp32 vector rate, bounds the launch lower, so HBM is the bound
                         that applies)
  step_device_ms         the whole step from host uint8, host clock around a device synchronise: upload of the bytes + the launch
  step_host_ms           today's host route on 16 threads: float32, normalise, the two permutes, float32 upload in chunks of 64 frames
  encode_fuse            from video_raw against from video: not measured here (needs the full ViT-g; the front end is outside bench.py)
For rocprofv3:
    rocprofv3 --kernel-trace --stats -d prof_video -- python3 tools/bench_video_frontend.py --reps 3 --no-host"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mraudio_amd.processors.alpro_processors import MEAN, STD, AlproVideoEvalProcessor_Stamps, _normalise  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--inner", type=int, default=5)
ap.add_argument("--clips", type=int, default=32)
ap.add_argument("--frames", type=int, default=32)
ap.add_argument("--size", type=int, default=224)
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_frontend_line.json"))
a = ap.parse_args()
dev = torch.device("cuda:0")
torch.set_num_threads(16)
B, T, S = a.clips, a.frames, a.size
PEAK_HBM = 8.0e12


def event_ms(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


g = torch.Generator().manual_seed(0)
raw = torch.randint(0, 256, (B, T, S, S, 3), generator=g, dtype=torch.uint8)
proc = AlproVideoEvalProcessor_Stamps(image_size=S, n_frms=T, device=dev)
proc.flat(raw[:1])                                            # binds the library
lib = proc._lib
side = int(round(S * 0.9 ** 0.5))
BOXES = {"identity": ((0, 0, S, S), 0, 0), "crop90": (((S - side) // 2, (S - side) // 3, side, side), 1, 1)}   # box, flip, quantize (floor with the crop)
src = raw.reshape(-1).to(dev)
out = torch.empty(B * T, 3, S, S, dtype=torch.float16, device=dev)
mean, std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
launch = {}
keep = []
for name, (box, flip, quant) in BOXES.items():
    idx, w = proc._table(S, S, box)
    idx_d, w_d = idx[None].contiguous().to(dev), w[None].contiguous().to(dev)
    rows = torch.tensor([[i * S * S * 3, S, S, 0, flip] for i in range(B * T)], dtype=torch.int64).to(dev)
    keep += [idx_d, w_d, rows]
    for form, tag in ((0, "lds"), (1, "gather")):
        def fn(rows=rows, idx_d=idx_d, w_d=w_d, form=form, quant=quant):
            lib.check(lib.lib().mra_debug_video_frames_forward(lib.ptr(src), src.numel(), lib.ptr(rows), B * T, lib.ptr(idx_d), lib.ptr(w_d), 1, S, mean,
                                                               std, quant, lib.ptr(out), lib.MRA_F16, form, lib.current_stream()), "video frames forward")
        launch[f"{name}_{tag}"] = fn


def step_device():
    proc.flat(raw)


def step_host():
    clips = torch.stack([_normalise(raw[b].permute(3, 0, 1, 2).float(), None, None) for b in range(B)])      # processor + collate: [B, 3, T, H, W]
    frames = clips.permute(0, 2, 1, 3, 4).reshape(B * T, 3, S, S)                                               # XInstructBLIP._encode
    return [frames[c0: c0 + 64].to(dev) for c0 in range(0, B * T, 64)]


for _ in range(a.warmup):
    for fn in launch.values():
        fn()
    step_device()
torch.cuda.synchronize()
t = {k: [] for k in list(launch) + ["step_device", "step_host"]}
for _ in range(a.reps):                      # alternating, same session
    for k, fn in launch.items():
        t[k].append(event_ms(fn, a.inner))
    t["step_device"].append(wall_ms(step_device))
    if not a.no_host:
        t["step_host"].append(wall_ms(step_host))
nbytes = float(lib.lib().mra_video_frames_bytes(B * T, S, S, S, lib.MRA_F16))
res = {"metric": "video_front_end", "clips": B, "frames_per_clip": T, "size": S, "out_dtype": "f16", "host_threads": torch.get_num_threads(),
       "reps": a.reps, "inner": a.inner, "peak_hbm_tb_s": PEAK_HBM / 1e12, "algorithmic_mb": round(nbytes / 1e6, 1), "bound": "hbm",
       "crop90_box": list(BOXES["crop90"][0]), "upload_mb_uint8": round(raw.numel() / 1e6, 1), "upload_mb_float32_today": round(raw.numel() * 4 / 1e6, 1)}
for k in launch:
    ms = median(t[k])
    res[k] = {"ms": round(ms, 4), "ms_best": round(min(t[k]), 4), "gb_s": round(nbytes / ms / 1e6, 1),
              "share_of_hbm_bound": round(nbytes / PEAK_HBM * 1e3 / ms, 3)}
res["step_device_ms"] = round(median(t["step_device"]), 3)
res["step_host_ms"] = round(median(t["step_host"]), 3) if not a.no_host else "not measured"
res["encode_fuse_from_video_raw"] = "not measured"
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
