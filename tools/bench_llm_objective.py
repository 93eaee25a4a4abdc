"""Times ``mra_llm_proj_backward`` alone -- the backward of the LLM projection, the link that carries the LM loss into the Q-Former --
against the same three products as stock PyTorch matmuls on the same tensors, and writes one JSON line (``--output``, default
``profiles/llm_proj_bwd_line.json``; also printed).  ONE process, device events, everything warmed up first, the two routes alternating
inside every repetition (so drift hits them alike), median and best of ``--reps`` (>= 11); a timed window is ``--inner`` back-to-back calls
(a single call is tens of microseconds) and the figures are per call.

    hip     one ``mra_llm_proj_backward`` (bf16 d_out): d_z = dY W, d_W += dY^T z16, d_b += colsum(dY)   (+ the conversion of z)
    torch   ``d_out @ W``, ``d_out.T @ z16``, ``d_out.sum(0)`` in bf16 on the same tensors (z16 converted once, outside the window)

Shapes: rows = 640 and 1920 (20 and 60 positions x 32 queries), hidden 768, llm_hidden 4096, bf16.  No speed is promised: the feature is the
gradient; the line records both numbers."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mraudio_amd import _lib  # noqa: E402
from mraudio_amd._lib import check, current_stream, lib, ptr  # noqa: E402
from mraudio_amd.qformer import QFormer, QFormerConfig  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--inner", type=int, default=20)
ap.add_argument("--rows", type=int, nargs="+", default=[640, 1920])
ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "llm_proj_bwd_line.json"))
a = ap.parse_args()
if a.reps < 11:
    ap.error("--reps must be at least 11")

dev = torch.device("cuda:0")
cfg = QFormerConfig(enc_width=768, layers=2, op_dtype=torch.bfloat16)
qf = QFormer(cfg, device=dev)
H, Lh = cfg.hidden, cfg.llm_hidden
gen = torch.Generator().manual_seed(0)
W = (torch.randn(Lh, H, generator=gen) * 0.02).to(dev).to(torch.bfloat16)
qf.push("llm_proj.weight", W)
qf.push("llm_proj.bias", torch.zeros(Lh))


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.inner


def median_of(routes):
    for _ in range(a.warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in routes}
    for _ in range(a.reps):
        for k, fn in routes.items():
            ms[k].append(event_ms(fn))
    out = {}
    for k, v in ms.items():
        v.sort()
        out[k] = {"ms": round(v[len(v) // 2], 4), "ms_best": round(v[0], 4), "ms_worst": round(v[-1], 4)}
    return out


res = {"metric": "llm_proj_bwd", "hidden": H, "llm_hidden": Lh, "dtype": "bf16", "reps": a.reps, "warmup": a.warmup, "inner": a.inner,
       "note": "ms per call = median of reps between device events over `inner` back-to-back calls, routes alternating inside each repetition",
       "rows": {}}
for rows in a.rows:
    g = torch.Generator().manual_seed(rows)
    z = torch.randn(rows, H, generator=g).to(dev)
    d_out = (torch.randn(rows, Lh, generator=g) * 0.5).to(dev).to(torch.bfloat16)
    z16 = z.to(torch.bfloat16)
    d_z = torch.empty(rows, H, dtype=torch.float32, device=dev)
    d_W = torch.zeros(Lh, H, dtype=torch.float32, device=dev)
    d_b = torch.zeros(Lh, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        nbytes = int(lib().mra_llm_proj_backward_workspace_bytes(qf._handle, rows, _lib.MRA_BF16))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def hip():
        check(lib().mra_llm_proj_backward(qf._handle, ptr(z), rows, ptr(d_out), _lib.MRA_BF16, ptr(d_z), ptr(d_W), ptr(d_b), ptr(ws), nbytes,
                                          current_stream()), "mra_llm_proj_backward")

    def stock():
        return d_out @ W, d_out.T @ z16, d_out.sum(0)

    with torch.cuda.device(dev):
        r = median_of({"hip": hip, "torch": stock})
    # the two routes compute the same thing (fp32 accumulation in both; torch rounds its results to bf16)
    d_W.zero_()
    d_b.zero_()
    hip()
    tz, tw, tb = stock()
    torch.cuda.synchronize()
    r["max_rel_diff"] = {k: round(((x - y.float()).abs().max() / y.float().abs().max()).item(), 5) for k, x, y in
                         (("d_z", d_z, tz), ("d_W", d_W, tw), ("d_b", d_b, tb))}
    flops = 2.0 * 2.0 * rows * Lh * H
    for k in ("hip", "torch"):
        r[k]["tflops"] = round(flops / (r[k]["ms"] * 1e-3) / 1e12, 1)
    r["ratio_hip_over_torch"] = round(r["hip"]["ms"] / r["torch"]["ms"], 3)
    res["rows"][str(rows)] = r
    print(f"rows {rows}: hip {r['hip']['ms']:.4f} ms ({r['hip']['ms_best']:.4f} .. {r['hip']['ms_worst']:.4f}), "
          f"torch {r['torch']['ms']:.4f} ms ({r['torch']['ms_best']:.4f} .. {r['torch']['ms_worst']:.4f})", file=sys.stderr, flush=True)
line = json.dumps(res)
print(line)
if a.output:
    os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
    with open(a.output, "w") as fh:
        fh.write(line + "\n")
