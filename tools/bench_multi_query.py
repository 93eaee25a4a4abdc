"""Times P prompts per clip on the video Q-Former and writes one JSON line (``--output``, default ``profiles/multi_query_line.json``; also
printed).  Three ways of scoring ``items x P`` prompt-items, in ONE process, between device events, every shape warmed up first, the
three arms alternating inside every repetition (so drift hits them alike), median and best of ``--reps`` (>= 11):

    (a) ``replicated``   one ``forward_fused`` on ``enc.repeat_interleave(P, 0)`` in automatic cross mode (the repeat is part of the arm)
    (b) ``multi_core0``  ``forward_multi`` with ``multi_core`` 0 (the core of the ordinary forward, K/V base from item / P)
    (c) ``multi_core1``  ``forward_multi`` with ``multi_core`` 1 (the shared-stream core)

Shapes: 40 items x Kv 257 with P in {1, 2, 4, 8, 16}; 32 items x Kv 8224 with P in {1, 2, 4, 8}; L = 32, f16, seeded weights.
Per arm: ms, ms_best, prompt-items / s and the workspace bytes."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mraudio_amd._lib import lib  # noqa: E402
from mraudio_amd.qformer import QFormer, QFormerConfig, draw_seeded  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--shapes", default="40x257:1,2,4,8,16;32x8224:1,2,4,8", help="ITEMSxKV:P,P,...;...")
ap.add_argument("--L", type=int, default=32)
ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "multi_query_line.json"))
a = ap.parse_args()
if a.reps < 11:
    ap.error("--reps must be at least 11")

dev = torch.device("cuda:0")
cfg = QFormerConfig(enc_width=1408, op_dtype=torch.float16)
qf = QFormer(cfg, device=dev)
g = qf.init_seeded_(seed=0, perturb=True)
qf.push("query_tokens", draw_seeded(g, (1, cfg.n_query, cfg.hidden), "w", True))
qf.sync_weights()
L = a.L


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


res = {"metric": "multi_query", "L": L, "dtype": "f16", "reps": a.reps, "warmup": a.warmup,
       "note": "ms = median of reps forwards between device events, arms alternating inside each repetition; items_per_s = items * P / median"}
for spec in a.shapes.split(";"):
    shape, ps = spec.split(":")
    items, kv = (int(x) for x in shape.split("x"))
    gen = torch.Generator().manual_seed(items * 31 + kv)
    enc = torch.randn(items, kv, cfg.enc_width, generator=gen).to(dev).to(torch.float16)
    for P in (int(p) for p in ps.split(",")):
        n = items * P
        ids = torch.randint(1000, cfg.vocab, (n, L), generator=gen).to(dev)
        att = torch.ones(n, cfg.n_query + L, dtype=torch.long, device=dev)

        def replicated():
            qf.forward_fused(ids, att, enc.repeat_interleave(P, 0), want_query=True, want_cls=True)

        def multi(core):
            qf.set_option("multi_core", core)
            qf.forward_multi(ids, att, enc, P, want_query=True, want_cls=True)

        arms = {"replicated": replicated, "multi_core0": lambda: multi(0), "multi_core1": lambda: multi(1)}
        for _ in range(a.warmup):
            for fn in arms.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in arms}
        for _ in range(a.reps):
            for k, fn in arms.items():
                ms[k].append(event_ms(fn))
        ws = {"replicated": int(lib().mra_qformer_workspace_bytes(qf._handle, n, L, kv)) + enc.numel() * 2 * P}
        for core in (0, 1):
            qf.set_option("multi_core", core)
            ws[f"multi_core{core}"] = int(lib().mra_qformer_multi_workspace_bytes(qf._handle, items, P, L, kv))
        row = {}
        for k, v in ms.items():
            v.sort()
            med = v[len(v) // 2]
            row[k] = {"ms": round(med, 4), "ms_best": round(v[0], 4), "items_per_s": round(n / med * 1e3, 1), "workspace_bytes": ws[k]}
        res[f"{items}x{kv}xP{P}"] = row
        print(f"{items}x{kv} P={P}: " + "  ".join(f"{k} {r['ms']:.3f} ms" for k, r in row.items()), file=sys.stderr, flush=True)
qf.set_option("multi_core", 0)
res["workspace_note"] = "replicated: the forward's workspace plus the replicated encoder rows"
line = json.dumps(res)
print(line)
if a.output:
    os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
    with open(a.output, "w") as fh:
        fh.write(line + "\n")
