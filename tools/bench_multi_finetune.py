"""Times the Q-Former training step (forward with a tape + backward) for P prompts per clip on the video Q-Former and writes one JSON
line (``--output``, default ``profiles/multi_finetune_line.json``; also printed).  Three routes to the gradients of ``items x P``
prompt-items, in ONE process, between device events, every shape warmed up first, the routes alternating inside every repetition (so
drift hits them alike), median and best of ``--reps`` (>= 11):

    (a) ``multi``        one ``forward_multi_train`` + backward: K/V projection, dK / dV tape and K/V weight gradients once per item
    (b) ``replicated``   one ``forward_train`` + backward on ``enc.repeat_interleave(P, 0)`` (the repeat is part of the route)
    (c) ``per_query``    P ``forward_train`` + backward calls of ``items`` items each, one per prompt slot

Shape: 20 items x Kv 257 with P in {1, 2, 4, 8}; L = 32, bf16, seeded weights.  The gradient buffer accumulates over the run (every
route ADDS into it); its values are not read.  Per route: ms, ms_best, prompt-items / s and the tape workspace bytes."""
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
ap.add_argument("--shapes", default="20x257:1,2,4,8", help="ITEMSxKV:P,P,...;...")
ap.add_argument("--L", type=int, default=32)
ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "multi_finetune_line.json"))
a = ap.parse_args()
if a.reps < 11:
    ap.error("--reps must be at least 11")

dev = torch.device("cuda:0")
cfg = QFormerConfig(enc_width=1408, op_dtype=torch.bfloat16)
qf = QFormer(cfg, device=dev)
g = qf.init_seeded_(seed=0, perturb=True)
qf.push("query_tokens", draw_seeded(g, (1, cfg.n_query, cfg.hidden), "w", True))
qf.enable_training()
L = a.L


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


res = {"metric": "multi_finetune", "L": L, "dtype": "bf16", "reps": a.reps, "warmup": a.warmup,
       "note": "ms = median of reps forward + backward between device events, routes alternating inside each repetition; "
               "items_per_s = items * P / median"}
for spec in a.shapes.split(";"):
    shape, ps = spec.split(":")
    items, kv = (int(x) for x in shape.split("x"))
    gen = torch.Generator().manual_seed(items * 31 + kv)
    enc = torch.randn(items, kv, cfg.enc_width, generator=gen).to(dev).to(torch.bfloat16)
    for P in (int(p) for p in ps.split(",")):
        n = items * P
        ids = torch.randint(1000, cfg.vocab, (n, L), generator=gen).to(dev)
        att = torch.ones(n, cfg.n_query + L, dtype=torch.long, device=dev)
        rq = torch.randn(n, cfg.n_query, cfg.hidden, generator=gen).to(dev)
        rc = torch.randn(n, cfg.hidden, generator=gen).to(dev)
        slot_ids = [ids[p::P].contiguous() for p in range(P)]
        slot_att = [att[p::P].contiguous() for p in range(P)]
        slot_rq, slot_rc = [rq[p::P].contiguous() for p in range(P)], [rc[p::P].contiguous() for p in range(P)]

        def step(z, c, wq, wc):
            ((z * wq).sum() + (c * wc).sum()).backward()

        def multi():
            step(*qf.forward_multi_train(ids, att, enc, P), rq, rc)

        def replicated():
            step(*qf.forward_train(ids, att, enc.repeat_interleave(P, 0)), rq, rc)

        def per_query():
            for p in range(P):
                step(*qf.forward_train(slot_ids[p], slot_att[p], enc), slot_rq[p], slot_rc[p])

        routes = {"multi": multi, "replicated": replicated, "per_query": per_query}
        for _ in range(a.warmup):
            for fn in routes.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in routes}
        for _ in range(a.reps):
            for k, fn in routes.items():
                ms[k].append(event_ms(fn))
        ws = {"multi": int(lib().mra_qformer_multi_train_workspace_bytes(qf._handle, items, P, L, kv)),
              "replicated": int(lib().mra_qformer_train_workspace_bytes(qf._handle, n, L, kv)) + enc.numel() * 2 * P,
              "per_query": int(lib().mra_qformer_train_workspace_bytes(qf._handle, items, L, kv))}
        row = {}
        for k, v in ms.items():
            v.sort()
            med = v[len(v) // 2]
            row[k] = {"ms": round(med, 4), "ms_best": round(v[0], 4), "items_per_s": round(n / med * 1e3, 1), "workspace_bytes": ws[k]}
        res[f"{items}x{kv}xP{P}"] = row
        print(f"{items}x{kv} P={P}: " + "  ".join(f"{k} {r['ms']:.3f} ms" for k, r in row.items()), file=sys.stderr, flush=True)
res["workspace_note"] = "replicated: the tape workspace plus the replicated encoder rows"
line = json.dumps(res)
print(line)
if a.output:
    os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
    with open(a.output, "w") as fh:
        fh.write(line + "\n")
