"""Times what the encoder-side gradients add to the Q-Former training step on the video Q-Former and writes one JSON line (``--output``,
default ``profiles/enc_grad_line.json``; also printed).  ONE process, device events, everything warmed up first, the routes alternating
inside every repetition (so drift hits them alike), median and best of ``--reps`` (>= 11).

Step routes (modality LayerNorm + forward with a tape + backward, 20 items x Kv 257, L = 32, bf16, seeded weights):

    (a) ``plain``      ``modality_ln`` under no_grad, ``forward_train`` + backward: today's step, no encoder-side gradient
    (b) ``ln_only``    ``modality_ln_train``: + ``mra_qformer_backward_enc`` and the LayerNorm backward for d ln.weight / d ln.bias
    (c) ``ln_and_dx``  the same with the raw features requiring grad: the LayerNorm backward writes d_x too

The new GEMM alone (``mra_debug_kvgrad_gemm`` on a random cache) against ``mra_kv_project`` at the same shape -- the forward launch that
executes the same flops (2 Ne Kv E ncross 2 768) -- alternating in the same session: ``kvgrad_gemm`` / ``kv_project`` ms and their ratio."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mraudio_amd._lib import check, current_stream, lib, ptr  # noqa: E402
from mraudio_amd.qformer import QFormer, QFormerConfig, draw_seeded  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--items", type=int, default=20)
ap.add_argument("--kv", type=int, default=257)
ap.add_argument("--L", type=int, default=32)
ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "enc_grad_line.json"))
a = ap.parse_args()
if a.reps < 11:
    ap.error("--reps must be at least 11")

dev = torch.device("cuda:0")
cfg = QFormerConfig(enc_width=1408, op_dtype=torch.bfloat16)
qf = QFormer(cfg, device=dev)
g = qf.init_seeded_(seed=0, perturb=True)
qf.push("query_tokens", draw_seeded(g, (1, cfg.n_query, cfg.hidden), "w", True))
gain = draw_seeded(g, (cfg.enc_width,), "g", True).to(dev).requires_grad_(True)
bias = draw_seeded(g, (cfg.enc_width,), "z", True).to(dev).requires_grad_(True)
qf.push("ln.weight", gain)
qf.push("ln.bias", bias)
qf.enable_training()
items, kv, L = a.items, a.kv, a.L


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


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
        out[k] = {"ms": round(v[len(v) // 2], 4), "ms_best": round(v[0], 4)}
    return out


gen = torch.Generator().manual_seed(items * 31 + kv)
raw = torch.randn(items, kv, cfg.enc_width, generator=gen).to(dev).to(torch.bfloat16)       # the encoder's output, operand dtype
raw_g = raw.clone().requires_grad_(True)
ids = torch.randint(1000, cfg.vocab, (items, L), generator=gen).to(dev)
att = torch.ones(items, cfg.n_query + L, dtype=torch.long, device=dev)
rq = torch.randn(items, cfg.n_query, cfg.hidden, generator=gen).to(dev)
rc = torch.randn(items, cfg.hidden, generator=gen).to(dev)


def step(enc):
    z, c = qf.forward_train(ids, att, enc)
    ((z * rq).sum() + (c * rc).sum()).backward()


def plain():
    with torch.no_grad():
        enc = qf.modality_ln(raw)
    step(enc)


def ln_only():
    step(qf.modality_ln_train(raw, gain, bias))


def ln_and_dx():
    step(qf.modality_ln_train(raw_g, gain, bias))
    raw_g.grad = None


res = {"metric": "enc_grad", "items": items, "kv": kv, "L": L, "dtype": "bf16", "reps": a.reps, "warmup": a.warmup,
       "note": "ms = median of reps between device events, routes alternating inside each repetition; step = modality LayerNorm + forward "
               "with a tape + backward"}
res["step"] = median_of({"plain": plain, "ln_only": ln_only, "ln_and_dx": ln_and_dx})
gain.grad = bias.grad = None

# the new GEMM alone against its forward twin
ncross = -(-cfg.layers // cfg.cross_freq)
cache_bytes = int(lib().mra_kv_cache_bytes(qf._handle, items, kv))
dkv = (torch.randn(cache_bytes // 2, generator=torch.Generator().manual_seed(3)) * 0.1).to(dev).to(torch.bfloat16)
kv_cache = torch.empty(cache_bytes // 2, dtype=torch.bfloat16, device=dev)
d_enc = torch.empty(items, kv, cfg.enc_width, dtype=torch.float32, device=dev)
with torch.no_grad():
    enc16 = qf.modality_ln(raw)


def kvgrad_gemm():
    check(lib().mra_debug_kvgrad_gemm(qf._handle, ptr(dkv), cache_bytes, items, kv, ptr(d_enc), d_enc.numel() * 4, current_stream()), "mra_debug_kvgrad_gemm")


def kv_project():
    check(lib().mra_kv_project(qf._handle, ptr(enc16), items, kv, ptr(kv_cache), current_stream()), "mra_kv_project")


with torch.cuda.device(dev):
    pair = median_of({"kvgrad_gemm": kvgrad_gemm, "kv_project": kv_project})
flops = 2.0 * items * kv * cfg.enc_width * ncross * 2 * cfg.hidden
for r in pair.values():
    r["tflops"] = round(flops / (r["ms"] * 1e-3) / 1e12, 1)
res["gemm"] = pair
res["gemm"]["ratio"] = round(pair["kvgrad_gemm"]["ms"] / pair["kv_project"]["ms"], 3)
res["gemm"]["flops"] = flops
print(f"step: " + "  ".join(f"{k} {r['ms']:.3f} ms" for k, r in res["step"].items()) +
      f"   gemm: kvgrad {pair['kvgrad_gemm']['ms']:.3f} ms, kv_project {pair['kv_project']['ms']:.3f} ms", file=sys.stderr, flush=True)
line = json.dumps(res)
print(line)
if a.output:
    os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
    with open(a.output, "w") as fh:
        fh.write(line + "\n")
