"""A/B of the LoRA branch (mraudio_amd/models/lora.py): the HIP route (mra_lora_down / mra_lora_up_add / mra_lora_wgrad inside one autograd
node) against the same arithmetic as stock torch ops on the same tensors (``LoraLinear(hip=False)``).

  1. one adapted linear, forward + backward, bf16, M = 2048 rows, K/N = 4096/4096 and 4096/11008 (the two linear shapes of a 7B Llama),
     R = 8, p = 0.05;
  2. the whole step (forward, loss, backward) of a small Llama with every linear adapted, with and without the HIP route.

ms per call = median of ``--reps`` repetitions between device events over ``--inner`` back-to-back calls, the two routes alternating inside
each repetition.  One JSON line on stdout, also written to ``--out`` (profiles/lora_line.json is such a line).

    python tools/bench_lora.py --out profiles/lora_line.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mraudio_amd.models.lora import LoraLinear, apply_lora, lora_modules, lora_parameters  # noqa: E402


def _time(fn, inner: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def _ab(routes: dict, reps: int, warmup: int, inner: int) -> dict:
    for _ in range(warmup):
        for fn in routes.values():
            _time(fn, inner)
    ms = {k: [] for k in routes}
    for _ in range(reps):
        for k, fn in routes.items():
            ms[k].append(_time(fn, inner))
    return {k: {"ms": round(statistics.median(v), 4), "ms_best": round(min(v), 4), "ms_worst": round(max(v), 4)} for k, v in ms.items()}


def bench_linear(dev, M: int, K: int, N: int, R: int, p: float, reps: int, warmup: int, inner: int) -> dict:
    torch.manual_seed(0)
    base = nn.Linear(K, N, bias=False, device=dev, dtype=torch.bfloat16)
    mod = LoraLinear(base, r=R, alpha=R, dropout=p).train()
    with torch.no_grad():
        mod.lora_B["default"].weight.normal_(0, 0.02)
    x = torch.randn(M, K, device=dev, dtype=torch.bfloat16).requires_grad_(True)
    g = torch.randn(M, N, device=dev, dtype=torch.bfloat16)

    def step(hip):
        def run():
            mod.hip = hip
            x.grad = None
            for q in mod.parameters():
                q.grad = None
            mod(x).backward(g)
        return run

    def base_only():
        x.grad = None
        base(x).backward(g)

    A, B = mod.lora_A["default"].weight, mod.lora_B["default"].weight

    def stock():   # what an off-the-shelf adapter runs: torch's own dropout (a stored mask, other random numbers), 16-bit matmuls, scale, add
        x.grad = A.grad = B.grad = None
        h = nn.functional.linear(nn.functional.dropout(x, p, True), A.to(x.dtype))
        (base(x) + nn.functional.linear(h, B.to(x.dtype)) * mod.scaling).backward(g)

    grads = {}
    for hip in (True, False):
        torch.manual_seed(1)
        step(hip)()
        grads[hip] = [x.grad.float().clone(), mod.lora_A["default"].weight.grad.clone(), mod.lora_B["default"].weight.grad.clone()]
    diff = {n: round(((a - b).norm() / b.norm()).item(), 5) for n, a, b in zip(("dx", "dA", "dB"), grads[True], grads[False])}
    out = _ab({"hip": step(True), "torch": step(False), "stock_dropout": stock, "base_linear_only": base_only}, reps, warmup, inner)
    out["rel_diff_hip_vs_torch"] = diff
    out["ratio_hip_over_torch"] = round(out["hip"]["ms"] / out["torch"]["ms"], 3)
    out["ratio_hip_over_stock_dropout"] = round(out["hip"]["ms"] / out["stock_dropout"]["ms"], 3)
    # what the adapter branch adds on top of the base linear's own forward + backward
    out["branch_ms"] = {k: round(out[k]["ms"] - out["base_linear_only"]["ms"], 4) for k in ("hip", "torch", "stock_dropout")}
    return out


def bench_llama(dev, reps: int, warmup: int, inner: int, R: int, p: float) -> dict:
    import transformers as tf

    torch.manual_seed(0)
    cfg = tf.LlamaConfig(vocab_size=4096, hidden_size=1024, intermediate_size=2752, num_hidden_layers=4, num_attention_heads=8,
                         num_key_value_heads=8, max_position_embeddings=1024)
    llm = tf.LlamaForCausalLM(cfg).to(dev).to(torch.bfloat16).requires_grad_(False)
    apply_lora(llm, r=R, alpha=R, dropout=p)
    llm.train()
    mods = list(lora_modules(llm).values())
    with torch.no_grad():
        for m in mods:
            m.lora_B["default"].weight.normal_(0, 0.02)
    ids = torch.randint(0, 4096, (4, 512), device=dev)               # 2048 rows per linear
    emb = llm.get_input_embeddings()(ids).detach().requires_grad_(True)   # the projections' output is where the gradient leaves the LM

    def step(hip):
        def run():
            for m in mods:
                m.hip = hip
            emb.grad = None
            for q in lora_parameters(llm):
                q.grad = None
            llm(inputs_embeds=emb, labels=ids).loss.backward()
        return run

    out = _ab({"hip": step(True), "torch": step(False)}, reps, warmup, inner)
    out["shape"] = {"layers": 4, "hidden": 1024, "inter": 2752, "rows": 2048, "adapted_linears": len(mods)}
    out["ratio_hip_over_torch"] = round(out["hip"]["ms"] / out["torch"]["ms"], 3)
    return out


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--rank", type=int, default=8)
    ap.add_argument("--dropout", type=float, default=0.05)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-llama", action="store_true")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_lora needs a GPU: a CPU timing says nothing about the kernels")
    dev = torch.device("cuda:0")
    line = {"metric": "lora", "dtype": "bf16", "rows": args.rows, "rank": args.rank, "dropout": args.dropout, "reps": args.reps, "warmup": args.warmup,
            "inner": args.inner,
            "note": "ms per call (forward + backward) = median of reps between device events over `inner` back-to-back calls, routes alternating "
                    "inside each repetition; torch = LoraLinear(hip=False), the same arithmetic "
                    "(the counter-based mask included) as stock ops; stock_dropout = torch's own dropout with a stored mask and 16-bit matmuls",
            "linear": {}}
    for K, N in ((4096, 4096), (4096, 11008)):
        line["linear"][f"{K}x{N}"] = bench_linear(dev, args.rows, K, N, args.rank, args.dropout, args.reps, args.warmup, args.inner)
    if not args.no_llama:
        line["llama_step"] = bench_llama(dev, args.reps, args.warmup, max(1, args.inner // 4), args.rank, args.dropout)
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
