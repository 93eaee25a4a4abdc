"""A/B/C of the LM objective's vocabulary head + cross-entropy (mraudio_amd/models/lm_head.py), forward + backward to the hidden states:

  (a) stock  lm_head over every position, the logits upcast to fp32, the causal shift and ``cross_entropy`` with ignore_index -100 -- what
             ``LlamaForCausalLM.forward(labels=...)`` runs after its decoder (transformers' ``ForCausalLMLoss``);
  (b) rows   ``lm_head_ce(hip=False)``: the labelled rows gathered, fp32 ``h_rows @ W.T``, ``logsumexp``, autograd;
  (c) fused  ``lm_head_ce(hip=True)``: ``mra_lm_head_ce_forward`` / ``mra_lm_head_ce_backward`` in one autograd node.

Shape: B = 2, S = 2700 (what the prompt assembler builds for T = 32 positions), V = 32001, K = 4096 (Vicuna-7B's head after ``[PAD]``), bf16,
40 labelled rows per sample.  ms per call = median of ``--reps`` repetitions between device events over ``--inner`` back-to-back calls, the
routes alternating inside each repetition, one process; peak MB = ``torch.cuda.max_memory_allocated`` over one call minus what was allocated
before it (inputs and weight excluded, the [B, S, K] gradient of the hidden states included).  One JSON line on stdout, also written to ``--out`` (profiles/lm_head_ce_line.json is such a line).

    python tools/bench_lm_head.py --out profiles/lm_head_ce_line.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mraudio_amd.models.lm_head import lm_head_ce  # noqa: E402


def _time(fn, inner: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def _peak_mb(fn, hidden) -> float:
    hidden.grad = None                      # the previous call's gradient is not this call's memory
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--seq", type=int, default=2700)
    ap.add_argument("--vocab", type=int, default=32001)
    ap.add_argument("--hidden", type=int, default=4096)
    ap.add_argument("--labelled", type=int, default=40, help="labelled rows per sample (the tail of the sequence, as an answer is)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_lm_head needs a GPU: a CPU timing says nothing about the kernels")
    dev = torch.device("cuda:0")
    B, S, V, K = args.batch, args.seq, args.vocab, args.hidden
    gen = torch.Generator(device=dev).manual_seed(0)
    hidden = torch.randn(B, S, K, device=dev, dtype=torch.bfloat16, generator=gen).requires_grad_(True)
    weight = (torch.randn(V, K, device=dev, dtype=torch.float32, generator=gen) * 0.02).to(torch.bfloat16)
    labels = torch.full((B, S), -100, device=dev)
    labels[:, S - args.labelled:] = torch.randint(0, V, (B, args.labelled), device=dev, generator=gen)

    def stock():
        hidden.grad = None
        logits = torch.nn.functional.linear(hidden, weight).float()
        shift = torch.nn.functional.pad(labels, (0, 1), value=-100)[..., 1:].contiguous()
        torch.nn.functional.cross_entropy(logits.view(-1, V), shift.view(-1), ignore_index=-100).backward()

    def route(hip):
        def run():
            hidden.grad = None
            lm_head_ce(hidden, weight, labels, hip=hip).backward()
        return run

    routes = {"stock": stock, "rows": route(False), "fused": route(True)}
    grads, losses = {}, {}
    for k, fn in routes.items():
        fn()
        grads[k] = hidden.grad.float().clone()
    with torch.no_grad():
        losses = {"rows": lm_head_ce(hidden, weight, labels, hip=False).item(), "fused": lm_head_ce(hidden, weight, labels, hip=True).item()}
    for _ in range(args.warmup):
        for fn in routes.values():
            _time(fn, args.inner)
    ms = {k: [] for k in routes}
    for _ in range(args.reps):
        for k, fn in routes.items():
            ms[k].append(_time(fn, args.inner))
    line = {"metric": "lm_head_ce", "dtype": "bf16", "B": B, "S": S, "V": V, "K": K, "labelled_rows": B * args.labelled, "reps": args.reps,
            "warmup": args.warmup, "inner": args.inner,
            "note": "forward + backward to the hidden states; ms = median of reps between device events over `inner` back-to-back calls, routes "
                    "alternating inside each repetition; peak_mb = max_memory_allocated over one call minus the allocation before it",
            "routes": {k: {"ms": round(statistics.median(v), 4), "ms_best": round(min(v), 4), "ms_worst": round(max(v), 4), "peak_mb": _peak_mb(routes[k], hidden)}
                       for k, v in ms.items()},
            "loss": losses,
            "rel_diff_dh": {"fused_vs_rows": round(((grads["fused"] - grads["rows"]).norm() / grads["rows"].norm()).item(), 5),
                            "stock_vs_rows": round(((grads["stock"] - grads["rows"]).norm() / grads["rows"].norm()).item(), 5)}}
    r = line["routes"]
    line["ratio_fused_over_rows"] = round(r["fused"]["ms"] / r["rows"]["ms"], 3)
    line["ratio_fused_over_stock"] = round(r["fused"]["ms"] / r["stock"]["ms"], 3)
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
