"""A/B of the prompt assembly in front of the LM (mraudio_amd/models/llm_prompt.py), forward plus backward to the projections:

  (a) cat   ``PromptAssembler.assemble_forward`` over ``{m: v.to(dt)}`` -- per call about ``T * (2 * modalities + 1) + 2`` pieces and one
            ``torch.cat``; autograd's backward (one ``select_backward`` per position and modality);
  (b) plan  ``PromptAssembler.plan_forward`` + ``assemble_plan``: one ``mra_gather_rows`` forward, one per modality backward.

Both build their prompt from the strings on every call (tokenizer included): that is what a training step pays.  Shapes: B = 2, T = 20
and T = 60, D = 4096, a bf16 table of 32001 rows, fp32 projections of two modalities.  ``ms`` = host clock around one call that ends in a
device synchronise, ``host_ms`` = the same clock when the call returns (everything enqueued), both medians of ``--reps`` repetitions with
the routes alternating inside each repetition, one process.  ``launches`` = device kernels and copies of one call as the torch profiler
counts them (null where it sees none).  ``gather`` = the forward ``mra_gather_rows`` launch alone between device events over ``--inner``
back-to-back launches, with its algorithmic bytes ``sum over rows of width * (bytes_in + bytes_out)`` and its share of the 8 TB/s HBM bound.
One JSON line on stdout, also written to ``--out`` (profiles/prompt_assembly_line.json is such a line).

    python tools/bench_prompt_assembly.py --out profiles/prompt_assembly_line.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mraudio_amd.models.llm_prompt import PromptAssembler, SimpleLlmTokenizer, assemble_plan, gather_rows  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
PROMPT = "Query: {}\nGiven the video and the query, find the relevant windows.\nRelevant windows: "
QUERIES = ["a person opens the door and walks out.", "someone sits down on the sofa and reads a book"]
ANSWERS = ["[[12, 18]]", "[[0, 4], [30, 36.5]]"]
Q = 32


def _launches(fn):
    """Device kernels + copies of one call, or None when the profiler reports none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower())
        return n or None
    except Exception:       # a profiler that cannot start is no reason to lose the timings
        return None


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--hidden", type=int, default=4096)
    ap.add_argument("--vocab", type=int, default=32001)
    ap.add_argument("--positions", type=int, nargs="+", default=[20, 60])
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_prompt_assembly needs a GPU: a CPU timing says nothing about the kernels")
    dev = torch.device("cuda:0")
    B, D = args.batch, args.hidden
    torch.manual_seed(0)
    emb = torch.nn.Embedding(args.vocab, D).to(torch.bfloat16).to(dev).requires_grad_(False)
    tok = SimpleLlmTokenizer()
    asm = PromptAssembler(tok, emb, modalities=("video", "audio"), device=dev)
    shapes = []
    for T in args.positions:
        samples = {"text_input": [PROMPT.format(QUERIES[b % 2]) for b in range(B)], "text_output": [ANSWERS[b % 2] for b in range(B)],
                   "timestamps": [[2 * t + b for t in range(T)] for b in range(B)], "duration": [2 * T + b for b in range(B)]}
        gen = torch.Generator(device=dev).manual_seed(T)
        media = {m: torch.randn(B, T * Q, D, device=dev, generator=gen).requires_grad_(True) for m in ("video", "audio")}
        atts = {m: torch.ones(B, T * Q, dtype=torch.long, device=dev) for m in media}
        plan0 = asm.plan_forward(samples, num=T)
        S = int(plan0.mask.shape[1])
        cot = torch.randn(B, S, D, device=dev, generator=gen).to(torch.bfloat16)

        def clear():
            for v in media.values():
                v.grad = None

        def cat():
            clear()
            embeds, _, _ = asm.assemble_forward(samples, {m: v.to(torch.bfloat16) for m, v in media.items()}, atts)
            embeds.backward(cot)

        def plan():
            clear()
            embeds, _, _ = assemble_plan(asm.plan_forward(samples, num=T), emb.weight, media, hip=True)
            embeds.backward(cot)

        routes = {"cat": cat, "plan": plan}
        grads = {}
        for k, fn in routes.items():
            fn()
            torch.cuda.synchronize()
            grads[k] = {m: v.grad.clone() for m, v in media.items()}
        same = all(torch.equal(grads["cat"][m], grads["plan"][m]) for m in media)
        for _ in range(args.warmup):
            for fn in routes.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in routes}
        host = {k: [] for k in routes}
        for _ in range(args.reps):
            for k, fn in routes.items():
                t0 = time.perf_counter()
                fn()
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                host[k].append((t1 - t0) * 1e3)
                ms[k].append((t2 - t0) * 1e3)
        launches = {k: _launches(fn) for k, fn in routes.items()}
        # the forward gather alone
        dplan = plan0.on(dev)["plan"]
        srcs = [emb.weight] + [media[m].detach().view(-1, D) for m in plan0.modalities]
        out = torch.empty(B * S, D, dtype=torch.bfloat16, device=dev)
        src_bytes = torch.tensor([2] + [4] * len(plan0.modalities))
        nbytes = int(((src_bytes[plan0.plan.view(-1, 2)[:, 0].long()] + 2) * D).sum())
        for _ in range(3):
            gather_rows(srcs, dplan, out=out)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ker = []
        for _ in range(args.reps):
            a.record()
            for _ in range(args.inner):
                gather_rows(srcs, dplan, out=out)
            b.record()
            b.synchronize()
            ker.append(a.elapsed_time(b) / args.inner)
        kms = statistics.median(ker)
        shapes.append({"T": T, "S": S, "rows": B * S, "pieces_cat": len(plan0.modalities) * 2 * T + T + 2, "gradients_bit_equal": bool(same),
                       "routes": {k: {"ms": round(statistics.median(ms[k]), 4), "ms_best": round(min(ms[k]), 4), "ms_worst": round(max(ms[k]), 4),
                                      "host_ms": round(statistics.median(host[k]), 4), "launches": launches[k]} for k in routes},
                       "ratio_plan_over_cat": round(statistics.median(ms["plan"]) / statistics.median(ms["cat"]), 3),
                       "gather": {"ms": round(kms, 5), "algorithmic_mb": round(nbytes / 1e6, 2), "tb_per_s": round(nbytes / (kms * 1e-3) / 1e12, 3),
                                  "fraction_of_hbm_bound": round(nbytes / HBM_BYTES_PER_S / (kms * 1e-3), 3)}})
    line = {"metric": "prompt_assembly", "dtype": "bf16 table, fp32 projections", "B": B, "D": D, "modalities": 2, "reps": args.reps, "warmup": args.warmup,
            "inner": args.inner,
            "note": "forward + backward to the projections, the prompt built from its strings on every call; ms = host clock around a call ending "
                    "in a device synchronise, host_ms = the clock when the call returns; medians, routes alternating inside each repetition; "
                    "gather = the forward mra_gather_rows launch alone between device events; HBM bound at 8 TB/s",
            "shapes": shapes}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
