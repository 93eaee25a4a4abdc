"""A/B of the LM prefill's attention (mraudio_amd/models/lm_decode.py):

  (a) kernel   ``prefill_attention(hip=True)`` (``mra_prefill_attention``: one launch under the key byte mask) against
               ``scaled_dot_product_attention`` under the bool ``[B, 1, S, S]`` mask the stock route builds (causal AND padding) on the same
               tensors: B = 2, Hq = Hkv = 32, D = 128, bf16 (one layer of a Vicuna-7B shape), S in {1900, 5400} (the prefix the prompt
               assembler builds at T = 20 / T = 60), 5 % left padding in the second sequence, q as the transposed view transformers hands over.
               ms per call, TF/s on the executed causal flops 4 D Hq sum_b n_b (n_b + 1) / 2 (n_b attended positions) and the fraction of 2.5 PF;
               the largest difference of either route from the definition as fp32 torch ops over the rows with an attended key.
  (b) generate the 4-layer Llama of tools/bench_lm_decode.py (hidden 1024, 8 heads of 128) behind a prefix of 1900 embedded positions, B = 2,
               ``HipLmDecoder`` (``lm_decode="hip_step"``) under ``prefill="stock"`` and ``prefill="hip"``: the prefill forward alone and the
               whole call of 64 greedy tokens, timed separately.

ms = median of ``--reps`` repetitions between device events, the routes alternating inside each repetition, one process.  Every timed step runs
under a time limit of its own (``--step-limit`` seconds: a watchdog ends the process, a hung step is not waited for).  One JSON line on stdout,
also written to ``--out`` (profiles/lm_prefill_line.json is such a line).

    python tools/bench_lm_prefill.py --out profiles/lm_prefill_line.json
"""
from __future__ import annotations

import argparse
import faulthandler
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mraudio_amd.models.lm_decode import hip_decode, prefill_attention  # noqa: E402
from mraudio_amd.models.lm_step import HipLmDecoder  # noqa: E402

LIMIT = 60.0


def _time(fn, inner: int) -> float:
    faulthandler.dump_traceback_later(LIMIT, exit=True)              # the step's own time limit: the process ends, nothing is retried
    try:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / inner
    finally:
        faulthandler.cancel_dump_traceback_later()


def _alternate(routes: dict, reps: int, warmup: int, inner: int) -> dict:
    for _ in range(warmup):
        for fn in routes.values():
            _time(fn, inner)
    ms = {k: [] for k in routes}
    for _ in range(reps):
        for k, fn in routes.items():
            ms[k].append(_time(fn, inner))
    return {k: {"ms": round(statistics.median(v), 4), "ms_best": round(min(v), 4), "ms_worst": round(max(v), 4)} for k, v in ms.items()}


def bench_kernel(dev, S: int, reps: int, warmup: int, inner: int) -> dict:
    B, H, D = 2, 32, 128
    gen = torch.Generator(device=dev).manual_seed(S)
    q = torch.randn(B, S, H, D, device=dev, dtype=torch.bfloat16, generator=gen).transpose(1, 2)      # [B, H, S, D] as a transposed view
    k = torch.randn(B, H, S, D, device=dev, dtype=torch.bfloat16, generator=gen)
    v = torch.randn(B, H, S, D, device=dev, dtype=torch.bfloat16, generator=gen)
    pad = S // 20
    key = torch.ones(B, 1, 1, S, dtype=torch.bool, device=dev)
    key[1, :, :, :pad] = False
    causal = torch.arange(S, device=dev)[None, :] <= torch.arange(S, device=dev)[:, None]
    full = (key & causal[None, None]).contiguous()                                                     # bool [B, 1, S, S]: what sdpa_mask builds
    scale = D ** -0.5
    routes = {"sdpa": lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=full, scale=scale),
              "hip": lambda: prefill_attention(q, k, v, key, scale, hip=True)}
    a, b = routes["hip"]().float(), routes["sdpa"]().transpose(1, 2).float()
    live = key[:, 0, 0, :, None, None].expand_as(a)                                                    # pad query rows: +0 here, anything there
    diff = (a - b)[live].abs().max().item()
    ops = torch.cat([prefill_attention(q[i:i + 1].float(), k[i:i + 1].float(), v[i:i + 1].float(), key[i:i + 1], scale, hip=False) for i in range(B)])
    against_ops = {n: round((x - ops)[live].abs().max().item(), 5) for n, x in (("hip", a), ("sdpa", b))}    # the definition as fp32 torch ops
    del ops
    out = _alternate(routes, reps, warmup, inner)
    flops = sum(4 * D * H * n * (n + 1) // 2 for n in (S, S - pad))
    for r in out.values():
        r["tf_per_s"] = round(flops / (r["ms"] * 1e-3) / 1e12, 2)
        r["fraction_of_2.5_pf"] = round(flops / (r["ms"] * 1e-3) / 2.5e15, 4)
    return {"S": S, "left_pad": pad, "flops": flops, "mask_bytes_sdpa": full.numel(), "mask_bytes_hip": key.numel(), "max_abs_diff": round(diff, 5),
            "max_abs_diff_against_fp32_ops": against_ops, "routes": out, "ratio_hip_over_sdpa": round(out["hip"]["ms"] / out["sdpa"]["ms"], 3)}


def bench_generate(dev, reps: int, warmup: int, prefix: int, new_tokens: int) -> dict:
    import transformers as tf

    torch.manual_seed(0)
    cfg = tf.LlamaConfig(vocab_size=4096, hidden_size=1024, intermediate_size=2752, num_hidden_layers=4, num_attention_heads=8,
                         num_key_value_heads=8, max_position_embeddings=4096, pad_token_id=0, bos_token_id=1, eos_token_id=2)
    llm = tf.LlamaForCausalLM(cfg).to(dev).to(torch.bfloat16).eval().requires_grad_(False)
    B = 2
    embeds = (torch.randn(B, prefix, 1024, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 0.5).to(torch.bfloat16)
    mask = torch.ones(B, prefix, dtype=torch.long, device=dev)
    mask[1, :prefix // 20] = 0
    pos = (mask.cumsum(-1) - 1).masked_fill(mask == 0, 1)
    fw = dict(inputs_embeds=embeds, attention_mask=mask, position_ids=pos, use_cache=True, return_dict=True, logits_to_keep=1)
    tokens = {}
    dec = {p: HipLmDecoder(llm, prefill=p) for p in ("stock", "hip")}

    def prefill_hip():
        with hip_decode(llm, prefill=True):
            llm(**fw)

    with torch.no_grad():
        pre = _alternate({"stock": lambda: llm(**fw), "hip": prefill_hip}, reps, warmup, 1)
        whole = _alternate({p: (lambda p=p: tokens.__setitem__(p, dec[p].generate(embeds, mask, new_tokens, ignore_eos=True))) for p in dec}, reps, warmup, 1)
    n = tokens["stock"].numel()
    return {"layers": 4, "hidden": 1024, "heads": 8, "head_dim": 128, "B": B, "prefix": prefix, "new_tokens": new_tokens, "lm_decode": "hip_step",
            "prefill": pre, "whole_call": whole, "tokens_equal_to_stock_prefill": f"{int((tokens['hip'] == tokens['stock']).sum())}/{n}",
            "ratio_prefill_hip_over_stock": round(pre["hip"]["ms"] / pre["stock"]["ms"], 3),
            "ratio_whole_hip_over_stock": round(whole["hip"]["ms"] / whole["stock"]["ms"], 3)}


def main(argv=None) -> None:
    global LIMIT
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--seqs", type=int, nargs="+", default=[1900, 5400])
    ap.add_argument("--prefix", type=int, default=1900)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--step-limit", type=float, default=60.0, help="seconds a single timed step may take before the process is ended")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_lm_prefill needs a GPU: a CPU timing says nothing about the kernels")
    LIMIT = args.step_limit
    dev = torch.device("cuda:0")
    line = {"metric": "lm_prefill", "dtype": "bf16", "reps": args.reps, "warmup": args.warmup, "inner": args.inner,
            "note": "ms = median of reps between device events, routes alternating inside each repetition; kernel: per call over `inner` back-to-back "
                    "calls, B = 2, Hq = Hkv = 32, D = 128, TF/s on the executed causal flops; generate: the prefill forward alone and the whole call "
                    "of 64 greedy tokens under lm_decode hip_step; every section is measured anew by every run of this tool: a line holds one session",
            "kernel": [bench_kernel(dev, S, args.reps, args.warmup, args.inner) for S in args.seqs],
            "generate": bench_generate(dev, args.reps, 1, args.prefix, args.new_tokens)}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
