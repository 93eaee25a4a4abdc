"""A/B of the LM's attention in training (mraudio_amd/models/lm_attention.py):

  (a) attention  forward + backward of one layer's attention through ``causal_attention(hip=True)`` (``mra_prefill_attention`` with lse, then
                 one ``mra_prefill_attention_backward``, under the key byte mask) against ``scaled_dot_product_attention`` forward + backward under
                 the bool ``[B, 1, S, S]`` mask the stock route builds, on the same tensors: B = 2, Hq = Hkv = 32, D = 128, bf16 (one layer of a
                 Vicuna-7B shape), S in {1900, 2700, 5400}, 5 % left padding in the second sequence, q as the transposed view transformers hands
                 over.  ms per forward + backward, TF/s on the executed causal flops (forward 4 D Hq sum_b n_b (n_b + 1) / 2 over the n_b attended
                 positions, backward 2.5 x that), the fraction of 2.5 PF, the peak memory over the call above what was allocated before it
                 (the [B, 1, S, S] mask counted with the SDPA route, which needs it), and the largest difference of the gradients.
  (b) step       forward + backward of the training step of the 4-layer Llama of tools/bench_lm_decode.py (hidden 1024, 8 heads of 128) with LoRA
                 adapters and the fused head + loss (``lm_loss="fused"``) over a prefix of 1900 embedded positions, B = 2, 64 labelled rows, as
                 ``_lm_ce`` runs it under ``lm_attention="stock"`` and ``"hip"``.

ms = median of ``--reps`` repetitions between device events, the routes alternating inside each repetition, one process.  Every timed step runs
under a time limit of its own (``--step-limit`` seconds: a watchdog ends the process, a hung step is not waited for).  One JSON line on stdout,
also written to ``--out`` (profiles/lm_attention_bwd_line.json is such a line).

    python tools/bench_lm_attention_bwd.py --out profiles/lm_attention_bwd_line.json
"""
from __future__ import annotations

import argparse
import contextlib
import faulthandler
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mraudio_amd.models.lm_attention import causal_attention, hip_train  # noqa: E402

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


def _peak(fn) -> int:
    """Bytes the call allocates at its peak above what was allocated before it."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    _time(fn, 1)
    return int(torch.cuda.max_memory_allocated() - base)


def bench_attention(dev, S: int, reps: int, warmup: int, inner: int) -> dict:
    B, H, D = 2, 32, 128
    gen = torch.Generator(device=dev).manual_seed(S)
    q = torch.randn(B, S, H, D, device=dev, dtype=torch.bfloat16, generator=gen).transpose(1, 2).requires_grad_(True)   # a transposed view
    k = torch.randn(B, H, S, D, device=dev, dtype=torch.bfloat16, generator=gen).requires_grad_(True)
    v = torch.randn(B, H, S, D, device=dev, dtype=torch.bfloat16, generator=gen).requires_grad_(True)
    dout = torch.randn(B, S, H, D, device=dev, dtype=torch.bfloat16, generator=gen)
    pad = S // 20
    key = torch.ones(B, 1, 1, S, dtype=torch.bool, device=dev)
    key[1, :, :, :pad] = False
    dout[1, :pad] = 0                                                # pad rows take no cotangent: nothing downstream attends them
    causal = torch.arange(S, device=dev)[None, :] <= torch.arange(S, device=dev)[:, None]
    scale = D ** -0.5
    grads = {}

    def sdpa(full=None):
        full = (key & causal[None, None]).contiguous() if full is None else full                      # bool [B, 1, S, S]: what sdpa_mask builds
        out = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=full, scale=scale).transpose(1, 2)
        grads["sdpa"] = torch.autograd.grad(out, (q, k, v), dout)

    def hip():
        grads["hip"] = torch.autograd.grad(causal_attention(q, k, v, key, scale, hip=True), (q, k, v), dout)

    peak = {"sdpa": _peak(sdpa), "hip": _peak(hip)}                  # the SDPA route's peak includes the mask it has to build
    live = key[:, 0, 0, :, None, None]                               # pad query rows: +0 here, NaN there
    diffs = {}
    for name, a, b in zip(("dq", "dk", "dv"), grads["hip"], grads["sdpa"]):
        a, b = a.float(), b.float().nan_to_num(0.0)
        if name == "dq":
            a, b = a * live.transpose(1, 2), b * live.transpose(1, 2)
        diffs[name] = round((a - b).abs().max().item(), 5)
    full = (key & causal[None, None]).contiguous()
    out = _alternate({"sdpa": lambda: sdpa(full), "hip": hip}, reps, warmup, inner)                    # timed with the mask already built
    fwd = sum(4 * D * H * n * (n + 1) // 2 for n in (S, S - pad))
    flops = fwd + 5 * fwd // 2
    for name, r in out.items():
        r["tf_per_s"] = round(flops / (r["ms"] * 1e-3) / 1e12, 2)
        r["fraction_of_2.5_pf"] = round(flops / (r["ms"] * 1e-3) / 2.5e15, 4)
        r["peak_bytes"] = peak[name]
    return {"S": S, "left_pad": pad, "flops_forward": fwd, "flops_forward_backward": flops, "mask_bytes_sdpa": full.numel(), "mask_bytes_hip": key.numel(),
            "max_abs_diff_of_gradients": diffs, "routes": out, "ratio_hip_over_sdpa": round(out["hip"]["ms"] / out["sdpa"]["ms"], 3)}


def bench_step(dev, reps: int, warmup: int, prefix: int) -> dict:
    import transformers as tf

    from mraudio_amd.models.lm_head import lm_head_ce
    from mraudio_amd.models.lora import apply_lora

    torch.manual_seed(0)
    cfg = tf.LlamaConfig(vocab_size=4096, hidden_size=1024, intermediate_size=2752, num_hidden_layers=4, num_attention_heads=8,
                         num_key_value_heads=8, max_position_embeddings=4096, pad_token_id=0, bos_token_id=1, eos_token_id=2)
    llm = tf.LlamaForCausalLM(cfg).to(dev).to(torch.bfloat16).requires_grad_(False)
    apply_lora(llm, r=8, alpha=8, dropout=0.05)
    llm.train()
    params = [p for p in llm.parameters() if p.requires_grad]
    B, answer = 2, 64
    embeds = (torch.randn(B, prefix, 1024, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 0.5).to(torch.bfloat16).requires_grad_(True)
    mask = torch.ones(B, prefix, dtype=torch.long, device=dev)
    mask[1, :prefix // 20] = 0
    targets = torch.randint(3, 4096, (B, prefix), device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    targets[:, :prefix - answer] = -100
    losses = {}

    def step(route):
        with (hip_train(llm) if route == "hip" else contextlib.nullcontext()):
            hidden = llm.get_decoder()(inputs_embeds=embeds, attention_mask=mask, return_dict=True).last_hidden_state
            loss = lm_head_ce(hidden, llm.lm_head.weight, targets)
        torch.autograd.grad(loss, [embeds] + params)
        losses[route] = loss.detach()

    peak = {r: _peak(lambda r=r: step(r)) for r in ("stock", "hip")}
    out = _alternate({r: (lambda r=r: step(r)) for r in ("stock", "hip")}, reps, warmup, 1)
    for r in out:
        out[r]["peak_bytes"] = peak[r]
    return {"layers": 4, "hidden": 1024, "heads": 8, "head_dim": 128, "B": B, "prefix": prefix, "labelled_rows": B * answer, "lora_r": 8, "lm_loss": "fused",
            "trainable_tensors": len(params), "routes": out, "loss": {r: round(v.item(), 5) for r, v in losses.items()},
            "ratio_hip_over_stock": round(out["hip"]["ms"] / out["stock"]["ms"], 3)}


def main(argv=None) -> None:
    global LIMIT
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--seqs", type=int, nargs="+", default=[1900, 2700, 5400])
    ap.add_argument("--prefix", type=int, default=1900)
    ap.add_argument("--step-limit", type=float, default=60.0, help="seconds a single timed step may take before the process is ended")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_lm_attention_bwd needs a GPU: a CPU timing says nothing about the kernels")
    LIMIT = args.step_limit
    dev = torch.device("cuda:0")
    line = {"metric": "lm_attention_bwd", "dtype": "bf16", "reps": args.reps, "warmup": args.warmup, "inner": args.inner,
            "note": "ms = median of reps between device events, routes alternating inside each repetition; attention: forward + backward per call over "
                    "`inner` back-to-back calls, B = 2, Hq = Hkv = 32, D = 128, TF/s on the executed causal flops (backward 2.5 x forward), the SDPA "
                    "route timed with its [B, 1, S, S] mask already built; step: forward + backward of the 4-layer Llama with LoRA and the fused head "
                    "+ loss; every section is measured anew by every run of this tool: a line holds one session",
            "attention": [bench_attention(dev, S, args.reps, args.warmup, args.inner) for S in args.seqs],
            "step": bench_step(dev, args.reps, 1, args.prefix)}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
