"""A/B of the LM decode's one-token attention (mraudio_amd/models/lm_decode.py):

  (a) kernel   ``decode_attention(hip=True)`` (``mra_decode_attention``: two launches) against ``scaled_dot_product_attention`` with one
               query row and a bool ``[B, 1, 1, S]`` mask on the same tensors: B = 2, Hq = Hkv = 32, D = 128, bf16 (one layer of a Vicuna-7B
               shape), S in {1900, 5400} (the prefix the prompt assembler builds at T = 20 / T = 60).  ms per call and TB/s on the
               algorithmic bytes 2 * B * Hkv * S * D * 2 (K and V read once).
  (b) generate 64 greedy tokens of a 4-layer Llama (hidden 1024, 8 heads of 128: the model of tools/bench_lora.py) behind a prefix of 1900
               embedded positions, B = 2, on four routes: stock (``generate`` as it comes: a growing cache, SDPA), static (stock attention
               over a static cache, ``disable_compile``), hip (``hip_decode``: the static cache with the one-token attention on HIP) and
               hip_step (``HipLmDecoder``: the LM's own prefill, then one ``mra_lm_step`` per token).
  (c) layer    ms per token of ``mra_lm_step`` alone on ONE 7B-shaped layer with random weights (hidden 4096, intermediate 11008, 32 heads of
               128, a 64-token vocabulary so that the head does not count, 21 cached keys: slot 20) at B = 1, 2 and 8, beside the same seven products as
               ``F.linear`` calls; bytes streamed = the seven weight matrices once, TB/s and the fraction of 8 TB/s on them.

ms = median of ``--reps`` repetitions between device events, the routes alternating inside each repetition, one process; (a) times
``--inner`` back-to-back calls per repetition.  One JSON line on stdout, also written to ``--out`` (profiles/lm_decode_line.json is such a line).

    python tools/bench_lm_decode.py --out profiles/lm_decode_line.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mraudio_amd.models.lm_decode import decode_attention, hip_decode  # noqa: E402
from mraudio_amd.models.lm_step import HipLmDecoder, rope_table, step_workspace_bytes  # noqa: E402


def _time(fn, inner: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


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
    q = torch.randn(B, H, 1, D, device=dev, dtype=torch.bfloat16, generator=gen)
    k = torch.randn(B, H, S, D, device=dev, dtype=torch.bfloat16, generator=gen)
    v = torch.randn(B, H, S, D, device=dev, dtype=torch.bfloat16, generator=gen)
    mask = torch.ones(B, 1, 1, S, dtype=torch.bool, device=dev)
    mask[1, :, :, :37] = False
    scale = D ** -0.5
    routes = {"sdpa": lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask, scale=scale),
              "hip": lambda: decode_attention(q, k, v, mask, scale, hip=True)}
    diff = (routes["hip"]().float() - routes["sdpa"]().float()).abs().max().item()
    out = _alternate(routes, reps, warmup, inner)
    nbytes = 2 * B * H * S * D * 2
    for r in out.values():
        r["tb_per_s"] = round(nbytes / (r["ms"] * 1e-3) / 1e12, 3)
    return {"S": S, "bytes": nbytes, "max_abs_diff": round(diff, 5), "routes": out, "ratio_hip_over_sdpa": round(out["hip"]["ms"] / out["sdpa"]["ms"], 3)}


def bench_generate(dev, reps: int, warmup: int, prefix: int, new_tokens: int) -> dict:
    import transformers as tf

    torch.manual_seed(0)
    cfg = tf.LlamaConfig(vocab_size=4096, hidden_size=1024, intermediate_size=2752, num_hidden_layers=4, num_attention_heads=8,
                         num_key_value_heads=8, max_position_embeddings=4096, pad_token_id=0, bos_token_id=1, eos_token_id=2)
    llm = tf.LlamaForCausalLM(cfg).to(dev).to(torch.bfloat16).eval().requires_grad_(False)
    B = 2
    embeds = (torch.randn(B, prefix, 1024, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 0.5).to(torch.bfloat16)
    mask = torch.ones(B, prefix, dtype=torch.long, device=dev)
    mask[1, :37] = 0
    kw = dict(inputs_embeds=embeds, attention_mask=mask, max_new_tokens=new_tokens, min_new_tokens=new_tokens, do_sample=False)
    tokens = {}

    def stock():
        tokens["stock"] = llm.generate(**kw)

    def static():
        tokens["static"] = llm.generate(cache_implementation="static", disable_compile=True, **kw)

    def hip():
        with hip_decode(llm):
            tokens["hip"] = llm.generate(cache_implementation="static", disable_compile=True, **kw)

    dec = HipLmDecoder(llm)

    def hip_step():
        tokens["hip_step"] = dec.generate(embeds, mask, new_tokens, ignore_eos=True)

    with torch.no_grad():
        out = _alternate({"stock": stock, "static": static, "hip": hip, "hip_step": hip_step}, reps, warmup, 1)
    n = tokens["stock"].numel()
    return {"layers": 4, "hidden": 1024, "heads": 8, "head_dim": 128, "B": B, "prefix": prefix, "new_tokens": new_tokens, "routes": out,
            "tokens_equal_to_stock": {k: f"{int((tokens[k] == tokens['stock']).sum())}/{n}" for k in ("static", "hip", "hip_step")},
            "ratio_hip_over_stock": round(out["hip"]["ms"] / out["stock"]["ms"], 3), "ratio_hip_over_static": round(out["hip"]["ms"] / out["static"]["ms"], 3),
            "ratio_hip_step_over_stock": round(out["hip_step"]["ms"] / out["stock"]["ms"], 3)}


def bench_layer(dev, reps: int, warmup: int, inner: int) -> dict:
    import ctypes as C

    import transformers as tf

    from mraudio_amd._lib import check, current_stream, lib

    torch.manual_seed(0)
    H, I, heads, D, V, Smax, slot = 4096, 11008, 32, 128, 64, 64, 20
    cfg = tf.LlamaConfig(vocab_size=V, hidden_size=H, intermediate_size=I, num_hidden_layers=1, num_attention_heads=heads,
                         num_key_value_heads=heads, max_position_embeddings=4096, pad_token_id=0, bos_token_id=1, eos_token_id=2)
    llm = tf.LlamaForCausalLM(cfg).to(dev).to(torch.bfloat16).eval().requires_grad_(False)
    layer = llm.model.layers[0]
    Ws = [layer.self_attn.q_proj.weight, layer.self_attn.k_proj.weight, layer.self_attn.v_proj.weight, layer.self_attn.o_proj.weight,
          layer.mlp.gate_proj.weight, layer.mlp.up_proj.weight, layer.mlp.down_proj.weight]
    nbytes = sum(w.numel() * 2 for w in Ws)
    dec = HipLmDecoder(llm)
    rows = []
    for B in (1, 2, 8):
        cache = (torch.randn(1, 2, B, heads, Smax, D, device=dev) * 0.1).to(torch.bfloat16)
        mask8 = torch.ones(B, Smax, dtype=torch.uint8, device=dev)
        position = torch.full((B,), slot, dtype=torch.int32, device=dev)
        rope = rope_table(llm, Smax + 1, dev)
        h = torch.empty(B, H, dtype=torch.bfloat16, device=dev)
        logits = torch.empty(B, V, dtype=torch.float32, device=dev)
        ws = torch.empty(step_workspace_bytes(B, H, I, heads, D, Smax), dtype=torch.uint8, device=dev)
        tin = torch.arange(B, dtype=torch.int32, device=dev)
        tout = torch.empty(B, dtype=torch.int32, device=dev)
        d = dec.descriptor(B, cache, mask8, position, rope, h, logits, None, ws, 0, [])
        d.slot, d.pos_offset, d.tokens_in, d.tokens_out = slot, 0, tin.data_ptr(), tout.data_ptr()
        step, stream = lib().mra_lm_step, current_stream()
        x, act = torch.randn(B, H, device=dev).to(torch.bfloat16), torch.randn(B, I, device=dev).to(torch.bfloat16)
        lin = torch.nn.functional.linear
        routes = {"mra_lm_step": lambda: check(step(C.byref(d), stream), "mra_lm_step"),
                  "f_linear_x7": lambda: [lin(x, w) for w in Ws[:6]] + [lin(act, Ws[6])]}
        out = _alternate(routes, reps, warmup, inner)
        for r in out.values():
            r["tb_per_s"] = round(nbytes / (r["ms"] * 1e-3) / 1e12, 3)
            r["fraction_of_8_tb_per_s"] = round(nbytes / (r["ms"] * 1e-3) / 8e12, 3)
        rows.append({"B": B, "routes": out, "ratio_step_over_f_linear": round(out["mra_lm_step"]["ms"] / out["f_linear_x7"]["ms"], 3)})
    return {"hidden": H, "intermediate": I, "heads": heads, "head_dim": D, "weight_bytes": nbytes, "cached_keys": slot + 1,
            "launches_per_step": 8 * cfg.num_hidden_layers + 4, "rows": rows}


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--seqs", type=int, nargs="+", default=[1900, 5400])
    ap.add_argument("--prefix", type=int, default=1900)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_lm_decode needs a GPU: a CPU timing says nothing about the kernels")
    dev = torch.device("cuda:0")
    line = {"metric": "lm_decode", "dtype": "bf16", "reps": args.reps, "warmup": args.warmup, "inner": args.inner,
            "note": "ms = median of reps between device events, routes alternating inside each repetition; kernel: per call over `inner` "
                    "back-to-back calls, B = 2, Hq = Hkv = 32, D = 128, TB/s on 2 * B * Hkv * S * D * 2 bytes; generate: per call of 64 greedy tokens; "
                    "every section is measured anew by every run of this tool: a line holds one session; layer: per mra_lm_step call (one 7B-shaped layer + a 64-token head) over `inner` back-to-back calls, TB/s on the seven weight matrices",
            "kernel": [bench_kernel(dev, S, args.reps, args.warmup, args.inner) for S in args.seqs],
            "generate": bench_generate(dev, args.reps, 1, args.prefix, args.new_tokens),
            "layer": bench_layer(dev, args.reps, args.warmup, args.inner)}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
