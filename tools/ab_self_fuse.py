"""A/B of ``mra_qformer_set_option("self_fuse", value)`` on the flagship step, in ONE process: bench.py's clip32x32 workload (32 clips, video
Kv 8224 x 1408, audio Kv 496 x 768, seeded weights and inputs as bench.py builds them), the values taken in turn for several rounds so that
clock and thermal drift meet every value alike (the style of tools/ab_cross_fuse.py).

    python tools/ab_self_fuse.py --values 0 1 --rounds 4 --steps 20 --warmup 2

Prints one JSON line: per value the ms / step of every round, their median and range.  ``--check`` also compares the step's outputs of every
value with those of the first one, bit for bit."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def flatten(out, prefix=""):
    """the step's outputs (tensors, or dicts of tensors per modality) as {name: clone}"""
    flat = {}
    for k, v in out.items():
        if torch.is_tensor(v):
            flat[prefix + k] = v.detach().clone()
        elif isinstance(v, dict):
            flat.update(flatten(v, prefix + k + "_"))
    return flat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--values", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--text-len", type=int, default=32)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    from mraudio_amd.models.xinstructblip import ENC_WIDTH, XInstructBLIP

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    model = XInstructBLIP(seed=0, perturb=False, op_dtype=torch.float16, device=dev)
    kv = {"video": 32 * 257, "audio": 496}
    g = torch.Generator(device=dev).manual_seed(1234)
    feats = {m: torch.randn(args.clips, kv[m], ENC_WIDTH[m], generator=g, device=dev, dtype=torch.float16) for m in ("video", "audio")}
    ids = torch.randint(1000, 30000, (args.clips, args.text_len), generator=g, device=dev)
    tmask = torch.ones(args.clips, args.text_len, dtype=torch.long, device=dev)

    def step():
        return model.fuse_score(feats, ids, tmask, bs=1, num=args.clips)

    def set_value(value):
        for m in ("video", "audio"):
            getattr(model, f"{m}_Qformer").set_option("self_fuse", value)

    for value in args.values:   # lazy one-time work of every form
        set_value(value)
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    ms = {value: [] for value in args.values}
    outs = {}
    for _ in range(args.rounds):
        for value in args.values:
            set_value(value)
            for _ in range(args.warmup):
                out = step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                out = step()
            torch.cuda.synchronize()
            ms[value].append((time.perf_counter() - t0) / args.steps * 1e3)
            outs[value] = flatten(out)
    line = {"workload": "clip32x32", "steps": args.steps, "rounds": args.rounds,
            "self_fuse": {str(value): {"ms_per_step": [round(v, 4) for v in ms[value]], "median": round(statistics.median(ms[value]), 4),
                                  "min": round(min(ms[value]), 4), "max": round(max(ms[value]), 4)} for value in args.values}}
    if args.check:
        first = outs[args.values[0]]
        line["bit_identical_to_first_value"] = {str(value): all(torch.equal(outs[value][k], first[k]) for k in first) for value in args.values[1:]}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
