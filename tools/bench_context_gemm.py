"""Stand-alone timing of the folded cross-attention's per-head context GEMM (step 6e: ctx = U_h W_v,h^T + b_v,h, batch = heads) on the tiles
the existing kernel families offer, through ``mra_debug_gemm`` with the forward's descriptor.  Headline shape by default: M = 1024 query
rows, N = 64, K = 1408, 12 heads.  Per candidate: 20 launches between two events, best and median of ``--rounds`` rounds.

    python tools/bench_context_gemm.py --rounds 7

Prints one JSON line: per candidate the tile, the family that ran, workgroups, us per launch."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GT_64, GT_K128_64x128, EPI_OP = 1, 6, 0
CANDIDATES = (("64x128 k128 (present)", GT_K128_64x128, 0, 128), ("64x64 two-buffer", GT_64, 0, 64), ("64x64 k128 (cross_fuse bit 4)", GT_64, 1, 64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=32)
    ap.add_argument("--width", type=int, default=1408)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    from mraudio_amd import _lib as L

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    Q, heads, K, M = 32, args.heads, args.width, args.items * 32
    g = torch.Generator(device=dev).manual_seed(3)
    u = torch.randn(args.items, heads * Q, K, generator=g, device=dev).half()
    wv = (torch.randn(heads * 64, K, generator=g, device=dev) * 0.05).half()
    bv = torch.randn(heads * 64, generator=g, device=dev)
    ctx = torch.empty(M, heads * 64, device=dev, dtype=torch.float16)
    nb = lambda t: t.numel() * t.element_size()
    out, ref = {}, None
    for name, tile, k128, rows in CANDIDATES:
        d = L.mra_gemm_desc()
        d.struct_bytes = ctypes.sizeof(L.mra_gemm_desc)
        d.A, d.a_bytes, d.W, d.w_bytes, d.bias, d.bias_bytes, d.C, d.c_bytes = u.data_ptr(), nb(u), wv.data_ptr(), nb(wv), bv.data_ptr(), nb(bv), ctx.data_ptr(), nb(ctx)
        d.a_view[:] = (heads * Q * K, Q, K)
        d.c_view[:] = (0, M, heads * 64)
        d.M, d.N, d.K, d.batch = M, 64, K, heads
        d.a_bs, d.w_bs, d.c_bs_bytes, d.bias_bs = Q * K, 64 * K, 128, 64
        d.tile_cfg, d.k128 = tile, k128
        fams = range(L.GEMM_FAMILIES)
        before = [L.gemm_launches(f, EPI_OP) for f in fams]

        def launch():
            L.check(L.lib().mra_debug_gemm(d, 1, EPI_OP, L.MRA_F16, L.current_stream()), name)

        launch()
        torch.cuda.synchronize()
        family = [f for f, b in zip(fams, before) if L.gemm_launches(f, EPI_OP) > b]
        if ref is None:
            ref = ctx.clone()
        us = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                launch()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) / 20 * 1e3)
        out[name] = {"tile": tile, "k128": k128, "family": family, "workgroups": -(-M // rows) * heads, "us_best": round(min(us), 2),
                     "us_median": round(statistics.median(us), 2), "bit_identical_to_present": bool(torch.equal(ctx, ref))}
    print(json.dumps({"shape": {"M": M, "N": 64, "K": K, "batch": heads}, "candidates": out}), flush=True)


if __name__ == "__main__":
    main()
