#!/usr/bin/env python3
"""cfg-G tiled-inference sweep over P image pairs, in one pass and as P single-pair sweeps, alternated in one process after a
warm-up (prints one JSON line): 8192^2 raster, 256^2 tiles at stride 128 (3 969 tiles), batch 32, the bench's model
(3 channels, 64 start kernels, depth 5, eval), tiles assembled by GpuGridTiles during the sweep, P = 4 pairs over four ortho
planes.
  one_pass_tiles_per_s   predict_pairs_linear_blend over GpuGridTiles(sweep_pairs=True), counting P forwards per tile, the
                         fuse (median + std) and the delivery of fused, spread and the P planes included
  baseline_tiles_per_s   P consecutive predict_linear_blend sweeps, one loader per pair: P x tiles over their total time
  one_pass_over_baseline their ratio (medians), and the min / max of either route over the rounds (the run-to-run spread)
then the fuse kernel alone (device events around --fuse-reps calls after a warm-up): GB/s of rd_fuse_planes for median + std at
P = 4 and P = 16 from the bytes its algorithm needs (8 P read + 16 written per pixel), beside rd_adam_step on 2^26 elements
(16 B read + 12 B written per element) in the same run, and their ratio; and the bytes a call brings to the host with and
without return_pairs (the size of the pinned block it fills)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--raster", type=int, default=8192)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--fuse-reps", type=int, default=10)
    ap.add_argument("--start-kernel", type=int, default=64)
    ap.add_argument("--depth", type=int, default=5)
    args = ap.parse_args()
    from resdepth_amd import GpuGridTiles, GpuPatchSampler, UNet, ops, predict_linear_blend, predict_pairs_linear_blend
    dev = torch.device("cuda", 0)
    n, t, p = args.raster, 256, args.pairs
    g = torch.Generator().manual_seed(5)
    dsm = torch.randn(n, n, generator=g) * 4 + 420
    dsm[n // 8:n // 8 + 100, n // 4:n // 4 + 300] = -9999.0
    orthos = torch.rand(4, n, n, generator=g) * 200 + 20
    smp = GpuPatchSampler(dsm, None, orthos, tile_size=t, nodata=-9999.0, dsm_std=3.0, ortho_mean=None, ortho_std=50.0, device=dev)
    area = {"x_extent": [(0, n - 1)], "y_extent": [(0, n - 1)]}
    pairs = [[k % 4, (k + 1 + k // 4) % 4] for k in range(p)]
    singles = [GpuGridTiles(smp, "test", area, "geom-stereo", [pr], batch_size=args.batch) for pr in pairs]
    swept = GpuGridTiles(smp, "test", area, "geom-stereo", pairs, batch_size=args.batch, sweep_pairs=True)
    torch.manual_seed(0)
    model = UNet(n_input_channels=3, start_kernel=args.start_kernel, depth=args.depth, bias_conv_layer=True).to(dev).eval()
    tiles = len(singles[0].dataset)
    assert len(swept.dataset) == p * tiles

    def one_pass(return_pairs=True):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = predict_pairs_linear_blend(swept, model, fuse="median", spread="std", return_pairs=return_pairs, host="reuse")
        torch.cuda.synchronize()
        return p * tiles / (time.perf_counter() - t0), res

    def baseline():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for ld in singles:
            predict_linear_blend(ld, model, host="reuse")
        torch.cuda.synchronize()
        return p * tiles / (time.perf_counter() - t0)

    one_pass(), one_pass(False), baseline()                       # warm-up: packed weights, allocator, pinned host memory
    a, b = [], []
    for _ in range(args.rounds):
        a.append(one_pass()[0])
        b.append(baseline())
    lean_rate, lean = one_pass(return_pairs=False)
    full = one_pass()[1]
    res = {"raster": n, "tile": t, "batch": args.batch, "tiles": tiles, "pairs": p,
           "one_pass_tiles_per_s": [round(v, 1) for v in a], "baseline_tiles_per_s": [round(v, 1) for v in b],
           "one_pass_over_baseline": round(float(np.median(a) / np.median(b)), 4),
           "one_pass_min_over_max": round(min(a) / max(a), 4), "baseline_min_over_max": round(min(b) / max(b), 4),
           "one_pass_no_pairs_tiles_per_s": round(lean_rate, 1),
           "host_bytes_with_pairs": int(full.host.t.numel() * 8), "host_bytes_without_pairs": int(lean.host.t.numel() * 8),
           "host_bytes_baseline": int(p * n * n * 8)}
    print(json.dumps(res), file=sys.stderr, flush=True)            # the sweep figures, should the kernel pass below fail
    del full, lean

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps

    px = n * n
    fused, spread = torch.empty(n, n, dtype=torch.float64, device=dev), torch.empty(n, n, dtype=torch.float64, device=dev)
    fuse = {}
    for q in (4, 16):
        planes = torch.randn(q, n, n, device=dev).to(torch.float64) * 3 + 400
        s = timed(lambda: ops.fuse_planes(planes, "median", "std", fused_out=fused, spread_out=spread), args.fuse_reps)
        fuse[q] = {"ms": round(s * 1e3, 3), "gb_per_s": round(px * 8.0 * (q + 2) / s / 1e9, 1)}
        del planes
    m = 1 << 26
    w, gr, m1, m2 = (torch.randn(m, device=dev) for _ in range(4))
    m2.abs_()
    s = timed(lambda: ops.adam_step(w, gr, m1, m2, 0.9, 0.999, 1e-8, 0.0, 1e-4, 1.0), args.fuse_reps)
    adam = {"ms": round(s * 1e3, 3), "gb_per_s": round(m * 28.0 / s / 1e9, 1)}
    res["fuse_median_std"] = {"P4": fuse[4], "P16": fuse[16], "adam_step": adam,
                              "P4_over_adam": round(fuse[4]["gb_per_s"] / adam["gb_per_s"], 3),
                              "P16_over_adam": round(fuse[16]["gb_per_s"] / adam["gb_per_s"], 3)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
