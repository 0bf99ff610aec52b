#!/usr/bin/env python3
"""cfg-G tiled-inference sweep, plain and with test-time augmentation, alternated in one process after a warm-up (prints one
JSON line): 8192^2 raster, 256^2 tiles at stride 128 (3 969 tiles), batch 32, the bench's model (3 channels, 64 start kernels,
depth 5, eval), tiles assembled by GpuGridTiles during the sweep.
  plain_tiles_per_s     the sweep as it is without tta
  tta_tiles_per_s       tiles per second under --tta (default d4: 8 forwards per tile)
  tta_samples_per_s     variant samples per second = tta_tiles_per_s x variants: what compares with plain_tiles_per_s
  samples_over_plain    their ratio (medians)
then, in a pass of its own without the model (kernel times are not taken from the timed rounds: the library's kernel timer,
rd_prof_*, puts HIP events around every launch), the assembly and blend of the first --kernel-batches batches of either sweep run
back to back on the sweep's raster: average duration of grid_tile_sums, grid_tile_write / grid_tile_write_aug and
blend_accumulate / blend_accumulate_tta, and the bandwidth of each from the bytes its algorithm needs: a write kernel reads and
writes 4 B per tile value (8 B); a blend reads 4 B per prediction value and reads + writes a double (16 B) per raster pixel that
the batch covers (the union of its tiles' squares, counted here on the host)."""
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
    ap.add_argument("--tta", default="d4")
    ap.add_argument("--kernel-batches", type=int, default=200)
    args = ap.parse_args()
    from resdepth_amd import GpuGridTiles, GpuPatchSampler, UNet, _lib, ops, predict_linear_blend, tiling
    dev = torch.device("cuda", 0)
    n, t = args.raster, 256
    g = torch.Generator().manual_seed(5)
    dsm = torch.randn(n, n, generator=g) * 4 + 420
    dsm[1000:1100, 2000:2300] = -9999.0
    orthos = torch.rand(2, n, n, generator=g) * 200 + 20
    smp = GpuPatchSampler(dsm, None, orthos, tile_size=t, nodata=-9999.0, dsm_std=3.0, ortho_mean=None, ortho_std=50.0, device=dev)
    area = {"x_extent": [(0, n - 1)], "y_extent": [(0, n - 1)]}
    plain = GpuGridTiles(smp, "test", area, "geom-stereo", [[0, 1]], batch_size=args.batch)
    tta = GpuGridTiles(smp, "test", area, "geom-stereo", [[0, 1]], batch_size=args.batch, tta=args.tta)
    variants = len(tta.dataset.tta)
    torch.manual_seed(0)
    model = UNet(n_input_channels=3, start_kernel=64, depth=5, bias_conv_layer=True).to(dev).eval()
    tiles = len(plain.dataset)

    def sweep(loader):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        predict_linear_blend(loader, model, host="reuse")
        torch.cuda.synchronize()
        return tiles / (time.perf_counter() - t0)

    sweep(plain), sweep(tta)                                       # warm-up: packed weights, allocator, pinned host raster
    a, b = [], []
    for _ in range(args.rounds):
        a.append(sweep(plain))
        b.append(sweep(tta))
    res = {"raster": n, "tile": t, "batch": args.batch, "tiles": tiles, "tta": args.tta, "variants": variants,
           "plain_tiles_per_s": [round(v, 1) for v in a], "tta_tiles_per_s": [round(v, 1) for v in b],
           "tta_samples_per_s": [round(v * variants, 1) for v in b],
           "samples_over_plain": round(float(np.median(b) * variants / np.median(a)), 4)}
    print(json.dumps(res), file=sys.stderr, flush=True)            # the sweep figures, should the kernel pass below fail

    ops_of = {"grid_tile_sums": "sums", "grid_tile_write": "write", "grid_tile_write_aug": "write", "blend_accumulate": "blend",
              "blend_accumulate_tta": "blend"}

    def kernels(loader):
        ds = loader.dataset
        g_ = len(ds.tta) if ds.tta else 1
        bounds = tiling.batch_bounds(len(ds), args.batch)[:args.kernel_batches]
        raster = torch.zeros(n, n, dtype=torch.float64, device=dev)
        pred = torch.randn(args.batch, 1, t, t, device=dev)
        std = torch.full((args.batch,), 3.0, device=dev)
        ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
        out = {}
        for timed in (False, True):                                # first pass: warm-up
            covered = values = 0
            _lib.prof_enable(2 if timed else 0)
            _lib.prof_reset()
            for k0, k1 in bounds:
                b = loader.assemble(k0, k1, ws)
                m = k1 - k0
                pos = torch.stack([b["patch_offset_y"], b["patch_offset_x"]], 1).to(torch.int32)
                reg = torch.stack([b[k] for k in ("patch_valid_pixels_uly", "patch_valid_pixels_ulx", "patch_valid_pixels_lry",
                                                  "patch_valid_pixels_lrx")], 1).to(torch.int32)
                ops.blend_accumulate(pred[:m], torch.nan_to_num(b["dsm_mean"]), std[:m], pos, reg, t, ds.stride, raster,
                                     aug=b.get("tta"), log2_variants=g_.bit_length() - 1)
                values += m * t * t
                if timed:
                    where = sorted(set(map(tuple, ds.pos[k0:k1])))
                    y0, x0 = min(y for y, _ in where), min(x for _, x in where)
                    cover = np.zeros((max(y for y, _ in where) + t - y0, max(x for _, x in where) + t - x0), dtype=bool)
                    for y, x in where:
                        cover[y - y0:y - y0 + t, x - x0:x - x0 + t] = True
                    covered += int(cover.sum())
            torch.cuda.synchronize()
            if timed:
                for e in _lib.prof_collect():
                    if e["name"] in ops_of and e["launches"]:
                        byts = {"sums": 4.0 * 3 * values, "write": 8.0 * 3 * values, "blend": 4.0 * values + 16.0 * covered}
                        out[e["name"]] = {"calls": int(e["launches"]), "us_per_call": round(e["ms"] * 1e3 / e["launches"], 2),
                                          "gb_per_s": round(byts[ops_of[e["name"]]] / (e["ms"] * 1e-3) / 1e9, 1)}
            _lib.prof_enable(0)
        return out
    res["kernel_batches"] = args.kernel_batches
    res["plain_kernels"], res["tta_kernels"] = kernels(plain), kernels(tta)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
