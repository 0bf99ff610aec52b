#!/usr/bin/env python3
"""A validation epoch (eval forward + masked L1 per batch, no host sync inside the epoch) over TWO rasters fed three ways,
alternated in one process after a warm-up (prints one JSON line):
  (a) resident: every batch assembled beforehand and kept in HBM (staging excluded);
  (b) valset:   one GpuValSet over both rasters, each batch one rd_assemble_train_patches call on the side stream (prefetch 1);
  (c) grids:    two GpuGridTiles ('val'), one per raster, run back to back (rd_assemble_grid_tiles).
Two 4096^2 rasters, 256^2 tiles at stride 256, batch 32, the bench's model (3 channels, 64 start kernels, depth 5, eval).
`--only assemble` runs GpuValSet's two kernels alone, batch after batch (no model), `--only assemble-grid` those of the two
GpuGridTiles: for isolated kernel times under rocprofv3 --kernel-trace --stats."""
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
    ap.add_argument("--raster", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=["all", "assemble", "assemble-grid"], default="all")
    args = ap.parse_args()
    from resdepth_amd import GpuGridTiles, GpuPatchSampler, GpuValSet, UNet, masked_l1_loss, tiling
    dev = torch.device("cuda", 0)
    n, t = args.raster, 256
    g = torch.Generator().manual_seed(5)
    datasets = []
    for k in range(2):
        dsm = torch.randn(n, n, generator=g) * 4 + 420 + 100 * k
        dsm[1000:1100, 2000:2300] = -9999.0
        gt = dsm + torch.randn(n, n, generator=g)
        orthos = torch.rand(2, n, n, generator=g) * 200 + 20
        smp = GpuPatchSampler(dsm, gt, orthos, tile_size=t, nodata=-9999.0, dsm_std=3.0 + k, ortho_mean=None, ortho_std=50.0 - 5 * k,
                              device=dev)
        datasets.append(dict(sampler=smp, area_defn={"x_extent": [(0, n - 1)], "y_extent": [(0, n - 1)]}, image_pairs=[[k, 1 - k]]))
    val = GpuValSet(datasets, "geom-stereo", batch_size=args.batch)
    grids = [GpuGridTiles(d["sampler"], "val", d["area_defn"], "geom-stereo", d["image_pairs"], batch_size=args.batch) for d in datasets]
    tiles = len(val.dataset)
    assert tiles == sum(len(x.dataset) for x in grids)
    res = {"raster": n, "tile": t, "batch": args.batch, "tiles": tiles}
    if args.only != "all":
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if args.only == "assemble":
                for k in range(len(val)):
                    val.assemble(k)
            else:
                for x in grids:
                    for k0, k1 in tiling.batch_bounds(len(x.dataset), args.batch):
                        x.assemble(k0, k1)
            torch.cuda.synchronize()
            res.setdefault("assemble_ms_per_batch", []).append(round((time.perf_counter() - t0) / len(val) * 1e3, 4))
        print(json.dumps(res), flush=True)
        return
    torch.manual_seed(0)
    model = UNet(n_input_channels=3, start_kernel=64, depth=5, bias_conv_layer=True).to(dev).eval()

    def epoch(loaders):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        total = torch.zeros((), dtype=torch.float64, device=dev)
        with torch.no_grad():
            for loader in loaders:
                for b in loader:
                    y = model(b["input"])
                    total += masked_l1_loss(y, b["target"], b["loss_mask"], b["dsm_mean"], b["dsm_std"]).double()
        torch.cuda.synchronize()
        return tiles / (time.perf_counter() - t0), float(total)

    resident = list(val)
    torch.cuda.synchronize()
    for feed in ([resident], [val], grids):                        # warm-up
        epoch(feed)
    a, b, c = [], [], []
    for _ in range(args.rounds):
        ra, la = epoch([resident])
        rb, lb = epoch([val])
        rc, lc = epoch(grids)
        a.append(round(ra, 1))
        b.append(round(rb, 1))
        c.append(round(rc, 1))
    med = lambda v: float(np.median(v))      # noqa: E731
    res.update(resident_tiles_per_s=a, valset_tiles_per_s=b, grids_tiles_per_s=c, valset_over_resident=round(med(b) / med(a), 4),
               grids_over_resident=round(med(c) / med(a), 4), valset_over_grids=round(med(b) / med(c), 4),
               loss_sums=[la, lb, lc])
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
