#!/usr/bin/env python3
"""cfg-G tiled-inference sweep fed three ways, alternated in one process after a warm-up (prints one JSON line):
  (a) resident: every batch of the sweep assembled beforehand and kept in HBM (the bench's convention: staging excluded);
  (b) grid:     GpuGridTiles assembling each batch from the resident rasters during the sweep (prefetch 1);
  (c) host:     a DataLoader over the numpy stand-in of the reference's __getitem__ (tests/grid_tiles_ref.py), `--workers`
                worker processes (spawned: they never open the GPU), pinned -- what a reference-style feed delivers.
8192^2 raster, 256^2 tiles at stride 128, batch 32, the bench's model (3 channels, 64 start kernels, depth 5, eval).
`--only grid --gt` traces the two assembly kernels with rocprofv3 while they overlap the sweep; `--only assemble --gt` runs them
alone, batch after batch (no model), for their isolated kernel times."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


class SharedStandIn(torch.utils.data.Dataset):
    """The stand-in over rasters in shared memory (torch tensors: spawned workers map them instead of copying 800 MB)."""

    def __init__(self, dsm, orthos_hwv, pos, reg, tile, stride, pair):
        self.dsm, self.orthos = dsm.share_memory_(), orthos_hwv.share_memory_()
        self.pos, self.reg, self.pair = pos, reg, pair
        self.tile_size, self.stride, self.raster_shape = tile, stride, tuple(dsm.shape)

    def __len__(self):
        return len(self.pos)

    def __getitem__(self, i):
        import grid_tiles_ref as R
        ds = R.StandInGridDataset(self.dsm.numpy(), None, self.orthos.numpy(), self.pos, self.reg, [self.pair] * len(self.pos),
                                  self.tile_size, self.stride, -9999.0, 3.0, None, 50.0, "geom-stereo")
        return ds[i]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--raster", type=int, default=8192)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--only", choices=["all", "grid", "assemble"], default="all")
    ap.add_argument("--gt", action="store_true", help="a ground-truth raster too (target + loss mask per tile)")
    args = ap.parse_args()
    from resdepth_amd import GpuGridTiles, GpuPatchSampler, UNet, predict_linear_blend
    dev = torch.device("cuda", 0)
    n, t = args.raster, 256
    g = torch.Generator().manual_seed(5)
    dsm = torch.randn(n, n, generator=g) * 4 + 420
    dsm[1000:1100, 2000:2300] = -9999.0
    orthos = torch.rand(2, n, n, generator=g) * 200 + 20
    gt = dsm + torch.randn(n, n, generator=g) if args.gt else None
    smp = GpuPatchSampler(dsm, gt, orthos, tile_size=t, nodata=-9999.0, dsm_std=3.0, ortho_mean=None, ortho_std=50.0, device=dev)
    area = {"x_extent": [(0, n - 1)], "y_extent": [(0, n - 1)]}
    grid = GpuGridTiles(smp, "test", area, "geom-stereo", [[0, 1]], batch_size=args.batch)
    torch.manual_seed(0)
    model = UNet(n_input_channels=3, start_kernel=64, depth=5, bias_conv_layer=True).to(dev).eval()
    tiles = len(grid.dataset)

    def sweep(loader):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = predict_linear_blend(loader, model)
        torch.cuda.synchronize()
        return tiles / (time.perf_counter() - t0), out

    res = {"raster": n, "tile": t, "batch": args.batch, "tiles": tiles, "gt": bool(args.gt)}
    if args.only == "assemble":
        from resdepth_amd import tiling
        bounds = tiling.batch_bounds(tiles, args.batch)
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k0, k1 in bounds:
                grid.assemble(k0, k1)
            torch.cuda.synchronize()
            res.setdefault("assemble_ms_per_batch", []).append(round((time.perf_counter() - t0) / len(bounds) * 1e3, 4))
        b = grid.assemble(0, args.batch)
        res["bytes_per_batch"] = int(sum(v.numel() * v.element_size() for k, v in b.items() if k in ("input", "target", "loss_mask"))
                                     + args.batch * t * t * 4 * (3 + args.gt))      # written once + raster planes read once
        print(json.dumps(res), flush=True)
        return
    if args.only == "grid":
        for _ in range(args.rounds):
            res.setdefault("grid_tiles_per_s", []).append(round(sweep(grid)[0], 1))
        print(json.dumps(res), flush=True)
        return

    class Resident(list):
        dataset = grid.dataset
    resident = Resident(grid)
    torch.cuda.synchronize()
    sweep(resident), sweep(grid)                                   # warm-up
    a, b = [], []
    for _ in range(args.rounds):
        ra, out_a = sweep(resident)
        rb, out_b = sweep(grid)
        a.append(round(ra, 1))
        b.append(round(rb, 1))
    res.update(resident_tiles_per_s=a, grid_tiles_per_s=b, grid_over_resident=round(float(np.median(b) / np.median(a)), 4),
               max_abs_diff_m=float(np.abs(out_a - out_b).max()))
    print(json.dumps(res), flush=True)
    del resident
    torch.cuda.empty_cache()
    ds = SharedStandIn(dsm, orthos.permute(1, 2, 0).contiguous(), grid.dataset.pos, grid.dataset.reg, t, grid.dataset.stride,
                       [0, 1])
    host = torch.utils.data.DataLoader(ds, batch_size=args.batch, shuffle=False, num_workers=args.workers, pin_memory=True,
                                       persistent_workers=True, multiprocessing_context="spawn", prefetch_factor=4)
    sweep(host)                                                    # warm-up: worker start
    rc, out_c = sweep(host)
    res.update(host_workers=args.workers, host_tiles_per_s=round(rc, 1), host_max_abs_diff_m=float(np.abs(out_c - out_b).max()))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
