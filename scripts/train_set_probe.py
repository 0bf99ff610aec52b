#!/usr/bin/env python3
"""Measurements of the training set and its statistics on one GPU; prints one JSON line per part.
  --part moments   rd_patch_moments over 20 000 random 256^2 patches of an 8192^2 raster, rd_patch_sums over the same positions
                   (same bytes: the baseline), the numpy stand-in on 200 of them, rd_region_moments over three planes x one 60 %
                   rectangle.  Kernel times: HIP events around `--reps` back-to-back calls after a warm-up, median of `--rounds`.
  --part loop      the cfg-S Trainer loop (bench.py's model and optimiser, batch 32) fed by GpuTrainSet over one raster, over
                   two rasters, and by SamplerLoader, alternated in one process, `--rounds` repeats each: tiles/s medians, the
                   ratio to SamplerLoader and SamplerLoader's own spread.
  --part assemble  rd_assemble_train_patches alone, batch after batch (no model), against GpuPatchSampler.random_batch."""
import argparse
import json
import os
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, reps, rounds):
    """median over `rounds` of the HIP-event time of `reps` back-to-back calls, in ms per call"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return float(np.median(out)), [round(v, 4) for v in out]


def rasters(n, dev, k=0, gt=True):
    from resdepth_amd import GpuPatchSampler
    g = torch.Generator().manual_seed(5 + k)
    dsm = torch.randn(n, n, generator=g) * 4 + 420
    dsm[1000:1100, 2000:2300] = -9999.0
    orthos = torch.rand(3, n, n, generator=g) * 200 + 20
    tgt = dsm + torch.randn(n, n, generator=g) if gt else None
    return GpuPatchSampler(dsm, tgt, orthos, tile_size=256, nodata=-9999.0, dsm_std=3.0, ortho_mean=110.0, ortho_std=50.0, device=dev)


def part_moments(args, dev):
    import train_set_ref as R
    from resdepth_amd import normalization as N
    from resdepth_amd._lib import check, load, ptr, stream_ptr
    n, t, m = args.raster, 256, args.patches
    smp = rasters(n, dev, gt=False)
    rng = np.random.RandomState(1)
    pos = np.stack([rng.randint(0, n - t + 1, m), rng.randint(0, n - t + 1, m)], 1)
    res = {"part": "moments", "raster": n, "tile": t, "patches": m, "bytes": 4.0 * m * t * t}
    lib = load()
    pos_d = torch.as_tensor(pos, dtype=torch.int32).to(dev)
    out = torch.empty(m, 3, dtype=torch.float64, device=dev)
    ws = torch.empty(lib.rd_patch_moments_ws_bytes(m, t), dtype=torch.uint8, device=dev)
    zero = torch.zeros(m, dtype=torch.int32, device=dev)
    sums = torch.empty(m, 2, dtype=torch.float64, device=dev)
    mom = lambda: check(lib.rd_patch_moments(ptr(smp.dsm_in), n, n, ptr(pos_d), m, t, -9999.0, 1, ptr(out), ptr(ws), ws.numel(),  # noqa: E731
                                             stream_ptr()))
    base = lambda: check(lib.rd_patch_sums(ptr(smp.dsm_in), n * n, ptr(zero), 1, ptr(pos_d), m, t, n, -9999.0, 1, ptr(sums),      # noqa: E731
                                           stream_ptr()))
    for name, fn in (("patch_moments", mom), ("patch_sums", base)):
        ms, all_ms = timed(fn, args.reps, args.rounds)
        res[name] = {"ms": round(ms, 4), "rounds_ms": all_ms, "tb_per_s": round(res["bytes"] / ms / 1e9, 3)}
    res["moments_over_sums"] = round(res["patch_moments"]["ms"] / res["patch_sums"]["ms"], 3)
    # 32 patches: does a small list fill the device?
    ms, _ = timed(lambda: check(lib.rd_patch_moments(ptr(smp.dsm_in), n, n, ptr(pos_d), 32, t, -9999.0, 1, ptr(out), ptr(ws), ws.numel(),
                                                     stream_ptr())), args.reps, args.rounds)
    res["patch_moments_32"] = {"ms": round(ms, 4), "tb_per_s": round(4.0 * 32 * t * t / ms / 1e9, 3)}
    t0 = time.perf_counter()
    value = N.compute_local_dsm_std_per_centered_patch([(smp, pos)])
    res["compute_local_dsm_std_s"] = round(time.perf_counter() - t0, 4)
    res["dsm_std"] = value
    plane = smp.dsm_in.cpu().numpy()
    t0 = time.perf_counter()
    ref = R.patch_stds(plane, pos[:200], t, -9999.0)
    dt = time.perf_counter() - t0
    got = np.sqrt(out[:200, 2].cpu().numpy() / (out[:200, 0].cpu().numpy() - 1))
    res["numpy_stand_in"] = {"s_for_200": round(dt, 3), "scaled_to_all_s": round(dt * m / 200, 1),
                             "max_rel_diff": float(np.abs(got / ref - 1).max())}
    print(json.dumps(res), flush=True)
    # region moments: three planes x one 60 % rectangle
    import ctypes as C
    rows = int(n * 0.6)
    rects = (C.c_int * 4)(0, rows, 0, n)
    planes = (C.c_int * 3)(0, 1, 2)
    need = lib.rd_region_moments_ws_bytes(n, n, 3, rects, 1)
    ws2 = torch.empty(need, dtype=torch.uint8, device=dev)
    out2 = torch.empty(3, dtype=torch.float64, device=dev)
    reg = lambda: check(lib.rd_region_moments(ptr(smp.orthos), n * n, 3, n, n, planes, 3, rects, 1, ptr(out2), ptr(ws2), ws2.numel(),  # noqa: E731
                                              stream_ptr()))
    ms, all_ms = timed(reg, max(1, args.reps // 2), args.rounds)
    nbytes = 4.0 * 3 * rows * n
    o = out2.cpu().numpy()
    res = {"part": "region", "planes": 3, "rect": [rows, n], "bytes": nbytes, "ms": round(ms, 4), "rounds_ms": all_ms,
           "tb_per_s": round(nbytes / ms / 1e9, 3), "mean": o[1], "std": float(np.sqrt(o[2] / o[0]))}
    print(json.dumps(res), flush=True)


def part_assemble(args, dev):
    from resdepth_amd import GpuTrainSet
    smp = rasters(args.raster, dev)
    area = {"x_extent": [(0, args.raster - 1)], "y_extent": [(0, int(args.raster * 0.6))]}
    ts = GpuTrainSet([dict(sampler=smp, area_defn=area, n_samples=2048, image_pairs=[[0, 1], [1, 2]])], "geom-stereo", args.batch,
                     generator=torch.Generator().manual_seed(1), rng=np.random.RandomState(1))
    tabs = ts.epoch_tables()[:32]
    g = torch.Generator().manual_seed(2)
    k = [0]

    def mine():
        ts._assemble(tabs[k[0] % len(tabs)])
        k[0] += 1
    ms_a, r_a = timed(mine, 32, args.rounds)
    ms_b, r_b = timed(lambda: smp.random_batch(args.batch, [0, 1], generator=g), 32, args.rounds)
    nbytes = args.batch * 256 * 256 * (4.0 * 4 * 2 + 1 + 4.0 * 3)
    print(json.dumps({"part": "assemble", "batch": args.batch, "train_set_ms_per_batch": round(ms_a, 4), "rounds": r_a,
                      "sampler_ms_per_batch": round(ms_b, 4), "sampler_rounds": r_b, "bytes_per_batch": nbytes,
                      "train_set_tb_per_s": round(nbytes / ms_a / 1e9, 3)}), flush=True)


def part_loop(args, dev):
    import bench
    from resdepth_amd import FusedAdam, GpuTrainSet, SamplerLoader, Trainer, UNet
    wl = bench.WORKLOADS["S"]
    n, bs, iters = args.raster, args.batch, args.iters
    s0, s1 = rasters(n, dev, 0), rasters(n, dev, 1)
    area = {"x_extent": [(0, n - 1)], "y_extent": [(0, int(n * 0.6))]}
    mk = lambda ss: GpuTrainSet([dict(sampler=s, area_defn=area, n_samples=iters * bs // len(ss), image_pairs=[[0, 1], [1, 2]])  # noqa: E731
                                 for s in ss], "geom-stereo", bs, permute_images_within_pair=True,
                                generator=torch.Generator().manual_seed(3), rng=np.random.RandomState(3), prefetch=args.prefetch)
    loaders = {"sampler_loader": SamplerLoader(s0, iters, bs, [0, 1], generator=torch.Generator().manual_seed(3), prefetch=args.prefetch),
               "train_set_1": mk([s0]), "train_set_2": mk([s0, s1])}
    torch.manual_seed(0)
    model = UNet(n_input_channels=wl["c"], start_kernel=64, depth=wl["depth"], bias_conv_layer=True).to(dev).train()
    opt = FusedAdam(model.parameters(), lr=2e-4, weight_decay=1e-5)
    tmp = tempfile.mkdtemp(prefix="rd_train_set_probe_")
    a = types.SimpleNamespace(model=model, optimizer=opt, scheduler=None, criterion=torch.nn.L1Loss(reduction="mean"),
                              trainloader=loaders["sampler_loader"], valloader=None, n_epochs=1, evaluate_rate=1,
                              save_model_rate=10 ** 9, freq_average_train_loss=10 ** 9, save_dir=tmp, log_file=None,
                              checkpoint_dir=os.path.join(tmp, "ck"), tboard_log_dir=os.path.join(tmp, "tb"), pretrained_path=None)
    tr = Trainer(a)
    tr.logger.handlers.clear()
    res = {"part": "loop", "batch": bs, "iterations": iters, "prefetch": args.prefetch, "tiles_per_s": {k: [] for k in loaders}}
    for rnd in range(args.rounds + 1):                         # round 0 warms every loader up
        for name, loader in loaders.items():
            tr.loader["train"] = loader
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.inference_one_epoch(rnd, "train")
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rnd:
                res["tiles_per_s"][name].append(round(len(loader) * bs / dt, 1))
    t0 = time.perf_counter()
    loaders["train_set_2"].epoch_tables()
    res["epoch_tables_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    med = {k: float(np.median(v)) for k, v in res["tiles_per_s"].items()}
    base = res["tiles_per_s"]["sampler_loader"]
    res["median"] = med
    res["ratio_to_sampler_loader"] = {k: round(v / med["sampler_loader"], 4) for k, v in med.items()}
    res["sampler_loader_spread"] = round((max(base) - min(base)) / med["sampler_loader"], 4)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["moments", "loop", "assemble"], default="moments")
    ap.add_argument("--raster", type=int, default=8192)
    ap.add_argument("--patches", type=int, default=20000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--prefetch", type=int, default=1)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    {"moments": part_moments, "loop": part_loop, "assemble": part_assemble}[args.part](args, dev)


if __name__ == "__main__":
    main()
