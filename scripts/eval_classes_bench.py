#!/usr/bin/env python3
"""GPU time of the class-partitioned evaluation (resdepth_amd.evaluation.evaluate_statistics) on an 8192^2 raster resident
in HBM with all four masks, two stripes and a residual threshold (20 statistics sets), against the same 20 sets through
20 single-set calls (resdepth_amd.evaluation.get_statistics: 10 calls with a threshold), and rd_dilate_mask (k = 2) alone.
Each: warm-up, then the median of 10 calls timed with HIP events.  Prints one JSON line.
    python scripts/eval_classes_bench.py [--size 8192] [--reps 10]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from resdepth_amd import _lib  # noqa: E402
from resdepth_amd.evaluation import (CLASS_BITS, VALID_AFTER, VALID_BEFORE, _evaluate, evaluate_statistics,  # noqa: E402
                                     get_statistics)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    n = a.size
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    gt = torch.randn(n, n, device=dev, generator=g, dtype=torch.float32) * 5 + 400
    init = gt + torch.randn(n, n, device=dev, generator=g) * 1.1
    pred = gt.double() + torch.randn(n, n, device=dev, generator=g, dtype=torch.float64) * 0.6
    for t, p in ((gt, 0.01), (init, 0.01), (pred, 0.01)):
        t[torch.rand(n, n, device=dev, generator=g) < p] = -9999.0

    def mask(p):
        return (torch.rand(n, n, device=dev, generator=g) < p).to(torch.uint8)

    masks = dict(mask_gt=(mask(0.92), 255.0), mask_building=(mask(0.04), 255.0), mask_water=(mask(0.1), 255.0),
                 mask_forest=(mask(0.15), 255.0))
    area = {"x_extent": [(0, n - 1), (n // 4, 3 * n // 4)], "y_extent": [(0, n // 3), (n // 2, n - 1)]}
    thr = 2.5

    def run_sets():
        return evaluate_statistics(pred, init, gt, area, residual_threshold=thr, nodata=-9999.0, **masks)

    # the 20 sets through the single-set kernel: explicit per-class masks (from one classification pass, untimed)
    _, _, cls, classes = _evaluate(pred, init, gt, area, masks["mask_gt"], masks["mask_building"], masks["mask_water"],
                                   masks["mask_forest"], thr, -9999.0, dev)
    explicit = []
    for c in classes:
        for raster, valid in ((init, VALID_BEFORE), (pred, VALID_AFTER)):
            need = valid | CLASS_BITS[c]
            explicit.append((raster, ((cls & need) == need).to(torch.uint8)))

    def run_single():
        for raster, m in explicit:
            get_statistics(raster, gt, -9999.0, m, thr)

    lib = _lib.load()
    bmask = masks["mask_building"][0].contiguous()
    bout = torch.empty_like(bmask)

    def run_dilate():
        _lib.check(lib.rd_dilate_mask(bmask.data_ptr(), bout.data_ptr(), n, n, 2, _lib.stream_ptr()), "dilate_mask")

    st = run_sets()
    t_sets, t_single, t_dil = timed(run_sets, a.reps), timed(run_single, a.reps), timed(run_dilate, a.reps)
    print(json.dumps({"raster": f"{n}x{n}", "sets": 2 * len(classes) * 2, "evaluate_statistics_ms": round(t_sets[0], 3),
                      "evaluate_statistics_ms_min_max": [round(t_sets[1], 3), round(t_sets[2], 3)],
                      "single_set_calls_ms": round(t_single[0], 3), "single_set_calls": len(explicit) * 2,
                      "speedup": round(t_single[0] / t_sets[0], 2), "dilate_k2_ms": round(t_dil[0], 4),
                      "after_all_MAE": st.after.all.MAE, "after_all_NMAD": st.after.all.NMAD}))


if __name__ == "__main__":
    main()
