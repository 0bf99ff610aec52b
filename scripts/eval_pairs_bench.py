#!/usr/bin/env python3
"""Wall time of scoring every pair plane of a sweep and the pool of all pairs (resdepth_amd.evaluation.
evaluate_pairs_statistics on device-resident planes) on an 8192^2 raster with all four masks, two stripes and a residual
threshold, at P = 4 and P = 8, against the route without it on the same data: per plane one classification of host arrays
(evaluation._evaluate, what evaluate_statistics / evaluate_performance run) with the residual and class rasters brought back,
the per-class compression and concatenation on the host (test.py:235-313), and get_statistics_masked per class.
Then the library's own profiler (rd_prof_*) over one call of the new route: time per kernel class, per histogram pass of one
plane and of the pool, the bytes a pass reads, and the same pooled passes with ONE statistics set (3 selectors instead of 30)
-- a pass that does not get cheaper with fewer bytes but does with fewer selectors is bound by the per-selector VALU / LDS
work.  Wall times: a host clock around calls that end in a device synchronise, warm-up first, the median of --reps calls
(--old-reps for the old route, which takes tens of seconds).  Prints one JSON line per P.
    python scripts/eval_pairs_bench.py [--size 8192] [--planes 4 8] [--reps 5] [--old-reps 2]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from resdepth_amd import _lib  # noqa: E402
from resdepth_amd.evaluation import (CLASS_BITS, VALID_AFTER, _evaluate, _Rows, evaluate_pairs_statistics,  # noqa: E402
                                     get_statistics_masked)

NODATA, THR = -9999.0, 2.5


def wall(fn, reps):
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ms), 2), [round(min(ms), 2), round(max(ms), 2)]


def scene(n, n_planes, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    gt = torch.randn(n, n, device=dev, generator=g, dtype=torch.float32) * 5 + 400
    init = gt + torch.randn(n, n, device=dev, generator=g) * 1.1
    pairs = torch.empty(n_planes, n, n, device=dev, dtype=torch.float64)
    for p in range(n_planes):
        pairs[p] = gt.double() + torch.randn(n, n, device=dev, generator=g, dtype=torch.float64) * (0.5 + 0.05 * p)
        pairs[p][torch.rand(n, n, device=dev, generator=g) < 0.01] = NODATA
    for t in (gt, init):
        t[torch.rand(n, n, device=dev, generator=g) < 0.01] = NODATA

    def mask(p):
        return (torch.rand(n, n, device=dev, generator=g) < p).to(torch.uint8)

    masks = dict(mask_gt=(mask(0.92), 255.0), mask_building=(mask(0.04), 255.0), mask_water=(mask(0.1), 255.0),
                 mask_forest=(mask(0.15), 255.0))
    area = {"x_extent": [(0, n - 1), (n // 4, 3 * n // 4)], "y_extent": [(0, n // 3), (n // 2, n - 1)]}
    return pairs, init, gt, masks, area


def old_route(pairs_h, init_h, gt_h, masks_h, area, dev):
    """P x (classify host arrays, residual + class rasters back), compress + concatenate per class, statistics per class"""
    pool, classes = None, None
    per_pair = []
    for plane in pairs_h:
        st, r_after, cls, classes = _evaluate(plane, init_h, gt_h, area, masks_h["mask_gt"], masks_h["mask_building"],
                                              masks_h["mask_water"], masks_h["mask_forest"], THR, NODATA, dev)
        per_pair.append(st)
        data, bits = r_after.cpu().numpy(), cls.cpu().numpy()
        pool = pool or {c: [] for c in classes}
        for c in classes:
            need = VALID_AFTER | CLASS_BITS[c]
            pool[c].append(data[(bits & need) == need])
    pooled = {c: get_statistics_masked(np.concatenate(pool[c]), THR, device=dev) for c in classes}
    return per_pair, pooled


def profile(fn):
    _lib.prof_enable(2)
    _lib.prof_reset()
    fn()
    torch.cuda.synchronize()
    out = {e["name"]: e for e in _lib.prof_collect()}
    _lib.prof_enable(0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--planes", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--old-reps", type=int, default=2)
    a = ap.parse_args()
    n = a.size
    dev = torch.device("cuda", 0)
    for n_planes in a.planes:
        pairs, init, gt, masks, area = scene(n, n_planes, dev)

        def new():
            return evaluate_pairs_statistics(pairs, init, gt, area, residual_threshold=THR, nodata=NODATA, **masks)

        st = new()                                                        # warm-up
        t_new = wall(new, a.reps)
        prof = profile(new)
        # the pooled passes with one set: same bytes, 3 selectors instead of 30
        res = pairs - gt.double()
        cls = torch.full((n, n), 8 | 16 | 32, dtype=torch.uint8, device=dev)
        prof1 = profile(lambda: _Rows(1, None, dev).pooled(res, n_planes, 0, n_planes, cls, None, [(0, None)]))
        del res, cls

        pairs_h, init_h, gt_h = pairs.cpu().numpy(), init.cpu().numpy(), gt.cpu().numpy()
        masks_h = {k: (v.cpu().numpy(), nd) for k, (v, nd) in masks.items()}
        k = min(1024, n)                                                  # warm-up of the old route's kernels on a corner
        old_route(pairs_h[:2, :k, :k], init_h[:k, :k], gt_h[:k, :k], {q: (v[:k, :k], nd) for q, (v, nd) in masks_h.items()},
                  None, dev)
        old = []
        t_old = wall(lambda: old.append(old_route(pairs_h, init_h, gt_h, masks_h, area, dev)), a.old_reps)
        per_pair, pooled = old[-1]
        same = all(abs(pooled[c][q] - st.pooled[c][q]) <= 1e-12 * max(1.0, abs(pooled[c][q])) for c in pooled
                   for q in ("count_total", "MAE", "RMSE", "median", "NMAD")) and \
            all(per_pair[p].after[c]["median"] == st.pairs[p][c]["median"] for p in range(n_planes) for c in pooled)

        ns = 10                                                           # 5 classes x (full, truncated)
        passes = 8 * (-(-2 * ns // 20) + -(-ns // 20))                    # histogram passes of one call
        one, pool = prof[f"residual_stats_pooled|select x1"], prof[f"residual_stats_pooled|select x{n_planes}"]
        pool1 = prof1[f"residual_stats_pooled|select x{n_planes}"]
        px = float(n) * n
        row = {"raster": f"{n}x{n}", "planes": n_planes, "new_ms": t_new[0], "new_ms_min_max": t_new[1],
               "old_route_ms": t_old[0], "old_route_ms_min_max": t_old[1], "speedup": round(t_old[0] / t_new[0], 1),
               "same_statistics": bool(same),
               "kernel_ms": {name: round(e["ms"], 3) for name, e in sorted(prof.items())},
               "plane_pass_ms": round(one["ms"] / (one["launches"] * passes), 4),
               "plane_pass_bytes": px * 11, "plane_pass_GBps": round(px * 11 / (one["ms"] / (one["launches"] * passes)) / 1e6, 1),
               "pooled_pass_ms": round(pool["ms"] / (pool["launches"] * passes), 4),
               "pooled_pass_bytes": px * (8 * n_planes + 3),
               "pooled_pass_GBps": round(px * (8 * n_planes + 3) / (pool["ms"] / (pool["launches"] * passes)) / 1e6, 1),
               "pooled_pass_over_planes_x_plane_pass": round(pool["ms"] / pool["launches"] /
                                                             (n_planes * one["ms"] / one["launches"]), 3),
               "pooled_pass_one_set_ms": round(pool1["ms"] / (pool1["launches"] * 16), 4),
               "pooled_all_MAE": st.pooled.all.MAE, "pooled_all_NMAD": st.pooled.all.NMAD}
        print(json.dumps(row), flush=True)
        del pairs, pairs_h, old, per_pair, pooled
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
