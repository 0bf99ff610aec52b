#!/usr/bin/env python3
"""What error quantiles and within-tolerance shares cost (resdepth_amd.evaluation, include/resdepth_hip_dist.h) on an 8192^2
raster with the five classes (10 statistics sets per side with a residual threshold), and for the pair sweep at P = 4:

  plain      evaluate_statistics(...) / evaluate_pairs_statistics(...) without options: the eight numbers
  options    the same call with abs_quantiles=LE, within=(1, 2)
  parent     (with --parent-lib: a build of the commit before the feature) the plain call through that library -- the same
             launches, so the same time within the run-to-run spread

The variants alternate call by call in ONE process; each call is timed with device events on its stream (it ends in a read-back,
so the host clock agrees) after a warm-up round; median and [min, max] of --reps rounds.  Then the library's profiler over one
call with options: the time of the eight-number call's kernels and of the quantile call's, next to what the schedule predicts --
a group of <= 20 selectors is eight histogram passes over the values; 10 sets x 3 quantiles are 2 groups beside the 2 groups
the medians take (20 median / absolute-median selectors, 10 NMAD selectors), plus one counting pass beside the moments pass
(evaluate_statistics scores 20 sets in one call: 3 groups beside 3).
Last, for context, the route this replaces: the residual raster and the class bytes copied to the host, np.quantile and a count
per class there.  Writes one JSON document (--out, default profiles/dist_stats.json).
    python scripts/dist_probe.py [--size 8192] [--planes 4] [--reps 7] [--parent-lib PATH] [--out PATH]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eval_pairs_bench import NODATA, THR, scene  # noqa: E402
from resdepth_amd import _lib, evaluation as E  # noqa: E402

WITHIN = (1.0, 2.0)


def other_library(path):
    """a second build of the library, bound like _lib.load() binds the first (the symbols it has)"""
    lib = ctypes.CDLL(path)
    tables = [getattr(_lib, name) for name in dir(_lib) if name.startswith("SIGNATURES")]
    for table in tables:
        for name, (res, args) in table.items():
            if hasattr(lib, name):
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = res, args
    return lib


class through:
    """the evaluation module's calls go through `lib` inside the block (None: the package's own library)"""

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        self.saved = E.load
        if self.lib is not None:
            E.load = lambda: self.lib

    def __exit__(self, *exc):
        E.load = self.saved


def alternate(variants, reps):
    """variants {name: fn}: a warm-up round, then reps rounds in which every variant runs once, the order rotated round by round
    (a call's time depends a little on what ran before it) -> {name: [ms per round]}"""
    ms = {k: [] for k in variants}
    names = list(variants)
    for rnd in range(reps + 1):
        for name in names[rnd % len(names):] + names[:rnd % len(names)]:
            fn = variants[name]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rnd:
                ms[name].append(a.elapsed_time(b))
    return ms


def summary(ms):
    return {k: {"median_ms": round(statistics.median(v), 2), "min_max_ms": [round(min(v), 2), round(max(v), 2)]} for k, v in ms.items()}


def profile(fn, lib=None):
    """the kernel classes of one call of fn, timed by the profiler of the library it runs through"""
    lib = lib or _lib.load()
    lib.rd_prof_enable(2)
    lib.rd_prof_reset()
    fn()
    torch.cuda.synchronize()
    arr = (_lib.ProfEntry * 64)()
    n = lib.rd_prof_collect(ctypes.cast(arr, ctypes.c_void_p), 64)
    lib.rd_prof_enable(0)
    return {arr[i].name.decode(): round(arr[i].ms, 3) for i in range(n)}


def host_route(r_after, cls, classes):
    """the residuals and class bytes to the host, np.quantile and a count per class there"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    data, bits = r_after.cpu().numpy(), cls.cpu().numpy()
    t1 = time.perf_counter()
    out = {}
    for c in classes:
        need = E.VALID_AFTER | E.CLASS_BITS[c]
        a = np.abs(data[(bits & need) == need])
        out[c] = ([float(v) for v in np.quantile(a, E.LE)] if a.size else None, [float((a <= t).mean()) if a.size else None for t in WITHIN])
    t2 = time.perf_counter()
    return {"copy_ms": round((t1 - t0) * 1e3, 1), "quantile_ms": round((t2 - t1) * 1e3, 1), "total_ms": round((t2 - t0) * 1e3, 1)}, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--planes", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dist_stats.json"))
    a = ap.parse_args()
    n, dev = a.size, torch.device("cuda", 0)
    parent = other_library(a.parent_lib) if a.parent_lib else None
    pairs, init, gt, masks, area = scene(n, a.planes, dev)
    opts = dict(abs_quantiles=E.LE, within=WITHIN)
    doc = {"raster": f"{n}x{n}", "device": torch.cuda.get_device_name(0), "rd_version": _lib.load().rd_version(),
           "parent_rd_version": parent.rd_version() if parent else None, "reps": a.reps, "options": "abs_quantiles=LE, within=(1, 2)"}

    def single(lib=None, **kw):
        with through(lib):
            return E.evaluate_statistics(pairs[0], init, gt, area, residual_threshold=THR, nodata=NODATA, **masks, **kw)

    def sweep(lib=None, **kw):
        with through(lib):
            return E.evaluate_pairs_statistics(pairs, init, gt, area, residual_threshold=THR, nodata=NODATA, **masks, **kw)

    def passes(n_sets, n_q=3):
        """reads of the values by one eight-number call and by one quantile call over n_sets sets: the moments / counting pass and
        eight histogram passes per group of <= 20 selectors (medians: 2 per set, then the NMADs; quantiles: n_q per set)"""
        groups = lambda k: -(-k // 20)                                    # noqa: E731
        return 1 + 8 * (groups(2 * n_sets) + groups(n_sets)), 1 + 8 * groups(n_q * n_sets)

    # evaluate_statistics: one call over 20 sets (initial and refined DSM x 5 classes x plain / truncated); the sweep: calls of 10
    for key, fn, n_sets in (("evaluate_statistics", single, 20), (f"evaluate_pairs_statistics_P{a.planes}", sweep, 10)):
        variants = {"plain": fn, "options": lambda fn=fn: fn(**opts)}
        if parent is not None:
            variants = {"parent": lambda fn=fn: fn(parent), **variants}
        t = summary(alternate(variants, a.reps))
        prof = profile(lambda fn=fn: fn(**opts))
        if parent is not None:
            t["parent_kernel_ms"] = profile(lambda fn=fn: fn(parent), parent)
        eight = sum(v for k, v in prof.items() if k.startswith("residual_stats_"))
        dist = sum(v for k, v in prof.items() if k.startswith("residual_dist_"))
        p8, pq = passes(n_sets)
        t.update(added_ms=round(t["options"]["median_ms"] - t["plain"]["median_ms"], 2), kernel_ms=prof,
                 eight_number_kernels_ms=round(eight, 3), quantile_kernels_ms=round(dist, 3),
                 schedule={"sets_per_call": n_sets, "eight_number_passes": p8, "quantile_passes": pq,
                           "predicted_quantile_over_eight": round(pq / p8, 3),
                           "measured_quantile_over_eight": round(dist / eight, 3) if eight else None})
        doc[key] = t

    st = single(**opts)
    _, r_after, cls, classes = E._evaluate(pairs[0], init, gt, area, masks["mask_gt"], masks["mask_building"], masks["mask_water"],
                                           masks["mask_forest"], THR, NODATA, dev)
    host_route(r_after[:1024], cls[:1024], classes)                      # numpy's first call
    t_host, got = host_route(r_after, cls, classes)
    worst = max(abs(st.after[c].abs_quantile[lv] - v) for c in classes if got[c][0] for lv, v in zip(E.LE, got[c][0]))
    same = all(st.after[c].within[t] == w for c in classes for t, w in zip(WITHIN, got[c][1]) if w is not None)
    doc["host_sort_route"] = dict(t_host, what="r_after + class bytes to the host, np.quantile(|r|, LE) and two counts per class",
                                  largest_quantile_difference_m=worst, same_shares=bool(same))
    doc["after_all"] = {"LE68": st.after.all.abs_quantile[0.68], "LE90": st.after.all.abs_quantile[0.9],
                        "LE95": st.after.all.abs_quantile[0.95], "within_1m": st.after.all.within[1.0],
                        "within_2m": st.after.all.within[2.0]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc), flush=True)


if __name__ == "__main__":
    main()
