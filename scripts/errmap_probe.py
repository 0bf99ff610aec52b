#!/usr/bin/env python3
"""What the error maps and the statistics by slope class cost (resdepth_amd.evaluation, include/resdepth_hip_errmap.h).  No
pass / fail bar: the numbers go to DESIGN.md 3.6b.

  rd_cell_stats   on an 8192^2 residual raster at cells 16, 64 and 256: time of the one launch (device events around it, median
                  and [min, max] of --reps after a warm-up) and algorithmic bytes/s -- 17 reads of every value and class byte
                  (the moments pass, 8 passes for the median and the absolute median, 8 for the NMAD) and one row per cell
  rd_dsm_slope    on the 8192^2 f32 ground truth: time and algorithmic bytes/s (4 bytes read, 8 written per pixel)
  evaluate_binned with 9 slope bins, end to end (classification, slope, bins, the engine's calls, the read-back)
  host route      for scale, at 2048^2 in the same process: the residuals and class bytes on the host and a numpy loop over the
                  cells of 64 calling the reference-pinned statistics (oracle/stats_oracle.py), beside rd_cell_stats there

Writes one JSON document (--out, default profiles/errmap.json).
    python scripts/errmap_probe.py [--size 8192] [--host-size 2048] [--reps 7] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import stats_oracle  # noqa: E402
from resdepth_amd import _lib, evaluation as E  # noqa: E402

NODATA = -9999.0
DEGREES = [0.0, 2.0, 5.0, 10.0, 15.0, 20.0, 30.0, 45.0, 60.0, 90.0]


def scene(n, dev, seed=0):
    """a rolling ground truth with 1 % nodata, an initial DSM with metre-scale and a refined one with decimetre-scale errors"""
    g = torch.Generator(device=dev).manual_seed(seed)
    y = torch.arange(n, device=dev, dtype=torch.float32)
    gt = 400.0 + 30.0 * torch.sin(y[:, None] / 97.0) * torch.cos(y[None, :] / 61.0) + torch.randn((n, n), generator=g, device=dev)
    gt[torch.rand((n, n), generator=g, device=dev) < 0.01] = NODATA
    init = gt + 2.0 * torch.randn((n, n), generator=g, device=dev)
    pred = (gt + 0.4 * torch.randn((n, n), generator=g, device=dev)).double()
    return pred, init, gt


def timed(fn, reps):
    """fn enqueues on the current stream -> [ms] of reps calls after one warm-up, each between two device events"""
    ms = []
    for k in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if k:
            ms.append(a.elapsed_time(b))
    return ms


def digest(ms, nbytes=None):
    d = {"median_ms": round(statistics.median(ms), 3), "min_max_ms": [round(min(ms), 3), round(max(ms), 3)]}
    if nbytes is not None:
        d["algorithmic_GB_per_s"] = round(nbytes / statistics.median(ms) / 1e6, 1)
    return d


def cell_call(r, cls, cell):
    rows, cols = cls.shape
    out = torch.empty((-(-rows // cell), -(-cols // cell), 8), dtype=torch.float64, device=r.device)
    lib = _lib.load()

    def fn():
        _lib.check(lib.rd_cell_stats(r.data_ptr(), cls.data_ptr(), rows, cols, cell, cell, E.VALID_AFTER, 0.0, out.data_ptr(),
                                     _lib.stream_ptr()), "cell_stats")
    return fn, out


def host_cells(r, cls, cell):
    """the route this replaces: a loop over the cells on the host"""
    rows, cols = cls.shape
    ok = (cls & E.VALID_AFTER) != 0
    out = np.full((-(-rows // cell), -(-cols // cell), 8), np.nan)
    for cy in range(out.shape[0]):
        for cx in range(out.shape[1]):
            win = (slice(cy * cell, (cy + 1) * cell), slice(cx * cell, (cx + 1) * cell))
            if ok[win].any():
                out[cy, cx] = list(stats_oracle.statistics(r[win].ravel(), ok[win].ravel()).values())
            else:
                out[cy, cx, 0] = 0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--host-size", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "errmap.json"))
    a = ap.parse_args()
    n, dev = a.size, torch.device("cuda", 0)
    doc = {"raster": f"{n}x{n}", "device": torch.cuda.get_device_name(0), "reps": a.reps}
    with torch.cuda.device(dev):
        pred, init, gt = scene(n, dev)
        _, r_after, cls, _ = E._classified(pred, init, gt, None, None, None, None, None, NODATA, dev, "errmap_probe")
        torch.cuda.synchronize()
        doc["rd_cell_stats"] = {}
        for cell in (16, 64, 256):
            fn, out = cell_call(r_after, cls, cell)
            d = digest(timed(fn, a.reps), 17.0 * 9.0 * n * n + 64.0 * out.shape[0] * out.shape[1])
            d["cells"] = out.shape[0] * out.shape[1]
            d["passes_over_the_raster"] = 17
            doc["rd_cell_stats"][f"cell_{cell}"] = d
        slope = torch.empty((n, n), dtype=torch.float64, device=dev)
        lib = _lib.load()
        doc["rd_dsm_slope"] = digest(timed(lambda: _lib.check(lib.rd_dsm_slope(
            gt.data_ptr(), 0, n, n, NODATA, 0.5, 0.5, slope.data_ptr(), _lib.stream_ptr()), "dsm_slope"), a.reps), 12.0 * n * n)
        binned = lambda: E.evaluate_binned(pred, init, gt, "slope", DEGREES, gsd=0.5, nodata=NODATA)     # noqa: E731
        doc["evaluate_binned_9_slope_bins"] = digest(timed(binned, a.reps))
        res = binned()
        doc["evaluate_binned_9_slope_bins"]["bins"] = [
            {"lo": b.lo, "hi": b.hi, "pixels": b.refined.count_total, "MAE_initial": b.initial.MAE, "MAE_refined": b.refined.MAE}
            for b in res]
        doc["evaluate_statistics_for_scale"] = digest(timed(lambda: E.evaluate_statistics(pred, init, gt, nodata=NODATA), a.reps))

        # for scale: the host loop at a size it finishes at, beside the kernel on the same window
        m = a.host_size
        rs, cs = r_after[:m, :m].contiguous(), cls[:m, :m].contiguous()
        fn, out = cell_call(rs, cs, 64)
        dev_ms = digest(timed(fn, a.reps))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rh, ch = rs.cpu().numpy(), cs.cpu().numpy()
        t1 = time.perf_counter()
        want = host_cells(rh, ch, 64)
        t2 = time.perf_counter()
        got = out.cpu().numpy()
        doc["host_route"] = {"raster": f"{m}x{m}", "cell": 64, "copy_ms": round((t1 - t0) * 1e3, 1),
                             "numpy_loop_ms": round((t2 - t1) * 1e3, 1), "rd_cell_stats": dev_ms,
                             "same_medians": bool(np.array_equal(got[..., [0, 1, 2, 5, 6]], want[..., [0, 1, 2, 5, 6]], equal_nan=True)),
                             "largest_MAE_RMSE_difference": float(np.nanmax(np.abs(got[..., 3:5] - want[..., 3:5])))}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc), flush=True)


if __name__ == "__main__":
    main()
