#!/usr/bin/env python3
"""What the co-registration costs (resdepth_amd.coregistration, include/resdepth_hip_coreg.h).  No pass / fail bar: the numbers go
to DESIGN.md 3.6d.

  rd_shift_sums          on an 8192^2 pair: time of the call (its two launches; device events around it, median and [min, max] of
                         --reps after a warm-up) and algorithmic bytes/s -- one read of the source, the reference and the class
                         byte of every pixel: 17 bytes with an f64 source, 13 with an f32 one (f64 reference, class bytes)
  rd_translate_bilinear  the same raster by a sub-pixel and by a whole-pixel shift: up to four taps read (32 bytes, f64) and one
                         double written per pixel, 40 bytes at most; 16 algorithmic bytes with every tap counted once
  rd_dsm_slope           on the same raster in the same run, for scale (4 or 8 bytes read, 8 written per pixel)
  coregister             end to end on a pair 0.7, -0.4 pixels and 1.5 m apart: the iterations, the resampling and the read-backs

Writes one JSON document (--out, default profiles/coreg.json).
    python scripts/coreg_bench.py [--size 8192] [--reps 7] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from resdepth_amd import _lib, coregistration as CR  # noqa: E402

NODATA = -9999.0
GSD = 0.5


def surface(x, y):
    return (400.0 + 30.0 * torch.sin(x / 97.0) * torch.cos(y / 61.0) + 8.0 * torch.sin((x + 2.0 * y) / 23.0)
            + 3.0 * torch.cos((2.0 * x - y) / 11.0))


def scene(n, dev, sx=0.7, sy=-0.4, sz=1.5, seed=0):
    """reference = a rolling surface on the grid, source = the same surface (sx, sy) pixels and sz away, 1 % nodata in each"""
    g = torch.Generator(device=dev).manual_seed(seed)
    i = torch.arange(n, device=dev, dtype=torch.float64)
    y, x = i[:, None], i[None, :]
    ref = surface(x, y)
    src = surface(x + sx, y + sy) - sz
    for t in (ref, src):
        t[torch.rand((n, n), generator=g, device=dev) < 0.01] = NODATA
    cls = (torch.rand((n, n), generator=g, device=dev) < 0.9).to(torch.uint8)
    return src, ref, cls


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
        d["algorithmic_bytes_per_pixel"] = nbytes
        d["algorithmic_GB_per_s"] = None       # filled by the caller, who knows the pixel count
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coreg.json"))
    a = ap.parse_args()
    n, dev = a.size, torch.device("cuda", 0)
    doc = {"raster": f"{n}x{n}", "device": torch.cuda.get_device_name(0), "reps": a.reps}
    lib = _lib.load()

    def rate(d):
        d["algorithmic_GB_per_s"] = round(d["algorithmic_bytes_per_pixel"] * n * n / d["median_ms"] / 1e6, 1)
        return d

    with torch.cuda.device(dev):
        src, ref, cls = scene(n, dev)
        src32 = src.float()
        nb = lib.rd_shift_sums_ws_bytes(n, n)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        out = torch.empty(10, dtype=torch.float64, device=dev)
        moved = torch.empty((n, n), dtype=torch.float64, device=dev)
        slope = torch.empty((n, n), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def sums(s, c, need):
            return lambda: _lib.check(lib.rd_shift_sums(
                s.data_ptr(), int(s.dtype == torch.float64), ref.data_ptr(), 1, c.data_ptr() if c is not None else None, need, n, n,
                NODATA, GSD, GSD, 0.0, 0.0, ws.data_ptr(), nb, out.data_ptr(), _lib.stream_ptr()), "shift_sums")

        def resample(s, tx, ty):
            return lambda: _lib.check(lib.rd_translate_bilinear(
                s.data_ptr(), int(s.dtype == torch.float64), n, n, NODATA, tx, ty, 1.5, float("nan"), moved.data_ptr(),
                _lib.stream_ptr()), "translate_bilinear")

        def horn(s):
            return lambda: _lib.check(lib.rd_dsm_slope(s.data_ptr(), int(s.dtype == torch.float64), n, n, NODATA, GSD, GSD,
                                                       slope.data_ptr(), _lib.stream_ptr()), "dsm_slope")

        doc["rd_dsm_slope"] = {"f32": rate(digest(timed(horn(src32), a.reps), 12.0)),
                               "f64": rate(digest(timed(horn(src), a.reps), 16.0))}
        doc["rd_shift_sums"] = {"f64_source_with_classes": rate(digest(timed(sums(src, cls, 1), a.reps), 17.0)),
                                "f32_source_with_classes": rate(digest(timed(sums(src32, cls, 1), a.reps), 13.0)),
                                "f64_source_no_classes": rate(digest(timed(sums(src, None, 0), a.reps), 16.0)),
                                "blocks": nb // 80, "tiles_per_block": -(-((n + 63) // 64) * ((n + 15) // 16) // (nb // 80))}
        doc["rd_translate_bilinear"] = {"f64_subpixel": rate(digest(timed(resample(src, 0.7, -0.4), a.reps), 16.0)),
                                        "f32_subpixel": rate(digest(timed(resample(src32, 0.7, -0.4), a.reps), 12.0)),
                                        "f64_whole_pixels": rate(digest(timed(resample(src, 1.0, -2.0), a.reps), 16.0)),
                                        "bytes_per_pixel_with_every_tap_counted": 40.0}
        slope_ms = doc["rd_dsm_slope"]["f32"]["median_ms"]
        doc["ratios_to_rd_dsm_slope_f32"] = {
            "rd_shift_sums_f32_source": round(doc["rd_shift_sums"]["f32_source_with_classes"]["median_ms"] / slope_ms, 2),
            "rd_shift_sums_f64_source": round(doc["rd_shift_sums"]["f64_source_with_classes"]["median_ms"] / slope_ms, 2),
            "rd_translate_bilinear_f32": round(doc["rd_translate_bilinear"]["f32_subpixel"]["median_ms"] / slope_ms, 2),
            "rd_translate_bilinear_f64": round(doc["rd_translate_bilinear"]["f64_subpixel"]["median_ms"] / slope_ms, 2),
            "bytes_rd_shift_sums_f32_source": round(13.0 / 12.0, 2), "bytes_rd_shift_sums_f64_source": round(17.0 / 12.0, 2)}

        run = lambda: CR.coregister(src32, ref, GSD, nodata=NODATA, mask=cls, tol=1e-4)      # noqa: E731
        doc["coregister_end_to_end"] = digest(timed(run, max(2, a.reps // 2)))
        res = run()
        doc["coregister_end_to_end"].update(
            iterations=len(res.history), converged=res.converged, px=list(res.shift.px), tz=res.shift.tz, count=res.shift.count,
            sigma0=res.shift.sigma0, truth={"px": [0.7, -0.4], "tz": 1.5},
            increments_px=[[h.px[0], h.px[1], h.tz] for h in res.history])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc), flush=True)


if __name__ == "__main__":
    main()
