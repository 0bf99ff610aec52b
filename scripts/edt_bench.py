#!/usr/bin/env python3
"""What the distance transform costs (resdepth_amd.morphology, include/resdepth_hip_edt.h).  No pass / fail bar: the numbers go to
DESIGN.md 3.6e.

On a --size^2 raster (default 8192), per input: the time of rd_edt_sq with idx (its three launches; device events around the call,
median and [min, max] of --reps after a warm-up), the split into the column pass (edt_band_kernel + edt_column_kernel) and the row
pass (edt_row_kernel) from the library's own event pairs (rd_prof_*, a run of its own), and algorithmic bytes over time as a
fraction of 8 TB/s.  Algorithmic bytes per pixel: the mask read (1), the offsets written and read (4 + 4), d2 and idx written
(4 + 4) = 17; what the kernels move is 25 (the column pass keeps its in-band rows in d2's storage: one more write and read).

  (a) building_mask   random axis-aligned rectangles at about 20 % cover
  (b) complement      the same bytes with invert=1, as edge_distance calls it
  (c) corner_pixel    a single set pixel in a corner: the worst case, every search runs the length of the row
  (d) fill_voids      a DSM with about 5 % voids in round blobs: rd_edt_sq on the void mask + rd_fill_nearest, and the front end
                      as a whole (the void mask and the allocations included)

Where scipy is installed, scipy.ndimage.distance_transform_edt(..., return_indices=True) on the same masks on the host is timed
once each, as context (--no-scipy skips it).  Writes one JSON document (--out, default profiles/edt.json).
    python scripts/edt_bench.py [--size 8192] [--reps 7] [--out PATH] [--no-scipy]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from resdepth_amd import _lib, morphology as M  # noqa: E402

HBM_BYTES_PER_S = 8e12
ALGORITHMIC_BYTES = 17.0
MOVED_BYTES = 25.0


def rectangles(n, dev, cover=0.2, seed=0):
    """random axis-aligned rectangles with sides of 20..120 pixels -> uint8 mask (a difference array summed twice)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    count = int(-torch.log(torch.tensor(1.0 - cover)).item() * n * n / 70.0 ** 2)
    y0, x0 = (torch.randint(0, n, (count,), generator=g, device=dev) for _ in range(2))
    h, w = (torch.randint(20, 121, (count,), generator=g, device=dev) for _ in range(2))
    y1, x1 = (y0 + h).clamp(max=n), (x0 + w).clamp(max=n)
    diff = torch.zeros((n + 1, n + 1), dtype=torch.int32, device=dev)
    one = torch.ones(count, dtype=torch.int32, device=dev)
    for ys, xs, sign in ((y0, x0, 1), (y0, x1, -1), (y1, x0, -1), (y1, x1, 1)):
        diff.index_put_((ys, xs), one * sign, accumulate=True)
    return (diff.cumsum(0).cumsum(1)[:n, :n] > 0).to(torch.uint8).contiguous()


def blobs(n, dev, seed=1):
    """round void blobs of 40 and 20 pixels radius, about 5 % of the raster -> bool mask (discs by buffer_mask itself)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.zeros((n, n), dtype=torch.bool, device=dev)
    for radius, count in ((40, n * n // 170000), (20, n * n // 85000)):
        seeds = torch.zeros((n, n), dtype=torch.uint8, device=dev)
        seeds.view(-1)[torch.randint(0, n * n, (count,), generator=g, device=dev)] = 1
        out |= M.buffer_mask(seeds, radius)
    return out


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


def digest(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_max_ms": [round(min(ms), 3), round(max(ms), 3)]}


def passes(fn, reps):
    """the library's event pairs around its kernel classes, per call -> {class: digest}"""
    per = {}
    _lib.prof_enable(2)
    try:
        for k in range(reps + 1):
            _lib.prof_reset()
            fn()
            torch.cuda.synchronize()
            for e in _lib.prof_collect():
                if k:
                    per.setdefault(e["name"], []).append(e["ms"])
    finally:
        _lib.prof_enable(0)
        _lib.prof_reset()
    return {name: digest(ms) for name, ms in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edt.json"))
    ap.add_argument("--no-scipy", action="store_true")
    a = ap.parse_args()
    n, dev = a.size, torch.device("cuda", 0)
    lib = _lib.load()
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    if a.no_scipy:
        ndimage = None
    doc = {"raster": f"{n}x{n}", "device": torch.cuda.get_device_name(0), "reps": a.reps, "band_rows": _lib.EDT_BAND_ROWS,
           "algorithmic_bytes_per_pixel": ALGORITHMIC_BYTES, "moved_bytes_per_pixel": MOVED_BYTES, "inputs": {}}

    with torch.cuda.device(dev):
        nb = lib.rd_edt_ws_bytes(n, n)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        d2 = torch.empty((n, n), dtype=torch.int32, device=dev)
        idx = torch.empty((n, n), dtype=torch.int32, device=dev)

        def edt(mask, invert):
            return lambda: _lib.check(lib.rd_edt_sq(mask.data_ptr(), invert, n, n, d2.data_ptr(), idx.data_ptr(), ws.data_ptr(), nb,
                                                    _lib.stream_ptr()), "edt_sq")

        def measure(name, mask, invert, reps):
            call = edt(mask, invert)
            d = {"set_fraction": round(float(((mask != 0) != bool(invert)).double().mean()), 6), "rd_edt_sq": digest(timed(call, reps))}
            split = passes(call, max(2, reps // 2))
            d["column_pass"], d["row_pass"] = split["edt_columns"], split["edt_rows"]
            sec = d["rd_edt_sq"]["median_ms"] / 1e3
            d["algorithmic_GB_per_s"] = round(ALGORITHMIC_BYTES * n * n / sec / 1e9, 1)
            d["fraction_of_8_TB_per_s"] = round(ALGORITHMIC_BYTES * n * n / sec / HBM_BYTES_PER_S, 4)
            d["bytes_bound_ms"] = round(ALGORITHMIC_BYTES * n * n / HBM_BYTES_PER_S * 1e3, 3)
            call()
            d["max_distance_px"] = round(float(d2.max()) ** 0.5, 1)
            if ndimage is not None:
                host = ((mask != 0) != bool(invert)).cpu().numpy()
                t0 = time.perf_counter()
                ndimage.distance_transform_edt(~host, return_indices=True)
                d["scipy_host_s"] = round(time.perf_counter() - t0, 2)
            doc["inputs"][name] = d
            print(name, json.dumps(d), flush=True)

        buildings = rectangles(n, dev)
        measure("building_mask", buildings, 0, a.reps)
        measure("complement", buildings, 1, a.reps)
        corner = torch.zeros((n, n), dtype=torch.uint8, device=dev)
        corner[0, 0] = 1
        measure("corner_pixel", corner, 0, max(2, a.reps // 3))

        i = torch.arange(n, device=dev, dtype=torch.float32)
        dsm = 400.0 + 30.0 * torch.sin(i[None, :] / 97.0) * torch.cos(i[:, None] / 61.0)
        void = blobs(n, dev)
        dsm[void] = -9999.0
        void_u8 = void.to(torch.uint8)
        out = torch.empty_like(dsm)

        def kernels():
            edt(void_u8, 1)()
            _lib.check(lib.rd_fill_nearest(dsm.data_ptr(), 0, d2.data_ptr(), idx.data_ptr(), n * n, M.NO_CAP, out.data_ptr(),
                                           _lib.stream_ptr()), "fill_nearest")

        d = {"void_fraction": round(float(void.double().mean()), 6), "kernels": digest(timed(kernels, a.reps))}
        split = passes(kernels, max(2, a.reps // 2))
        d["column_pass"], d["row_pass"], d["rd_fill_nearest"] = split["edt_columns"], split["edt_rows"], split["fill_nearest"]
        d["rd_fill_nearest"]["algorithmic_GB_per_s"] = round(16.0 * n * n / d["rd_fill_nearest"]["median_ms"] / 1e6, 1)
        d["front_end"] = digest(timed(lambda: M.fill_voids(dsm), a.reps))
        filled = M.fill_voids(dsm)
        d["voids_left"] = int((filled == -9999.0).sum())
        doc["inputs"]["fill_voids"] = d
        print("fill_voids", json.dumps(d), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc), flush=True)


if __name__ == "__main__":
    main()
