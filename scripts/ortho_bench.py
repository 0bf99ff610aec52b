#!/usr/bin/env python3
"""Time rd_ortho_rpc (include/resdepth_hip_ortho.h) on one GPU and write / extend profiles/ortho.json.

    python scripts/ortho_bench.py [--size 8192] [--image 16384] [--label shipped] [--rows all|footprint] [--out profiles/ortho.json]

The C entry point is timed with device events around the call on pre-allocated outputs: one warm-up, then the median of 7 with
the minimum and maximum.  Rows: geographic / UTM, the three resamplings, P = 1, 2, 4, an image aligned with the grid and one turned
by 30 degrees; beside each time the bytes model (4 + 4P (+ P for valid) per pixel plus each image region once) and the fp64 model
(about 250 flops for the map projection and about 130 per view, per pixel) -- models for orientation, not measurements.  The
measured coordinate deviation from the numpy oracle (tests/ortho_ref.py) and the oracle's time on a 1024^2 crop go in as well.

How a wave's 64 pixels lie on the grid (ORTHO_FW in csrc/rd_tiles.hip: 64 x 1, 16 x 4 or 8 x 8) is a compile-time constant of the
library: the footprint rows were taken by building the library once per value and running `--rows footprint --label 16x4` on each
(RESDEPTH_HIP_LIB names the library to load); every run merges its rows into the file under its label.
"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ortho_ref as R  # noqa: E402
from resdepth_amd import _lib, ortho  # noqa: E402

DEV = "cuda:0"
UTM_GT, GEO_GT = (465000.0, 0.25, 0.0, 5247000.0, 0.0, -0.25), (8.0, 3.3e-6, 0.0, 47.4, 0.0, -2.25e-6)
ZOOM = 0.7                                              # the grid covers 0.7 of the image's half-size: about 1.4 image px per DSM px


def models_for(size, image, crs, angle, n):
    gt, name = (UTM_GT, "utm") if crs == "utm" else (GEO_GT, "geographic")
    w, h = gt[1] * size, gt[5] * size                   # a 2 x 2 grid whose pixel centres are the corners of the DSM
    lon, lat = R.ground(2, 2, (gt[0] - 0.5 * w, w, gt[3] - 0.5 * h, h), name, 9.0, 0.0)
    return [R.synthetic_rpc((float(lon.min()), float(lon.max())), (float(lat.min()), float(lat.max())), (300.0, 500.0), image, image,
                            angle_deg=angle, zoom=ZOOM, shift=(7.0 * v, -5.0 * v), seed=v) for v in range(n)]


def pack(models, images):
    desc = np.zeros(len(models), dtype=ortho._VIEW_DESC)
    for d, m, im in zip(desc, models, images):
        d["image"], d["pitch"], d["rows"], d["cols"], d["dtype"] = im.data_ptr(), im.stride(0), im.shape[0], im.shape[1], 1
        d["image_nodata"] = float("nan")
        for name in R.SCALARS + R.VECTORS:
            d[name] = m[name]
    return torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to(DEV)


def timed(fn, reps=7):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--image", type=int, default=16384)
    ap.add_argument("--label", default="shipped")
    ap.add_argument("--rows", choices=("all", "footprint"), default="all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ortho.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ortho_bench: no GPU: nothing is measured without one")
    lib = _lib.load()
    size, image = a.size, a.image
    n = size * size
    g = torch.Generator(device=DEV).manual_seed(1)
    dsm = 400.0 + 20.0 * torch.rand((size, size), generator=g, device=DEV)
    images = [torch.randint(1, 30000, (image, image), generator=g, device=DEV, dtype=torch.int16) for _ in range(2)]
    out = torch.empty((4, size, size), dtype=torch.float32, device=DEV)
    valid = torch.empty((4, size, size), dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    rows = []

    def run(crs, kind, p, angle, with_valid=True):
        gt = UTM_GT if crs == "utm" else GEO_GT
        views = pack(models_for(size, image, crs, angle, p), [images[v % 2] for v in range(p)])

        def call():
            rc = lib.rd_ortho_rpc(dsm.data_ptr(), size, size, gt[0], gt[1], gt[3], gt[5], _lib.ORTHO_CRS[crs], 9.0, 0.0, -9999.0, 0.0,
                                  views.data_ptr(), p, _lib.ORTHO_RESAMPLING[kind], 0.0, out.data_ptr(),
                                  valid.data_ptr() if with_valid else None, None, stream)
            assert rc == 0, lib.rd_last_error_string()
        t = timed(call)
        share = float(valid[:p].float().mean())
        region = (ZOOM * image) ** 2                    # elements of an image under the grid
        model_bytes = n * (4 + 4 * p + (p if with_valid else 0)) + min(p, 2) * region * 2
        model_flop = n * ((250 if crs == "utm" else 0) + 130 * p)
        row = dict(label=a.label, crs=crs, resampling=kind, views=p, angle_deg=angle, valid_share=round(share, 4), **t,
                   model_bytes=model_bytes, model_fp64_flop=model_flop,
                   model_GBps=round(model_bytes / t["ms_median"] / 1e6, 1), model_fp64_GFLOPs=round(model_flop / t["ms_median"] / 1e6, 1))
        rows.append(row)
        print(json.dumps(row), flush=True)

    if a.rows == "footprint":
        for angle in (0.0, 30.0):
            for kind in ("bilinear", "bicubic"):
                run("utm", kind, 2, angle)
    else:
        for crs in ("geographic", "utm"):
            for kind in ("nearest", "bilinear", "bicubic"):
                for angle in (0.0, 30.0):
                    run(crs, kind, 2, angle)
        for p in (1, 4):
            for angle in (0.0, 30.0):
                run("utm", "bilinear", p, angle)

    extra = {}
    if a.rows == "all":
        # the coordinate deviation from the oracle, and the oracle's time, on a 1024^2 crop of the same scene
        crop = 1024
        z = dsm[:crop, :crop].contiguous()
        for crs in ("geographic", "utm"):
            gt = UTM_GT if crs == "utm" else GEO_GT
            models = models_for(size, image, crs, 30.0, 2)
            got = ortho.project_grid([im.view(torch.uint16) for im in images], [ortho.RPC(**m) for m in models], z, gt,
                                     "geographic" if crs == "geographic" else ("utm", 32, "N")).cpu().numpy()
            t0 = time.perf_counter()
            want, _ = R.coords(z.cpu().numpy(), -9999.0, (gt[0], gt[1], gt[3], gt[5]), crs, 9.0, 0.0, 0.0, models, [(0.0, 0.0)] * 2)
            t1 = time.perf_counter()
            extra["coords_max_abs_dev_px_" + crs] = float(np.nanmax(np.abs(got - want)))
            extra["oracle_coords_seconds_1024sq_2views_" + crs] = round(t1 - t0, 3)
        t0 = time.perf_counter()
        R.resample(images[0][:4096, :4096].cpu().numpy().view(np.uint16), None, want[0, ..., 0] % 4000, want[0, ..., 1] % 4000, "bilinear")
        extra["oracle_bilinear_seconds_1024sq_1view"] = round(time.perf_counter() - t0, 3)
        print(json.dumps(extra), flush=True)

    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc.setdefault("what", "rd_ortho_rpc on one MI355X: device events around the C call, median of 7 after a warm-up; the model "
                           "columns are the bytes and fp64 operations the header's cost model counts, not measurements")
    doc["device"] = torch.cuda.get_device_name(0)
    doc["dsm"], doc["image"] = [size, size], [image, image, "uint16"]
    doc["rows"] = [r for r in doc.get("rows", []) if (r["label"], r["footprint_run"]) != (a.label, a.rows == "footprint")]
    for r in rows:
        r["footprint_run"] = a.rows == "footprint"
    doc["rows"] += rows
    doc.update(extra)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
