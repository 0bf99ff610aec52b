#!/usr/bin/env python3
"""Golden fixtures for the class-partitioned evaluation (resdepth_amd.evaluation.evaluate_performance): produced by the
REFERENCE's own `evaluate_performance` (lib/evaluation.py:163-457), build container only.  RESDEPTH_REF names a
checkout of the original ResDepth.  Import stand-ins as in make_golden_stats.py; the rasters are in-memory datasets
(subclasses of a stub gdal.Dataset), the mask paths are names that fdutil.file_exists / rasterutils.load_raster map to
such datasets.  Every get_statistics call is recorded in call order at full precision, the report on logger_stats is
captured as text.  Output: g18_eval.npz (data only; masks np.packbits-ed)."""
import io
import logging
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ["RESDEPTH_REF"])


def stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


class _EasyDict(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)
    __setattr__ = dict.__setitem__


class Dataset:
    pass


stub("easydict", EasyDict=_EasyDict)
stub("osgeo", gdal=stub("osgeo.gdal", GA_ReadOnly=0, Dataset=Dataset))
stub("torchvision", transforms=stub("torchvision.transforms", Compose=type("Compose", (), {}),
                                    ToTensor=type("ToTensor", (), {}), Normalize=type("Normalize", (), {})))
stub("torchsummary", summary=lambda *a, **k: None)
import torch.utils  # noqa: E402
torch.utils.tensorboard = stub("torch.utils.tensorboard", SummaryWriter=type("SummaryWriter", (), {}))
from lib import evaluation  # noqa: E402  (reference)


class Band:
    def __init__(self, values, nodata):
        self.values, self.nodata = values, nodata

    def ReadAsArray(self):
        return self.values.copy()

    def GetNoDataValue(self):
        return self.nodata


class FakeDataset(Dataset):
    def __init__(self, values, nodata, gsd=1.0):
        self.band, self.gsd = Band(values, nodata), gsd

    def GetRasterBand(self, i):
        return self.band

    def ReadAsArray(self):
        return self.band.ReadAsArray()

    def GetGeoTransform(self):
        return (1000.0, self.gsd, 0.0, 2000.0, 0.0, -self.gsd)


DATASETS = {}
evaluation.fdutil.file_exists = lambda p: p in DATASETS
evaluation.rasterutils.load_raster = lambda fn, mode=0: DATASETS[fn]
CALLS = []
_get_statistics = evaluation.get_statistics


def recording_get_statistics(res, thr=None):
    st = _get_statistics(res, thr)
    row = [float(st[k]) for k in KEYS]
    row += [float(st.truncated[k]) for k in TKEYS] if thr else [np.nan] * len(TKEYS)
    CALLS.append(row)
    return st


evaluation.get_statistics = recording_get_statistics
KEYS = ["count_total", "diff_max", "diff_min", "MAE", "RMSE", "absolute_median", "median", "NMAD"]
TKEYS = ["count_total", "MAE", "RMSE", "absolute_median", "median", "NMAD"]
NODATA, GSD = -9999.0, 9.6


def q(x, step):
    """values on a binary grid: exact in f32 / f64 and compressible"""
    return np.round(x / step) * step


def mask_raster(rng, h, w, p, nodata_frac=0.0, blobs=0):
    """uint8 mask values: 1 = set, 0 / 2 = unset, 255 = nodata; optional rectangular blobs of 1 (buildings)"""
    m = np.where(rng.rand(h, w) < p, 1, rng.choice([0, 2], size=(h, w))).astype(np.uint8)
    for _ in range(blobs):
        y, x = rng.randint(-2, h), rng.randint(-2, w)
        m[max(y, 0):y + rng.randint(2, 9), max(x, 0):x + rng.randint(2, 9)] = 1
    m[rng.rand(h, w) < nodata_frac] = 255
    return m


rng = np.random.RandomState(18)
# (shape, masks given, area_defn, threshold)
cases = [
    ((61, 97), "gbwf", {"x_extent": [(0, 96), (10, 50)], "y_extent": [(0, 20), (35, 60)]}, 2.0),
    ((130, 75), "b", None, 1.5),
    ((61, 97), "bf", {"x_extent": [(5, 90)], "y_extent": [(3, 57)]}, None),
    ((130, 75), "", None, None),
    ((61, 97), "gbw", {"x_extent": [(0, 40), (41, 96)], "y_extent": [(0, 29), (30, 60)]}, 3.0),
]
out = {}
for i, ((h, w), which, area, thr) in enumerate(cases):
    gt = q(rng.randn(h, w) * 5 + 420, 1 / 16).astype(np.float32)
    init = (gt + q(rng.standard_t(3, size=(h, w)) * 1.2, 1 / 256)).astype(np.float32)
    pred = gt.astype(np.float64) + q(rng.laplace(size=(h, w)) * 0.6, 1 / 1024)
    gt[rng.rand(h, w) < 0.03] = NODATA
    init[rng.rand(h, w) < 0.02] = NODATA
    pred[rng.rand(h, w) < 0.02] = NODATA
    masks = {}
    if "g" in which:
        masks["g"] = (mask_raster(rng, h, w, 0.9, 0.02), 255.0)
    if "b" in which:
        bm = mask_raster(rng, h, w, 0.03, 0.04 if i == 4 else 0.0, blobs=12)
        if i == 4:                                      # buildings on the border and on both sides of the stripe edges
            bm[0, 5:9] = bm[h - 1, 60:64] = bm[20:23, 0] = bm[40:44, w - 1] = 1
            bm[28:32, 38:44] = 1
            bm[29, 41] = 255
        masks["b"] = (bm, 255.0)
    if "w" in which:
        masks["w"] = (mask_raster(rng, h, w, 0.15, 0.01), 255.0)
    if "f" in which:
        masks["f"] = (mask_raster(rng, h, w, 0.2, 0.01), 255.0)
    DATASETS.clear()
    for k, (v, nd) in masks.items():
        DATASETS[f"mask_{k}.tif"] = FakeDataset(v, nd)
    ds_in, ds_gt = FakeDataset(init, NODATA, GSD), FakeDataset(gt, NODATA, GSD)
    text = io.StringIO()
    logger_stats = logging.getLogger(f"g18_stats_{i}")
    logger_stats.setLevel(logging.INFO)
    logger_stats.propagate = False
    logger_stats.addHandler(logging.StreamHandler(text))
    logger_root = logging.getLogger("g18_root")
    CALLS.clear()
    path = {k: (f"mask_{k}.tif" if k in masks else None) for k in "gbwf"}
    res = evaluation.evaluate_performance(pred.copy(), ds_in, ds_gt, logger_root, area, path["g"], path["b"], path["w"],
                                          path["f"], logger_stats, thr)
    p = f"c{i}/"
    out[p + "pred"], out[p + "init"], out[p + "gt"] = pred, init, gt
    for k, (v, nd) in masks.items():
        out[p + "mask_" + k] = v
    if area is not None:
        out[p + "area"] = np.array([list(x) + list(y) for x, y in zip(area["x_extent"], area["y_extent"])], np.int64)
    out[p + "thr"] = np.float64(-1.0 if thr is None else thr)
    out[p + "calls"] = np.array(CALLS)
    out[p + "report"] = np.array(text.getvalue())
    out[p + "classes"] = np.array(list(res.keys()))
    for c, r in res.items():
        out[p + "rmask_" + c] = np.packbits(np.ma.getmaskarray(r))
    out[p + "rall"] = res["all"].compressed()
out["n"] = np.array(len(cases))
out["nodata"], out["gsd"] = np.float64(NODATA), np.float64(GSD)
fn = os.path.join(HERE, "g18_eval.npz")
np.savez_compressed(fn, **out)
print("g18_eval.npz", os.path.getsize(fn), [len(out[f"c{i}/calls"]) for i in range(len(cases))])
