#!/usr/bin/env python3
"""Golden fixture for the evaluation of all pair planes of a sweep (resdepth_amd.evaluation.evaluate_pairs_statistics /
evaluate_pairs_performance): produced by the REFERENCE's own `evaluate_performance` and `get_statistics`
(lib/evaluation.py), build container only.  RESDEPTH_REF names a checkout of the original ResDepth.  Import stand-ins and
in-memory datasets as in make_golden_eval.py.

One raster, P = 3 predictions with different nodata pixels, two area stripes (disjoint: test.py pools per stripe, so a pixel
in two stripes would enter the reference's pool twice), all four masks, a threshold.  Recorded:
  p{k}/calls, p{k}/report   evaluate_performance on prediction k: every get_statistics call in call order, the report text
  pooled/calls              get_statistics per class on the residuals pooled as test.py:235-313 pools them: per prediction
                            and stripe the compressed class residuals of the stripe's slice, concatenated in that order
                            (np.concatenate: test.py's np.ma.array(list).flatten() is the same values for equal-length
                            parts and fails on ragged ones with a current numpy)
Output: g22_pairs_eval.npz (data only; every mask as two np.packbits-ed planes, value == 1 and value == 255 (nodata):
tests/test_eval_pairs_cpu.py:g22_masks rebuilds the uint8 rasters 0 / 1 / 255 the reference was given)."""
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
KEYS = ["count_total", "diff_max", "diff_min", "MAE", "RMSE", "absolute_median", "median", "NMAD"]
TKEYS = ["count_total", "MAE", "RMSE", "absolute_median", "median", "NMAD"]
CLASSES = ["all", "building", "terrain", "terrain_nowater", "terrain_nowater_noforest"]
NODATA, GSD, THR, P = -9999.0, 0.5, 1.5, 3


def recording_get_statistics(res, thr=None):
    st = _get_statistics(res, thr)
    row = [float(st[k]) for k in KEYS]
    row += [float(st.truncated[k]) for k in TKEYS] if thr else [np.nan] * len(TKEYS)
    CALLS.append(row)
    return st


evaluation.get_statistics = recording_get_statistics


def q(x, step):
    """values on a binary grid: exact in f32 / f64 and compressible"""
    return np.round(x / step) * step


def mask_raster(rng, h, w, p, nodata_frac=0.0, blobs=0):
    """uint8 mask values: 1 = set, 0 = unset, 255 = nodata; optional rectangular blobs of 1 (buildings)"""
    m = (rng.rand(h, w) < p).astype(np.uint8)
    for _ in range(blobs):
        y, x = rng.randint(-2, h), rng.randint(-2, w)
        m[max(y, 0):y + rng.randint(2, 9), max(x, 0):x + rng.randint(2, 9)] = 1
    m[rng.rand(h, w) < nodata_frac] = 255
    return m


rng = np.random.RandomState(22)
h, w = 71, 93
area = {"x_extent": [(0, 92), (7, 80)], "y_extent": [(0, 30), (38, 70)]}
gt = q(rng.randn(h, w) * 5 + 420, 1 / 16).astype(np.float32)
init = (gt + q(rng.standard_t(3, size=(h, w)) * 1.2, 1 / 256)).astype(np.float32)
gt[rng.rand(h, w) < 0.03] = NODATA
init[rng.rand(h, w) < 0.02] = NODATA
pairs = np.empty((P, h, w), np.float64)
for k in range(P):
    pairs[k] = np.where(gt == NODATA, 400.0, gt).astype(np.float64) + q(rng.laplace(size=(h, w)) * (0.5 + 0.2 * k) + 0.05 * k,
                                                                      1 / 1024)
    pairs[k][rng.rand(h, w) < 0.02 + 0.02 * k] = NODATA          # every prediction has nodata pixels of its own
pairs[1][10:14, 20:31] = NODATA                                  # and a block that is valid in the other two
masks = {"g": (mask_raster(rng, h, w, 0.9, 0.02), 255.0), "b": (mask_raster(rng, h, w, 0.03, 0.02, blobs=12), 255.0),
         "w": (mask_raster(rng, h, w, 0.15, 0.01), 255.0), "f": (mask_raster(rng, h, w, 0.2, 0.01), 255.0)}
masks["b"][0][29:40, 40:46] = 1                                  # a building across the gap between the stripes
for k, (v, nd) in masks.items():
    DATASETS[f"mask_{k}.tif"] = FakeDataset(v, nd)
ds_in, ds_gt = FakeDataset(init, NODATA, GSD), FakeDataset(gt, NODATA, GSD)
logger_root = logging.getLogger("g22_root")
out = {"pairs": pairs, "init": init, "gt": gt, "thr": np.float64(THR), "nodata": np.float64(NODATA), "gsd": np.float64(GSD)}
for k, (v, nd) in masks.items():
    assert set(np.unique(v)) <= {0, 1, 255}
    out["mask_" + k + "/set"], out["mask_" + k + "/nodata"] = np.packbits(v == 1), np.packbits(v == 255)
out["area"] = np.array([list(x) + list(y) for x, y in zip(area["x_extent"], area["y_extent"])], np.int64)
pool = {c: [] for c in CLASSES}
for k in range(P):
    text = io.StringIO()
    logger_stats = logging.getLogger(f"g22_stats_{k}")
    logger_stats.setLevel(logging.INFO)
    logger_stats.propagate = False
    logger_stats.addHandler(logging.StreamHandler(text))
    CALLS.clear()
    res = evaluation.evaluate_performance(pairs[k].copy(), ds_in, ds_gt, logger_root, area, "mask_g.tif", "mask_b.tif",
                                          "mask_w.tif", "mask_f.tif", logger_stats, THR)
    assert list(res.keys()) == CLASSES
    out[f"p{k}/calls"] = np.array(CALLS)
    out[f"p{k}/report"] = np.array(text.getvalue())
    for x, y in zip(area["x_extent"], area["y_extent"]):          # test.py:217-258
        for c in CLASSES:
            pool[c].append(res[c][y[0]:y[1] + 1, x[0]:x[1] + 1].compressed())
CALLS.clear()
for c in CLASSES:                                                 # test.py:288-314
    recording_get_statistics(np.ma.array(np.concatenate(pool[c])).flatten(), THR)
out["pooled/calls"] = np.array(CALLS)
out["classes"] = np.array(CLASSES)
fn = os.path.join(HERE, "g22_pairs_eval.npz")
np.savez_compressed(fn, **out)
print("g22_pairs_eval.npz", os.path.getsize(fn), [len(out[f"p{k}/calls"]) for k in range(P)], len(CALLS))
