#!/usr/bin/env python3
"""Golden fixtures for the training set and its normalisation statistics (GpuTrainSet, resdepth_amd.normalization): produced by
the REFERENCE's own `DsmOrthoDataset._determine_patches` / `__getitem__` for sampling_strategy 'train'
(lib/DsmOrthoDataset.py:161-371), `utils.compute_local_dsm_std_per_centered_patch` over
DataLoader(ConcatDataset, batch_size=1) (lib/utils.py:111-158) and `utils.compute_satellite_image_normalization`
(lib/utils.py:161-200), build container only.

As in make_golden_grid.py the datasets are created with object.__new__ and filled with in-memory rasters, and stand-in modules
replace GDAL, easydict, torchsummary, tensorboard and torchvision; `lib.rasterutils.load_raster` is replaced by an in-memory
band object so that compute_satellite_image_normalization runs unmodified.  Two rasters, T = 16: "flat" (heights near 2400 m,
relief under 1 m, nodata holes, exact zeros in the target) and "city" (as g19's), three ortho planes of integer radiances each.
Output: g20_train.npz (data only)."""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get("RESDEPTH_REFERENCE", os.path.join(HERE, "..", "..", "..", "ResDepth")))   # a reference checkout


def stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


class _EasyDict(dict):
    __getattr__ = dict.get
    __setattr__ = dict.__setitem__


class _Compose:
    def __init__(self, ts):
        self.transforms = ts

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x


class _ToTensor:
    def __call__(self, a):
        a = np.asarray(a)
        t = torch.from_numpy(np.ascontiguousarray(a))
        return t.unsqueeze(0) if t.dim() == 2 else t.permute(2, 0, 1).contiguous()


class _Normalize:
    def __init__(self, mean, std):
        self.mean, self.std = mean, std

    def __call__(self, t):
        mean = torch.as_tensor(self.mean, dtype=t.dtype).view(-1, 1, 1)
        std = torch.as_tensor(self.std, dtype=t.dtype).view(-1, 1, 1)
        return t.clone().sub_(mean).div_(std)


stub("easydict", EasyDict=_EasyDict)
stub("osgeo", gdal=stub("osgeo.gdal", GA_ReadOnly=0))
stub("torchvision", transforms=stub("torchvision.transforms", Compose=_Compose, ToTensor=_ToTensor, Normalize=_Normalize))
stub("torchsummary", summary=lambda *a, **k: None)
import torch.utils  # noqa: E402
torch.utils.tensorboard = stub("torch.utils.tensorboard", SummaryWriter=type("SummaryWriter", (), {}))

from lib import rasterutils, utils  # noqa: E402  (reference)
from lib.DsmOrthoDataset import DsmOrthoDataset  # noqa: E402  (reference)

T, V = 16, 3
NODATA = np.float32(-9999.0)
rng = np.random.RandomState(20)


def make_raster(h, w, base, relief_steps, step, gt_steps):
    dsm_in = (base + rng.randint(0, relief_steps, (h, w)) * step).astype(np.float32)
    dsm_gt = (dsm_in + rng.randint(-gt_steps, gt_steps + 1, (h, w)) * step).astype(np.float32)
    return dsm_in, dsm_gt


# "flat": relief 255 / 256 m at 2400 m; "city": quarter-metre heights around 430 m (as g19)
flat_in, flat_gt = make_raster(48, 64, 2400.0, 256, 1 / 256, 16)
flat_in[5:8, 10:14] = NODATA
flat_in[30:33, 40:47] = NODATA
flat_gt[20:23, 30:33] = NODATA
flat_gt[3, 4] = flat_gt[41, 50] = flat_gt[17, 60] = 0.0
flat_orthos = rng.randint(20, 84, (48, 64, V)).astype(np.float32)
city_in, city_gt = make_raster(80, 112, 420.0, 81, 0.25, 6)
city_in[60:62, 90:97] = NODATA
city_in[12:15, 20:22] = NODATA
city_gt[70:72, 80:84] = NODATA
city_gt[41, 50] = city_gt[66, 100] = 0.0
city_orthos = rng.randint(20, 84, (80, 112, V)).astype(np.float32)
# flat: dsm_std 32 -- the reference's np.ma.mean accumulates in float32, so its patch mean carries up to a few ulp(2400) = 2.4e-4 m
# of its own rounding; divided by 32 that stays under the 3e-5 bar the samples are compared at (city: ulp(430) / 3.25 = 1e-5)
RASTERS = {"flat": dict(dsm_in=flat_in, dsm_gt=flat_gt, orthos=flat_orthos, dsm_std=32.0, ortho_std=41.0),
           "city": dict(dsm_in=city_in, dsm_gt=city_gt, orthos=city_orthos, dsm_std=3.25, ortho_std=41.0)}

FLAT_AREA = {"x_extent": [(0, 63)], "y_extent": [(0, 47)]}
FLAT_AREAS = {"x_extent": [(0, 30), (34, 63)], "y_extent": [(0, 47), (10, 40)]}
CITY_AREA = {"x_extent": [(20, 99)], "y_extent": [(10, 71)]}
CITY_AREAS = {"x_extent": [(0, 31), (70, 105)], "y_extent": [(0, 15), (40, 71)]}
P3 = [[0, 1], [1, 2], [0, 2]]
# name -> dict(seed, channels, use_all, datasets=[dict(raster, area, n_samples, pairs)], dsm_mean, ortho_mean, transforms)
CASES = {
    "stereo_all": dict(seed=1, channels="geom-stereo", use_all=True, dsm_mean=None, ortho_mean=51.5,
                       datasets=[dict(raster="city", area=CITY_AREAS, n_samples=3, pairs=P3)]),
    "stereo_rand": dict(seed=2, channels="geom-stereo", use_all=False, dsm_mean=None, ortho_mean=None,
                        datasets=[dict(raster="city", area=CITY_AREA, n_samples=6, pairs=P3)]),
    "mono": dict(seed=3, channels="geom-mono", use_all=True, dsm_mean=None, ortho_mean=None,
                 datasets=[dict(raster="flat", area=FLAT_AREA, n_samples=4, pairs=[[1], [2]])]),
    "geom": dict(seed=4, channels="geom", use_all=False, dsm_mean=None, ortho_mean=None,
                 datasets=[dict(raster="flat", area=FLAT_AREAS, n_samples=6, pairs=None)]),
    "views_only": dict(seed=5, channels="stereo", use_all=False, dsm_mean=None, ortho_mean=None,
                       datasets=[dict(raster="city", area=CITY_AREA, n_samples=4, pairs=[[2, 0], [1, 0]])]),
    "fixed_mean": dict(seed=6, channels="geom-stereo", use_all=False, dsm_mean=431.25, ortho_mean=51.5,
                       datasets=[dict(raster="city", area=CITY_AREA, n_samples=4, pairs=[[0, 2]])]),
    "raw": dict(seed=7, channels="geom-mono", use_all=False, dsm_mean=None, ortho_mean=None, transform_dsm=False,
                transform_orthos=False, datasets=[dict(raster="flat", area=FLAT_AREA, n_samples=3, pairs=[[2]])]),
    "concat": dict(seed=8, channels="geom-stereo", use_all=False, dsm_mean=None, ortho_mean=51.5,
                   datasets=[dict(raster="flat", area=FLAT_AREAS, n_samples=4, pairs=[[0, 1], [1, 2]]),
                             dict(raster="city", area=CITY_AREAS, n_samples=4, pairs=P3)]),
}


def make_dataset(c, d):
    r = RASTERS[d["raster"]]
    ds = object.__new__(DsmOrthoDataset)
    ds.tile_size, ds.sampling_strategy, ds.augment, ds.stride = T, "train", False, None
    ds.input_channels = c["channels"]
    ds.transform_dsm, ds.transform_orthos = c.get("transform_dsm", True), c.get("transform_orthos", True)
    ds.dsm_mean, ds.dsm_std = c["dsm_mean"], np.asarray(r["dsm_std"]).astype(np.float32)
    ds.ortho_mean = None if c["ortho_mean"] is None else np.asarray(c["ortho_mean"]).astype(np.float32)
    ds.ortho_std = np.asarray(r["ortho_std"]).astype(np.float32)
    ds.use_all_stereo_pairs, ds.permute_images_within_pair = c["use_all"], False
    ds.raster_gt = "in-memory"
    ds.dsm_input, ds.dsm_target, ds.orthos, ds.nodata = r["dsm_in"], r["dsm_gt"], r["orthos"], np.array(NODATA)
    if d["pairs"] is not None:
        ds.image_pairs = d["pairs"]
    ds.area_defn, ds.n_samples = d["area"], d["n_samples"]
    ds._determine_patches()                       # draws from np.random, in dataset order
    return ds


out = {"nodata": NODATA, "tile": np.array(T), "cases": np.array(list(CASES)), "rasters": np.array(list(RASTERS))}
for name, r in RASTERS.items():
    out[f"{name}/dsm_in"], out[f"{name}/dsm_gt"] = r["dsm_in"], r["dsm_gt"]
    out[f"{name}/orthos_u8"] = r["orthos"].astype(np.uint8)                 # exact: integer radiances
    out[f"{name}/dsm_std"], out[f"{name}/ortho_std"] = np.float32(r["dsm_std"]), np.float32(r["ortho_std"])
for name, c in CASES.items():
    np.random.seed(c["seed"])
    dsets = [make_dataset(c, d) for d in c["datasets"]]
    smp = [ds[i] for ds in dsets for i in range(len(ds))]
    n = len(smp)
    out[f"{name}/settings"] = np.array(json.dumps(c))
    out[f"{name}/dataset_id"] = np.concatenate([np.full(len(ds), k, dtype=np.int64) for k, ds in enumerate(dsets)])
    out[f"{name}/pos"] = np.concatenate([np.array(ds.patch_position, dtype=np.int64).reshape(-1, 2) for ds in dsets])
    out[f"{name}/pair_idx"] = np.concatenate([np.asarray(ds.image_pair_indices, dtype=np.int64) for ds in dsets])
    out[f"{name}/input"] = np.stack([s["input"].numpy() for s in smp])
    out[f"{name}/dsm_mean"] = np.array([float(s["dsm_mean"]) for s in smp], dtype=np.float64)
    out[f"{name}/target"] = np.stack([s["target"].numpy() for s in smp])
    out[f"{name}/loss_mask"] = np.stack([s["loss_mask"].numpy() for s in smp])
    out[f"{name}/offsets"] = np.array([[int(s["patch_offset_y"]), int(s["patch_offset_x"])] for s in smp], dtype=np.int64)
    out[f"{name}/scalars"] = np.array([[float(s["nodata"]), float(s["dsm_std"])] for s in smp], dtype=np.float64)
    assert all(np.isnan(s[f"patch_valid_pixels_{k}"]) for s in smp for k in ("uly", "ulx", "lry", "lrx"))
    assert out[f"{name}/loss_mask"].dtype == np.bool_
    print(name, n, "samples, input", out[f"{name}/input"].shape)

# ---- compute_local_dsm_std_per_centered_patch: the reference's own function over DataLoader(ConcatDataset, batch_size=1) ----
# n = 21: (n - 1) * 0.05 = 1 is an integer (the percentiles fall ON samples); n = 30: it is not (linear interpolation)
for name, counts, seed in (("std21", (11, 10), 31), ("std30", (15, 15), 32)):
    c = dict(channels="geom", use_all=False, dsm_mean=None, ortho_mean=None, transform_dsm=False, transform_orthos=False)
    np.random.seed(seed)
    dsets = [make_dataset(c, dict(raster=rn, area=area, n_samples=k, pairs=None))
             for rn, area, k in (("flat", FLAT_AREAS, counts[0]), ("city", CITY_AREA, counts[1]))]
    out[f"{name}/dataset_id"] = np.concatenate([np.full(len(ds), k, dtype=np.int64) for k, ds in enumerate(dsets)])
    out[f"{name}/pos"] = np.concatenate([np.array(ds.patch_position, dtype=np.int64).reshape(-1, 2) for ds in dsets])
    for ds in dsets:                       # no patch with fewer than two valid pixels, in either raster
        for y, x in ds.patch_position:
            assert (ds.dsm_input[y:y + T, x:x + T] != NODATA).sum() >= 2 and (ds.dsm_target[y:y + T, x:x + T] != NODATA).sum() >= 2
    loader = torch.utils.data.DataLoader(torch.utils.data.ConcatDataset(dsets), batch_size=1, shuffle=False, num_workers=0)
    for ident in ("raster_in", "raster_gt"):
        seen = []
        real = np.percentile
        np.percentile = lambda a, q, *k, **kw: (seen.append(np.array(a, dtype=np.float64)), real(a, q, *k, **kw))[1]   # the stds it averages
        try:
            value = utils.compute_local_dsm_std_per_centered_patch(loader, raster_identifier=ident)
        finally:
            np.percentile = real
        assert len(seen) == 2 and np.array_equal(seen[0], seen[1]) and np.isfinite(seen[0]).all()
        out[f"{name}/{ident}/std"] = np.float64(value)
        out[f"{name}/{ident}/stds"] = seen[0]
        print(name, ident, value, "from", len(seen[0]), "samples")


# ---- compute_satellite_image_normalization, unmodified, over in-memory bands ------------------------------------------------
class _Band:
    def __init__(self, a):
        self.a = a

    def GetRasterBand(self, k):
        return self

    def ReadAsArray(self):
        return self.a


IMAGES = {f"{rn}:{j}": r["orthos"][..., j] for rn, r in RASTERS.items() for j in range(V)}
rasterutils.load_raster = lambda path: _Band(IMAGES[path])
NORM = [dict(raster="flat", pairs=[[0, 1], [1, 0]], area=FLAT_AREAS), dict(raster="city", pairs=P3, area=CITY_AREAS)]
cfg_data = [_EasyDict(image_pairs=[tuple(p) for p in d["pairs"]], image_list=[f"{d['raster']}:{j}" for j in range(V)],
                      area_defn=_EasyDict(d["area"])) for d in NORM]
mean, std = utils.compute_satellite_image_normalization(cfg_data)
total = sum(float(RASTERS[d["raster"]]["orthos"][y0:y1 + 1, x0:x1 + 1, j].sum()) for d in NORM
            for j in sorted({i for p in d["pairs"] for i in p}) for (x0, x1), (y0, y1) in zip(d["area"]["x_extent"], d["area"]["y_extent"]))
assert total < 2 ** 24                                     # the float32 sum of np.mean is exact
out["norm/settings"] = np.array(json.dumps(NORM))
out["norm/mean"], out["norm/std"] = np.float64(mean), np.float64(std)
print("norm", mean, std, "sum", total)

path = os.path.join(HERE, "g20_train.npz")
np.savez_compressed(path, **out)
print("g20_train.npz", os.path.getsize(path), "bytes (g19_grid.npz:", os.path.getsize(os.path.join(HERE, "g19_grid.npz")), ")")
