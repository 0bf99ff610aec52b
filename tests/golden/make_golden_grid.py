#!/usr/bin/env python3
"""Golden fixtures for the validation / inference grid tiles (GpuGridTiles): samples produced by the REFERENCE's own
`DsmOrthoDataset._determine_patches` (lib/DsmOrthoDataset.py:373-431, which calls rasterutils.create_regular_grid) and
`__getitem__` (:161-291) for sampling_strategy 'val' and 'test' (build container only).

As in make_golden_samples.py the dataset is created with object.__new__ (its constructor reads GeoTIFFs through GDAL), the
attributes its constructor would set are filled with in-memory rasters, and stand-in modules replace GDAL, easydict,
torchsummary, tensorboard and torchvision (functional: ToTensor -> tensor[1,H,W], Normalize -> (t - mean) / std in float32,
Compose).  The rasters hold quarter-metre heights and integer radiances, so the npz compresses.
Output: g19_grid.npz (rasters, the orthos as uint8 [H, W, V]; per case its settings as JSON, positions, boxes, pair indices and every sample dict; data only)."""
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

from lib.DsmOrthoDataset import DsmOrthoDataset  # noqa: E402  (reference)

T, H, W, V = 16, 80, 112, 3
NODATA = np.float32(-9999.0)
rng = np.random.RandomState(19)
dsm_in = (430 + rng.randint(-40, 41, (H, W)) / 4).astype(np.float32)
dsm_gt = (dsm_in + rng.randint(-6, 7, (H, W)) / 4).astype(np.float32)
dsm_in[5:8, 10:14] = NODATA
dsm_in[60:62, 90:97] = NODATA
dsm_gt[20:23, 30:33] = NODATA
dsm_gt[70:72, 80:84] = NODATA
dsm_gt[3, 4] = dsm_gt[41, 50] = dsm_gt[66, 100] = 0.0     # the reference's mask also drops exact zeros
orthos = rng.randint(20, 84, (H, W, V)).astype(np.float32)

TWO_AREAS = {"x_extent": [(0, 31), (70, 105)], "y_extent": [(0, 15), (40, 71)]}
TEST_AREA = {"x_extent": [(20, 59)], "y_extent": [(10, 41)]}
TEST_AREAS = {"x_extent": [(4, 35), (60, 99)], "y_extent": [(50, 73), (6, 29)]}
# name -> settings; ortho_mean None = per tile; dsm_mean None / 0.0 = per tile
CASES = {
    "val_stereo": dict(strategy="val", channels="geom-stereo", pairs=[[0, 1], [1, 2], [0, 2]], area=TWO_AREAS, gt=True,
                       dsm_mean=None, ortho_mean=51.5),
    "test_stereo": dict(strategy="test", channels="geom-stereo", pairs=[[2, 1]], area=TEST_AREA, gt=True,
                        dsm_mean=None, ortho_mean=None),
    "test_geom_nogt": dict(strategy="test", channels="geom", pairs=None, area=TEST_AREAS, gt=False, dsm_mean=None,
                           ortho_mean=None),
    "test_views_only": dict(strategy="test", channels="stereo", pairs=[[2, 0]], area=TEST_AREA, gt=True, dsm_mean=None,
                            ortho_mean=None),
    "test_fixed_mean": dict(strategy="test", channels="geom-stereo", pairs=[[0, 2]], area=TEST_AREA, gt=True,
                            dsm_mean=431.25, ortho_mean=51.5),
    "test_zero_mean": dict(strategy="test", channels="geom", pairs=None, area=TEST_AREA, gt=True, dsm_mean=0.0,
                           ortho_mean=None),
    "val_mono_raw": dict(strategy="val", channels="geom-mono", pairs=[[1], [2]], area=TEST_AREA, gt=True, dsm_mean=None,
                         ortho_mean=None, transform_dsm=False, transform_orthos=False),
}

out = {"dsm_in": dsm_in, "dsm_gt": dsm_gt, "orthos_u8": orthos.astype(np.uint8),       # exact: integer radiances
       "nodata": NODATA, "tile": np.array(T),
       "dsm_std": np.float32(3.25), "ortho_std": np.float32(41.0), "cases": np.array(list(CASES))}
for name, c in CASES.items():
    ds = object.__new__(DsmOrthoDataset)
    ds.tile_size, ds.sampling_strategy, ds.augment = T, c["strategy"], False
    ds.stride = int(T * 0.5) if c["strategy"] == "test" else T                # the constructor's default (:99-104)
    ds.input_channels = c["channels"]
    ds.transform_dsm, ds.transform_orthos = c.get("transform_dsm", True), c.get("transform_orthos", True)
    ds.dsm_mean, ds.dsm_std = c["dsm_mean"], np.asarray(3.25).astype(np.float32)
    ds.ortho_mean = None if c["ortho_mean"] is None else np.asarray(c["ortho_mean"]).astype(np.float32)
    ds.ortho_std = np.asarray(41.0).astype(np.float32)
    ds.permute_images_within_pair = False
    ds.raster_gt = "in-memory" if c["gt"] else None
    ds.dsm_input, ds.orthos, ds.nodata = dsm_in, orthos, np.array(NODATA)
    if c["gt"]:
        ds.dsm_target = dsm_gt
    if c["pairs"] is not None:
        ds.image_pairs = c["pairs"]
    ds.area_defn = c["area"]
    ds._determine_patches()
    n = len(ds)
    out[f"{name}/settings"] = np.array(json.dumps(c))
    out[f"{name}/stride"] = np.array(ds.stride)
    out[f"{name}/pos"] = np.array(ds.patch_position, dtype=np.int64).reshape(n, 2)
    out[f"{name}/reg"] = np.array(ds.patch_valid_pixels, dtype=np.int64).reshape(n, 4)
    out[f"{name}/pair_idx"] = np.asarray(ds.image_pair_indices, dtype=np.int64)
    smp = [ds[i] for i in range(n)]
    out[f"{name}/input"] = np.stack([s["input"].numpy() for s in smp])
    out[f"{name}/dsm_mean"] = np.array([float(s["dsm_mean"]) for s in smp], dtype=np.float64)
    if c["gt"]:
        out[f"{name}/target"] = np.stack([s["target"].numpy() for s in smp])
        out[f"{name}/loss_mask"] = np.stack([s["loss_mask"].numpy() for s in smp])
    meta = ["patch_offset_y", "patch_offset_x", "patch_valid_pixels_uly", "patch_valid_pixels_ulx", "patch_valid_pixels_lry",
            "patch_valid_pixels_lrx"]
    out[f"{name}/meta"] = np.array([[int(s[k]) for k in meta] for s in smp], dtype=np.int64).reshape(n, 6)
    out[f"{name}/scalars"] = np.array([[float(s["nodata"]), float(s["dsm_std"])] for s in smp], dtype=np.float64)
    print(name, n, "samples, input", out[f"{name}/input"].shape)
path = os.path.join(HERE, "g19_grid.npz")
np.savez_compressed(path, **out)
print("g19_grid.npz", os.path.getsize(path), "bytes")
