#!/usr/bin/env python3
"""Golden fixture for the multi-dataset validation set (GpuValSet): the samples of the REFERENCE's own
ConcatDataset([DsmOrthoDataset(d, sampling_strategy='val') ...]) (lib/utils.py:256-270; `_determine_patches`,
lib/DsmOrthoDataset.py:373-431, and `__getitem__`, :161-291) over two in-memory datasets, and the batch sizes its
DataLoader(batch_size=5, shuffle=False) yields (build container only).

As in make_golden_grid.py the datasets are created with object.__new__ (the constructor reads GeoTIFFs through GDAL), the
attributes the constructor would set are filled with in-memory rasters, and stand-in modules replace GDAL, easydict,
torchsummary, tensorboard and torchvision.  The two datasets differ in everything a raster descriptor holds -- raster shape,
nodata, DSM std, ortho mean (one fixed, one per tile) / std, number of ortho planes and of pairs -- and in the DSM mean (per
tile / given), so a mix-up shows.  Quarter-metre heights and integer radiances, so the npz compresses.
Output: g21_valset.npz (per dataset its rasters, the orthos as uint8 [H, W, V], and its settings as JSON; the concatenated
list's dataset ids, positions, boxes, pair indices and every sample dict; the DataLoader's batch sizes; data only)."""
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

from torch.utils.data import ConcatDataset, DataLoader  # noqa: E402

T = 16
rng = np.random.RandomState(21)


def raster(h, w, v, base, nodata, holes_in, holes_gt, zeros):
    dsm_in = (base + rng.randint(-40, 41, (h, w)) / 4).astype(np.float32)
    dsm_gt = (dsm_in + rng.randint(-6, 7, (h, w)) / 4).astype(np.float32)
    for y0, y1, x0, x1 in holes_in:
        dsm_in[y0:y1, x0:x1] = nodata
    for y0, y1, x0, x1 in holes_gt:
        dsm_gt[y0:y1, x0:x1] = nodata
    for y, x in zeros:
        dsm_gt[y, x] = 0.0                                   # the reference's mask also drops exact zeros
    return dsm_in, dsm_gt, rng.randint(20, 84, (h, w, v)).astype(np.float32)


# ortho_mean None = per tile; dsm_mean None = per tile.  Dataset 0 has 8 grid positions x 3 pairs = 24 samples: not a multiple
# of the batch size 5, so a batch straddles the two datasets
DATASETS = [
    dict(shape=(80, 112), planes=3, base=430, nodata=-9999.0, dsm_std=3.25, ortho_mean=51.5, ortho_std=41.0, dsm_mean=None,
         pairs=[[0, 1], [1, 2], [0, 2]], area={"x_extent": [(0, 31), (70, 105)], "y_extent": [(0, 15), (40, 71)]},
         holes_in=[(5, 8, 10, 14), (60, 62, 90, 97)], holes_gt=[(8, 11, 20, 23), (50, 52, 80, 84)], zeros=[(3, 4), (41, 75), (66, 100)]),
    dict(shape=(64, 96), planes=2, base=388, nodata=-32767.0, dsm_std=2.5, ortho_mean=None, ortho_std=37.0, dsm_mean=389.25,
         pairs=[[1, 0], [0, 1]], area={"x_extent": [(3, 60)], "y_extent": [(2, 41)]},
         holes_in=[(10, 13, 20, 26), (30, 31, 40, 58)], holes_gt=[(4, 9, 5, 9), (25, 28, 33, 36)], zeros=[(2, 3), (20, 44), (40, 59)]),
]
CHANNELS = "geom-stereo"

out = {"tile": np.array(T), "channels": np.array(CHANNELS), "n_datasets": np.array(len(DATASETS))}
parts = []
for di, c in enumerate(DATASETS):
    h, w = c["shape"]
    nodata = np.float32(c["nodata"])
    dsm_in, dsm_gt, orthos = raster(h, w, c["planes"], c["base"], nodata, c["holes_in"], c["holes_gt"], c["zeros"])
    ds = object.__new__(DsmOrthoDataset)
    ds.tile_size, ds.sampling_strategy, ds.augment = T, "val", False
    ds.stride = T                                                             # the constructor's default for 'val' (:99-104)
    ds.input_channels = CHANNELS
    ds.transform_dsm, ds.transform_orthos = True, True
    ds.dsm_mean, ds.dsm_std = c["dsm_mean"], np.asarray(c["dsm_std"]).astype(np.float32)
    ds.ortho_mean = None if c["ortho_mean"] is None else np.asarray(c["ortho_mean"]).astype(np.float32)
    ds.ortho_std = np.asarray(c["ortho_std"]).astype(np.float32)
    ds.permute_images_within_pair = False
    ds.raster_gt = "in-memory"
    ds.dsm_input, ds.dsm_target, ds.orthos, ds.nodata = dsm_in, dsm_gt, orthos, np.array(nodata)
    ds.image_pairs = c["pairs"]
    ds.area_defn = c["area"]
    ds._determine_patches()
    parts.append(ds)
    out[f"d{di}/dsm_in"], out[f"d{di}/dsm_gt"], out[f"d{di}/orthos_u8"] = dsm_in, dsm_gt, orthos.astype(np.uint8)   # exact
    out[f"d{di}/settings"] = np.array(json.dumps({k: c[k] for k in ("nodata", "dsm_std", "ortho_mean", "ortho_std", "dsm_mean",
                                                                    "pairs", "area")}))
    print("dataset", di, len(ds), "samples")
cat = ConcatDataset(parts)
n = len(cat)
smp = [cat[i] for i in range(n)]
out["dataset_id"] = np.concatenate([np.full(len(p), di, dtype=np.int64) for di, p in enumerate(parts)])
out["pos"] = np.concatenate([np.array(p.patch_position, dtype=np.int64).reshape(len(p), 2) for p in parts])
out["reg"] = np.concatenate([np.array(p.patch_valid_pixels, dtype=np.int64).reshape(len(p), 4) for p in parts])
out["pair_idx"] = np.concatenate([np.asarray(p.image_pair_indices, dtype=np.int64) for p in parts])
out["input"] = np.stack([s["input"].numpy() for s in smp])
out["target"] = np.stack([s["target"].numpy() for s in smp])
out["loss_mask"] = np.stack([s["loss_mask"].numpy() for s in smp])
out["dsm_mean"] = np.array([float(s["dsm_mean"]) for s in smp], dtype=np.float64)
meta = ["patch_offset_y", "patch_offset_x", "patch_valid_pixels_uly", "patch_valid_pixels_ulx", "patch_valid_pixels_lry",
        "patch_valid_pixels_lrx"]
out["meta"] = np.array([[int(s[k]) for k in meta] for s in smp], dtype=np.int64).reshape(n, 6)
out["scalars"] = np.array([[float(s["nodata"]), float(s["dsm_std"])] for s in smp], dtype=np.float64)
out["batch_sizes"] = np.array([int(b["input"].shape[0]) for b in DataLoader(cat, batch_size=5, shuffle=False)], dtype=np.int64)
print(n, "samples, input", out["input"].shape, "batches", out["batch_sizes"].tolist())
path = os.path.join(HERE, "g21_valset.npz")
np.savez_compressed(path, **out)
print("g21_valset.npz", os.path.getsize(path), "bytes")
