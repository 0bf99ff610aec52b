"""numpy stand-in for the reference's validation / inference samples (TEST INFRASTRUCTURE ONLY): DsmOrthoDataset.__getitem__
for sampling_strategy 'val' / 'test' (lib/DsmOrthoDataset.py:161-291) with the loss mask cut to the non-overlap box
(:434-470).  Pinned by tests/golden/g19_grid.npz (produced by the reference's own __getitem__); the GPU tests use it on
rasters too large for a fixture."""
import numpy as np
import torch
from torch.utils.data import Dataset

META = ("patch_offset_y", "patch_offset_x", "patch_valid_pixels_uly", "patch_valid_pixels_ulx", "patch_valid_pixels_lry",
        "patch_valid_pixels_lrx")


def grid_sample(dsm_in, dsm_gt, orthos_hwv, pos, box, pair, tile, nodata, dsm_std, ortho_mean, ortho_std, channels,
                dsm_mean=None, transform_dsm=True, transform_orthos=True, mean_override=None):
    """-> {"input", "target", "loss_mask", "dsm_mean"} (target / loss_mask None without a ground truth).  `mean_override`: use
    this per-tile DSM mean instead of computing one (a given mean makes the arithmetic elementwise)."""
    y, x = pos
    t = tile
    nodata = np.float32(nodata)
    patch = dsm_in[y:y + t, x:x + t]
    if transform_dsm:
        if mean_override is not None:
            raw = mean_override
        elif not dsm_mean:                                                            # :193-195 (`if not self.dsm_mean`)
            raw = np.ma.mean(np.ma.masked_where(patch == nodata, patch))              # a float64 value; Normalize rounds it
        else:
            raw = dsm_mean
        mean, std = np.float32(raw), np.float32(dsm_std)
        norm = lambda a: ((a - mean) / std).astype(np.float32)                        # noqa: E731
    else:
        raw = 0.0
        norm = lambda a: a.astype(np.float32)                                         # noqa: E731
    chans = []
    if channels != "stereo":
        chans.append(norm(patch)[None])
    if channels != "geom":
        o = orthos_hwv[y:y + t, x:x + t, list(pair)].transpose((2, 0, 1)).astype(np.float32)
        if transform_orthos:
            om = np.float32(o.mean() if not ortho_mean else ortho_mean)              # :230-241
            o = ((o - om) / np.float32(ortho_std)).astype(np.float32)
        chans.append(o)
    out = {"input": np.concatenate(chans, 0), "dsm_mean": float(raw), "target": None, "loss_mask": None}
    if dsm_gt is not None:
        g = dsm_gt[y:y + t, x:x + t]
        uly, ulx, lry, lrx = box
        inside = np.zeros((t, t), dtype=bool)
        inside[uly:lry + 1, ulx:lrx + 1] = True
        out["target"] = norm(g)[None]
        out["loss_mask"] = (inside & (g != 0) & (g != nodata))[None]
    return out


class StandInGridDataset(Dataset):
    """Host dataset over the stand-in: the reference's sample dicts (torch tensors) for a sample list, plus what
    predict_linear_blend reads (tile_size, stride, raster_shape, pos)."""

    def __init__(self, dsm_in, dsm_gt, orthos_hwv, pos, reg, pairs, tile, stride, nodata, dsm_std, ortho_mean, ortho_std,
                 channels, dsm_mean=None, mean_override=None):
        self.a = (dsm_in, dsm_gt, orthos_hwv)
        self.pos, self.reg, self.pairs = list(pos), list(reg), list(pairs)
        self.tile_size, self.stride, self.raster_shape = int(tile), int(stride), tuple(dsm_in.shape)
        self.kw = dict(tile=tile, nodata=nodata, dsm_std=dsm_std, ortho_mean=ortho_mean, ortho_std=ortho_std, channels=channels,
                       dsm_mean=dsm_mean)
        self.mean_override = mean_override

    def __len__(self):
        return len(self.pos)

    def __getitem__(self, i):
        mo = None if self.mean_override is None else self.mean_override[i]
        s = grid_sample(*self.a, self.pos[i], self.reg[i], self.pairs[i], mean_override=mo, **self.kw)
        d = {"input": torch.from_numpy(s["input"]), "dsm_mean": torch.tensor(s["dsm_mean"], dtype=torch.float64),
             "dsm_std": torch.tensor(float(self.kw["dsm_std"]), dtype=torch.float32),
             "nodata": torch.tensor(float(self.kw["nodata"]), dtype=torch.float32)}
        for k, v in zip(META, tuple(self.pos[i]) + tuple(self.reg[i])):
            d[k] = torch.tensor(int(v))
        if s["target"] is not None:
            d["target"], d["loss_mask"] = torch.from_numpy(s["target"]), torch.from_numpy(s["loss_mask"])
        return d
