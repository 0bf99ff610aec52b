"""The two statistics train.py computes before it builds its loaders (train.py:107-138), as reductions over the rasters a
GpuPatchSampler keeps in HBM: the robust DSM scale of `utils.compute_local_dsm_std_per_centered_patch` (lib/utils.py:111-158,
a batch-1 DataLoader over every training patch cast to float128 in the reference) and the ortho-image mean / std of
`utils.compute_satellite_image_normalization` (lib/utils.py:161-200)."""
from __future__ import annotations

import itertools
import math

import numpy as np
import torch

from ._lib import check, load, ptr, stream_ptr


def patch_moments(sampler, positions, raster_identifier: str = "raster_in", use_nodata: bool = True) -> torch.Tensor:
    """(count, mean, M2 = sum (x - mean)^2) in fp64 per tile x tile patch at `positions` [n, 2] (y, x) of the sampler's input
    DSM ('raster_in') or target DSM ('raster_gt'), over the pixels != nodata -> device tensor [n, 3] (rd_patch_moments)."""
    if raster_identifier not in ("raster_in", "raster_gt"):
        raise ValueError(f"raster_identifier must be 'raster_in' or 'raster_gt' (got {raster_identifier!r})")
    plane = sampler.dsm_in if raster_identifier == "raster_in" else sampler.dsm_gt
    if plane is None:
        raise ValueError("the sampler has no ground-truth raster")
    pos = torch.as_tensor(np.asarray(positions), dtype=torch.int32).reshape(-1, 2)
    n, t = pos.shape[0], sampler.tile
    if n == 0:
        return torch.empty(0, 3, dtype=torch.float64, device=sampler.device)
    if int(pos.min()) < 0 or int(pos[:, 0].max()) + t > sampler.h or int(pos[:, 1].max()) + t > sampler.w:
        raise ValueError("patch position outside the raster")
    with torch.cuda.device(sampler.device):
        pos = pos.to(sampler.device).contiguous()
        out = torch.empty(n, 3, dtype=torch.float64, device=sampler.device)
        lib = load()
        ws = torch.empty(lib.rd_patch_moments_ws_bytes(n, t), dtype=torch.uint8, device=sampler.device)
        check(lib.rd_patch_moments(ptr(plane), sampler.h, sampler.w, ptr(pos), n, t, sampler.nodata, 1 if use_nodata else 0,
                                   ptr(out), ptr(ws), ws.numel(), stream_ptr()), "patch_moments")
    return out


def local_dsm_stds(groups, raster_identifier: str = "raster_in") -> np.ndarray:
    """The per-sample unbiased standard deviations (lib/utils.py:149-150), float64, concatenated in group order."""
    stds = []
    for gi, (sampler, positions) in enumerate(groups):
        m = patch_moments(sampler, positions, raster_identifier).cpu().numpy()
        bad = np.nonzero(m[:, 0] < 2)[0]
        if bad.size:
            y, x = np.asarray(positions).reshape(-1, 2)[bad[0]]
            raise ValueError(f"compute_local_dsm_std_per_centered_patch: patch {int(bad[0])} of group {gi} at (y, x) = ({int(y)}, "
                             f"{int(x)}) has {int(m[bad[0], 0])} valid pixels (< 2): its standard deviation is undefined")
        stds.append(np.sqrt(m[:, 2] / (m[:, 0] - 1.0)))
    return np.concatenate(stds) if stds else np.zeros(0)


def trimmed_mean(stds) -> float:
    """Mean of the values between the 5th and the 95th percentile, both included (numpy's default linear interpolation,
    lib/utils.py:152-156)."""
    stds = np.asarray(stds, dtype=np.float64)
    p95, p5 = np.percentile(stds, 95), np.percentile(stds, 5)
    return stds[np.logical_and(stds >= p5, stds <= p95)].mean().item()


def compute_local_dsm_std_per_centered_patch(groups, raster_identifier: str = "raster_in") -> float:
    """utils.compute_local_dsm_std_per_centered_patch over groups = [(GpuPatchSampler, positions [n, 2]), ...] (one group per
    dataset of the reference's ConcatDataset; positions e.g. from tiling.draw_train_samples -- the reference draws a sample
    list of its own for this pass, train.py:111-118)."""
    stds = local_dsm_stds(groups, raster_identifier)
    if stds.size == 0:
        raise ValueError("compute_local_dsm_std_per_centered_patch: no patches")
    return trimmed_mean(stds)


def region_moments(sampler, image_ids, area_defn) -> np.ndarray:
    """(count, mean, M2) in fp64 over the ortho planes `image_ids` x the rectangles of `area_defn` (inclusive extents,
    lib/utils.py:185-191), one rd_region_moments call -> float64 [3] on the host."""
    if sampler.orthos is None:
        raise ValueError("the sampler has no ortho images")
    planes = [int(i) for i in image_ids]
    xe, ye = area_defn["x_extent"], area_defn["y_extent"]
    if len(xe) != len(ye) or not planes or not len(xe):
        raise ValueError("compute_satellite_image_normalization: empty image list or malformed area_defn")
    rects = []
    for (x0, x1), (y0, y1) in zip(xe, ye):
        if x0 < 0 or y0 < 0 or x1 >= sampler.w or y1 >= sampler.h or x1 < x0 or y1 < y0:
            raise ValueError(f"area x {x0}..{x1}, y {y0}..{y1} is not inside the {sampler.h} x {sampler.w} raster")
        rects += [int(y0), int(y1) + 1, int(x0), int(x1) + 1]
    n_stack = sampler.orthos.shape[0]
    if any(p < 0 or p >= n_stack for p in planes):
        raise ValueError(f"an image index is outside the {n_stack} ortho planes")
    import ctypes as C
    lib = load()
    c_planes, c_rects = (C.c_int * len(planes))(*planes), (C.c_int * len(rects))(*rects)
    need = lib.rd_region_moments_ws_bytes(sampler.h, sampler.w, len(planes), c_rects, len(rects) // 4)
    with torch.cuda.device(sampler.device):
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=sampler.device)
        out = torch.empty(3, dtype=torch.float64, device=sampler.device)
        check(lib.rd_region_moments(ptr(sampler.orthos), sampler.h * sampler.w, n_stack, sampler.h, sampler.w, c_planes,
                                    len(planes), c_rects, len(rects) // 4, ptr(out), ptr(ws), ws.numel(), stream_ptr()),
              "region_moments")
    return out.cpu().numpy()


def merge_moments(parts):
    """Chan's pairwise update over [(count, mean, M2), ...] in list order, fp64."""
    n, mean, m2 = 0.0, 0.0, 0.0
    for c, m, q in parts:
        c, m, q = float(c), float(m), float(q)
        if c == 0:
            continue
        tot = n + c
        d = m - mean
        m2 = m2 + q + d * d * n * c / tot
        mean = mean + d * c / tot
        n = tot
    return n, mean, m2


def compute_satellite_image_normalization(groups):
    """utils.compute_satellite_image_normalization over groups = [(GpuPatchSampler, image_pairs, area_defn), ...] -> (mean,
    std): mean and population std of the unique images of each dataset's pairs over its training rectangles, all datasets
    pooled."""
    parts = []
    for sampler, image_pairs, area_defn in groups:
        ids = sorted(set(itertools.chain(*image_pairs)))
        parts.append(region_moments(sampler, ids, area_defn))
    n, mean, m2 = merge_moments(parts)
    if n == 0:
        raise ValueError("compute_satellite_image_normalization: no pixels")
    return mean, math.sqrt(m2 / n)
