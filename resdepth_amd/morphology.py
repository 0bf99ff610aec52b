"""Distances to a mask on the GPU (include/resdepth_hip_edt.h): the exact Euclidean distance transform with its feature transform,
and what rests on it -- the signed distance to a mask's boundary (the covariate of a distance-binned evaluation), Euclidean
buffers, and nearest-valid filling of DSM voids.

The reference has none of this: it leaves distances, metric buffers and void filling to GDAL and scipy on the host.  No CPU
fallback: the transform and the fill are kernels of libresdepth_hip.so; the square root, the scaling by the GSD and the
comparisons against a threshold are elementwise torch operations on the device rasters that come back.

Pixels are square here: `gsd` is one positive finite number, or a (gsd_y, gsd_x) pair of EQUAL entries.  Anisotropic pixels are
out of scope and raise ValueError.

The distance-binned report of a refined DSM is a composition, with nothing added to evaluation.py:
    d = edge_distance(mask_building, gsd)
    print_binned(evaluate_binned(pred, initial, gt, d, edges=[-inf, -2, 0, 2, 5, inf]), logger, unit="m")
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ._lib import EDT_MAX_COLS, EDT_MAX_ROWS, EDT_NONE, check, load, ptr, stream_ptr, workspace
from .evaluation import _first_device, _float_raster, _on, _pair_of

NO_CAP = EDT_NONE - 1                                 # max_d2 of rd_fill_nearest that caps nothing


# ---- arguments, checked on the host before a device is needed ---------------------------------------------------------------------
def _shape2(x, who, what):
    shape = tuple(np.shape(x))
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"{who}: {what} must be a non-empty 2-D raster, got shape {shape}")
    if shape[0] > EDT_MAX_ROWS or shape[1] > EDT_MAX_COLS:
        raise ValueError(f"{who}: {what} of shape {shape} exceeds {EDT_MAX_ROWS} rows x {EDT_MAX_COLS} columns "
                         "(RD_EDT_MAX_ROWS, RD_EDT_MAX_COLS): cut the raster into overlapping pieces")
    return shape


def _gsd(gsd, who):
    try:
        gsd_y, gsd_x = _pair_of(gsd, f"{who}: gsd", float)
    except TypeError:
        raise ValueError(f"{who}: gsd {gsd!r} must be a scalar or (gsd_y, gsd_x)") from None
    if not (0.0 < gsd_x < math.inf and 0.0 < gsd_y < math.inf):
        raise ValueError(f"{who}: gsd {gsd!r} must be positive and finite")
    if gsd_x != gsd_y:
        raise ValueError(f"{who}: gsd {gsd!r}: anisotropic pixels are out of scope, gsd_y must equal gsd_x")
    return gsd_x


def squared_threshold(distance, gsd):
    """A distance in metres -> the largest d2 in pixels^2 within it: t = floor((distance / gsd)^2 + 1e-9), at most RD_EDT_NONE - 1
    (which caps nothing).  The 1e-9 keeps a radius that is a whole number of pixels on the near side of the rounding of the
    division.  distance >= 0, gsd > 0."""
    q = (float(distance) / float(gsd)) ** 2 + 1e-9
    return NO_CAP if q >= NO_CAP else int(math.floor(q))


def _mask_bytes(mask, dev):
    """the mask as device bytes: non-zero = set.  A uint8 raster is taken as it is (any non-zero byte counts as set)."""
    m = _on(mask, dev)
    return m if m.dtype == torch.uint8 else (m != 0).to(torch.uint8).contiguous()


# ---- the two kernels' entry points ------------------------------------------------------------------------------------------------
def _edt(mask_u8, invert, want_idx):
    """device uint8 raster -> (d2, idx or None) int32 device rasters of rd_edt_sq"""
    rows, cols = mask_u8.shape
    lib = load()
    with torch.cuda.device(mask_u8.device):
        nb = lib.rd_edt_ws_bytes(rows, cols)
        ws = workspace(nb, mask_u8.device)
        d2 = torch.empty((rows, cols), dtype=torch.int32, device=mask_u8.device)
        idx = torch.empty((rows, cols), dtype=torch.int32, device=mask_u8.device) if want_idx else None
        check(lib.rd_edt_sq(ptr(mask_u8), int(bool(invert)), rows, cols, ptr(d2), ptr(idx), ptr(ws), nb, stream_ptr()), "edt_sq")
    return d2, idx


def _metres(d2, gsd):
    """int32 d2 -> fp64 sqrt(d2) * gsd, inf where nothing is set"""
    d = torch.sqrt(d2.to(torch.float64)) * gsd
    return torch.where(d2 == EDT_NONE, torch.full_like(d, math.inf), d)


# ---- the front end ------------------------------------------------------------------------------------------------------------------
def distance_transform(mask, gsd=1.0, *, invert=False, squared=False, return_indices=False, device="cuda"):
    """The exact Euclidean distance from every pixel to the nearest SET pixel of `mask` (rd_edt_sq).

    mask: a 2-D raster (array / tensor; non-zero = set, or zero = set with invert=True), at most 32768 rows x 16384 columns;
    gsd: metres per pixel, a positive finite scalar -- a (gsd_y, gsd_x) pair must have equal entries, anisotropic pixels are out
    of scope.
    -> device fp64 raster sqrt(d2) * gsd, 0 on a set pixel and inf where the mask has no set pixel at all; with squared=True the
    int32 raster d2 in pixels^2 as the kernel wrote it (RD_EDT_NONE = 2147483647 where nothing is set; gsd is not applied).
    return_indices=True: -> (distances, indices), indices an int64 [rows, cols, 2] tensor (row, col) of the nearest set pixel,
    -1 where there is none.  Ties go to the pixel with the smallest |column offset|, then the smaller column, then the smaller
    row.
    The cost grows with the distances themselves: a mask with features everywhere costs a few passes over the raster, a single
    set pixel in a corner of an 8192 x 8192 raster about 1e4 LDS reads per pixel (DESIGN.md 3.6e has the measured times).
    ValueError for bad arguments before any launch."""
    who = "distance_transform"
    _shape2(mask, who, "mask")
    g = _gsd(gsd, who)
    dev = _first_device(mask, default=device)
    d2, idx = _edt(_mask_bytes(mask, dev), invert, return_indices)
    dist = d2 if squared else _metres(d2, g)
    if not return_indices:
        return dist
    cols = d2.shape[1]
    i64 = idx.to(torch.int64)
    rc = torch.stack((torch.div(i64, cols, rounding_mode="floor"), i64 % cols), dim=-1)
    return dist, torch.where((i64 < 0)[..., None], torch.full_like(rc, -1), rc)


def edge_distance(mask, gsd=1.0, device="cuda"):
    """The signed distance, in metres, from every pixel to the boundary of `mask` -> device fp64 raster: OUTSIDE the mask + the
    distance to the nearest mask pixel, INSIDE the mask - the distance to the nearest pixel that is not in the mask.  Two calls
    of rd_edt_sq on the same bytes, the second with invert=1; no complemented copy of the mask is made.  There are no zeros: the
    smallest magnitude is one pixel (gsd).  An empty mask gives +inf everywhere, a full one -inf.
    The covariate of a distance-binned evaluation: evaluate_binned(pred, initial, gt, edge_distance(mask_building, gsd),
    edges=[-inf, -2, 0, 2, 5, inf]).  gsd as in distance_transform (square pixels only)."""
    who = "edge_distance"
    _shape2(mask, who, "mask")
    g = _gsd(gsd, who)
    dev = _first_device(mask, default=device)
    m = _mask_bytes(mask, dev)
    outside, _ = _edt(m, 0, False)                    # to the nearest mask pixel: 0 inside
    inside, _ = _edt(m, 1, False)                     # to the nearest pixel outside the mask: 0 outside
    return torch.where(outside == 0, -_metres(inside, g), _metres(outside, g))


def buffer_mask(mask, radius, gsd=1.0, device="cuda"):
    """A Euclidean buffer of `mask` -> device bool raster.  With t = floor((|radius| / gsd)^2 + 1e-9) on the host
    (squared_threshold): radius >= 0 is the dilation by a disc, d2 <= t with d2 the squared distance to the nearest mask pixel;
    radius < 0 is the erosion, d2 of the COMPLEMENT > t.  radius 1 and 2 pixels equal evaluation.dilate_mask(mask, 1) and
    (mask, 2); from 3 pixels on the cross dilation is a diamond and this is a disc.  A ring of 2..10 m is
    buffer_mask(m, 10, gsd) & ~buffer_mask(m, 2, gsd).  gsd as in distance_transform (square pixels only)."""
    who = "buffer_mask"
    _shape2(mask, who, "mask")
    g = _gsd(gsd, who)
    radius = float(radius)
    if math.isnan(radius):
        raise ValueError(f"{who}: radius is NaN")
    t = squared_threshold(abs(radius), g)
    dev = _first_device(mask, default=device)
    m = _mask_bytes(mask, dev)
    if radius >= 0:
        return _edt(m, 0, False)[0] <= t
    return _edt(m, 1, False)[0] > t


def fill_voids(dsm, nodata=-9999, *, max_distance=None, gsd=1.0, return_mask=False, device="cuda"):
    """Nearest-valid filling of the voids of a DSM (rd_edt_sq on the void mask, rd_fill_nearest) -> device raster of the DSM's
    element type (f32 / f64 read as given, anything else as f64).

    A pixel is a VOID when it equals `nodata` or is NaN (nodata=None: NaN only).  A void takes the value of the nearest valid
    pixel -- ties as in distance_transform -- when that pixel lies within max_distance metres (d2 <= floor((max_distance /
    gsd)^2 + 1e-9); None: no cap); other voids keep their value.  Valid pixels are copied bit for bit, so a raster without
    voids comes back bit-identical, and a raster without a valid pixel comes back unchanged.  No interpolation.
    return_mask=True: -> (filled, mask), mask a bool raster of the voids that were filled.
    gsd as in distance_transform (square pixels only)."""
    who = "fill_voids"
    _shape2(dsm, who, "dsm")
    g = _gsd(gsd, who)
    cap = NO_CAP
    if max_distance is not None:
        md = float(max_distance)
        if not md >= 0.0:
            raise ValueError(f"{who}: max_distance {max_distance!r} must be >= 0 (or None for no cap)")
        cap = squared_threshold(md, g)
    dev = _first_device(dsm, default=device)
    z = _float_raster(dsm, dev)
    void = torch.isnan(z) if nodata is None else (torch.isnan(z) | (z == float(nodata)))
    d2, idx = _edt(void.to(torch.uint8), 1, True)     # set = not a void
    out = torch.empty_like(z)
    with torch.cuda.device(dev):
        check(load().rd_fill_nearest(ptr(z), int(z.dtype == torch.float64), ptr(d2), ptr(idx), z.numel(), cap, ptr(out),
                                     stream_ptr()), "fill_nearest")
    if return_mask:
        return out, void & (d2 <= cap)
    return out
