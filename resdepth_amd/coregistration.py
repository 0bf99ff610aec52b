"""Co-registration of a DSM to its reference on the GPU (include/resdepth_hip_coreg.h): the least-squares 3-D translation between
two gridded surfaces, linearised and iterated, and the sub-pixel resampler that applies it.

The reference requires co-registered rasters of its user (README lines 65-71, lib/DsmOrthoDataset.py:167) and has no way to check
or to repair them; everything here is new.  No CPU fallback: the sums and the resampling are kernels of libresdepth_hip.so, the
3 x 3 system is solved in fp64 on the host out of the ten sums that come back.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ._lib import check, load, ptr, stream_ptr, workspace
from .evaluation import AttrDict, _first_device, _float_raster, _pair_of

NSUMS = 10                                            # RD_SHIFT_NSUMS
COND_MAX = 1e12                                       # a normal matrix beyond this constrains nothing worth reporting


# ---- arguments, checked on the host before a device is needed ---------------------------------------------------------------------
def _shape2(x, who, what):
    shape = tuple(np.shape(x))
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"{who}: {what} must be a non-empty 2-D raster, got shape {shape}")
    return shape


def _gsd(gsd, who):
    try:
        gsd_y, gsd_x = _pair_of(gsd, f"{who}: gsd", float)
    except TypeError:
        raise ValueError(f"{who}: gsd {gsd!r} must be a scalar or (gsd_y, gsd_x)") from None
    if not (0.0 < gsd_x < math.inf and 0.0 < gsd_y < math.inf):
        raise ValueError(f"{who}: gsd {gsd!r} must be positive and finite")
    return gsd_y, gsd_x


def _options(source, reference, gsd, mask, residual_threshold, max_slope, who):
    """-> (shape, gsd_y, gsd_x, thr, the tangent of max_slope or 0)"""
    shape = _shape2(source, who, "source")
    if _shape2(reference, who, "reference") != shape:
        raise ValueError(f"{who}: source {shape} and reference {tuple(np.shape(reference))} differ in shape")
    if mask is not None and tuple(np.shape(mask)) != shape:
        raise ValueError(f"{who}: mask shape {tuple(np.shape(mask))} != raster shape {shape}")
    gsd_y, gsd_x = _gsd(gsd, who)
    thr = 0.0
    if residual_threshold is not None:
        thr = float(residual_threshold)
        if not 0.0 < thr < math.inf:
            raise ValueError(f"{who}: residual_threshold {residual_threshold!r} must be positive and finite")
    tangent = 0.0
    if max_slope is not None:
        if not 0.0 < float(max_slope) < 90.0:
            raise ValueError(f"{who}: max_slope {max_slope!r} must lie in (0, 90) degrees")
        tangent = math.tan(math.radians(float(max_slope)))
    return shape, gsd_y, gsd_x, thr, tangent


def _nodata(nodata):
    return float("nan") if nodata is None else float(nodata)


def _mask_bytes(mask, dev):
    """the pixels allowed to vote as class bytes: bit 0 set where the mask is"""
    if mask is None:
        return None
    m = mask if torch.is_tensor(mask) else torch.from_numpy(np.ascontiguousarray(mask))
    return (m.to(dev) != 0).to(torch.uint8).contiguous()


# ---- the two kernels ----------------------------------------------------------------------------------------------------------------
def _sums(src, ref, cls, nodata, gsd_y, gsd_x, thr, tangent):
    """device rasters -> the ten sums on the host (one synchronisation: the copy of ten doubles)"""
    rows, cols = src.shape
    lib = load()
    with torch.cuda.device(src.device):
        nb = lib.rd_shift_sums_ws_bytes(rows, cols)
        ws = workspace(nb, src.device)
        out = torch.empty(NSUMS, dtype=torch.float64, device=src.device)
        check(lib.rd_shift_sums(ptr(src), int(src.dtype == torch.float64), ptr(ref), int(ref.dtype == torch.float64), ptr(cls),
                                1 if cls is not None else 0, rows, cols, nodata, gsd_x, gsd_y, thr, tangent, ptr(ws), nb,
                                ptr(out), stream_ptr()), "shift_sums")
        return out.cpu().numpy()


def _translate(src, nodata, tx, ty, tz, fill):
    rows, cols = src.shape
    out = torch.empty((rows, cols), dtype=torch.float64, device=src.device)
    with torch.cuda.device(src.device):
        check(load().rd_translate_bilinear(ptr(src), int(src.dtype == torch.float64), rows, cols, nodata, tx, ty, tz, fill,
                                           ptr(out), stream_ptr()), "translate_bilinear")
    return out


# ---- the solve ------------------------------------------------------------------------------------------------------------------------
def solve_shift(sums, gsd_y, gsd_x):
    """The ten sums of rd_shift_sums -> the shift that puts the source onto the reference: tx, ty, tz in metres (tz in the DSM's
    unit), px = (tx / gsd_x, ty / gsd_y), count, sums, sigma0 (the root of the residual sum of squares over N - 3) and cov (3 x 3,
    of tx, ty, tz).  numpy.linalg.solve of the 3 x 3 normal equations in fp64.  RuntimeError where the members constrain nothing:
    fewer than three, or a normal matrix whose condition number exceeds 1e12 (a plane, a constant surface)."""
    sums = np.asarray(sums, dtype=np.float64)
    n, sp, sq, sd, spp, spq, sqq, spd, sqd, sdd = (float(v) for v in sums)
    if n < 3:
        raise RuntimeError(f"estimate_shift: {int(n)} member pixels, a 3-D shift needs at least three")
    normal = np.array([[spp, spq, sp], [spq, sqq, sq], [sp, sq, n]])
    rhs = np.array([spd, sqd, sd])
    with np.errstate(all="ignore"):
        cond = float(np.linalg.cond(normal)) if np.isfinite(normal).all() else math.inf
    if not cond <= COND_MAX:
        raise RuntimeError(f"estimate_shift: the normal matrix has condition number {cond:.3g} (> {COND_MAX:g}): the surface "
                           "over the member pixels (a plane, a constant) does not constrain a 3-D shift")
    a, b, c = (float(v) for v in np.linalg.solve(normal, rhs))
    sol = np.array([a, b, c])
    rss = max(float(sdd - 2.0 * sol @ rhs + sol @ normal @ sol), 0.0)
    sigma0 = math.sqrt(rss / (n - 3.0)) if n > 3 else float("nan")
    flip = np.diag([-1.0, -1.0, 1.0])                   # tx = -a, ty = -b, tz = c
    cov = sigma0 * sigma0 * (flip @ np.linalg.inv(normal) @ flip)
    return AttrDict(tx=-a, ty=-b, tz=c, px=(-a / gsd_x, -b / gsd_y), count=int(n), sums=sums, sigma0=sigma0, cov=cov)


# ---- the front end ------------------------------------------------------------------------------------------------------------------
def estimate_shift(source, reference, gsd, *, nodata=-9999, mask=None, residual_threshold=None, max_slope=None, device="cuda"):
    """Are these two rasters aligned?  One linearised least-squares estimate of the 3-D translation that puts `source` onto
    `reference` (rd_shift_sums, include/resdepth_hip_coreg.h): with p, q Horn's gradient of the source per metre and d =
    reference - source, d ~ a p + b q + c over the member pixels; tx = -a, ty = -b (metres, columns to the right and rows
    downwards), tz = c.

    source, reference: equal 2-D rasters (arrays / tensors, f32 / f64 read as given); gsd: a scalar or (gsd_y, gsd_x); nodata: of
    both rasters (None: none); mask: the pixels allowed to vote (bool / uint8, non-zero = allowed), the user's stable terrain;
    residual_threshold: pixels with |d| above it do not vote; max_slope: degrees, pixels steeper than it (building edges) do not.
    -> AttrDict tx, ty, tz, px = (tx / gsd_x, ty / gsd_y), count, sums (the ten numbers as they came back), sigma0, cov.
    One estimate is exact for small shifts of smooth surfaces only: coregister() iterates.  Ten doubles cross to the host and the
    call synchronises once.  ValueError for bad arguments before any launch; RuntimeError where the members constrain nothing."""
    who = "estimate_shift"
    _, gsd_y, gsd_x, thr, tangent = _options(source, reference, gsd, mask, residual_threshold, max_slope, who)
    dev = _first_device(source, reference, default=device)
    src, ref = _float_raster(source, dev), _float_raster(reference, dev)
    sums = _sums(src, ref, _mask_bytes(mask, dev), _nodata(nodata), gsd_y, gsd_x, thr, tangent)
    return solve_shift(sums, gsd_y, gsd_x)


def _shift_px(shift_px, dz, who):
    try:
        tx, ty = _pair_of(shift_px, f"{who}: shift_px", float)
        dz = float(dz)
    except TypeError:
        raise ValueError(f"{who}: shift_px {shift_px!r} must be a scalar or (x, y) in pixels") from None
    if not (math.isfinite(tx) and math.isfinite(ty) and math.isfinite(dz)):
        raise ValueError(f"{who}: shift ({tx}, {ty}, {dz}) must be finite")
    return tx, ty, dz


def translate(dsm, shift_px, dz=0.0, *, nodata=-9999, fill=float("nan"), device="cuda"):
    """The resampler on its own (rd_translate_bilinear): the content of `dsm` moved by shift_px = (x, y) pixels -- columns to the
    right, rows downwards -- and lifted by dz, resampled bilinearly -> device fp64 raster.  A shift by whole pixels is an exact
    copy; `fill` where a needed tap is outside the raster, nodata or NaN."""
    _shape2(dsm, "translate", "dsm")
    tx, ty, dz = _shift_px(shift_px, dz, "translate")
    dev = _first_device(dsm, default=device)
    return _translate(_float_raster(dsm, dev), _nodata(nodata), tx, ty, dz, float(fill))


def coregister(source, reference, gsd, *, max_iter=10, tol=1e-3, fill=float("nan"), nodata=-9999, mask=None,
               residual_threshold=None, max_slope=None, device="cuda"):
    """Remove the 3-D offset of `source` against `reference`: estimate_shift iterated.  Every iteration resamples the ORIGINAL
    source by the shift accumulated so far (never a resampled raster again), estimates the increment and adds it; it stops when
    the increment is below `tol` -- in pixels for tx and ty, in the DSM's unit for tz -- or after max_iter iterations.
    -> AttrDict
      shifted    device fp64 raster: the original source resampled ONCE by the total shift, `fill` where undefined; with
                 fill=nodata it goes straight into evaluate_statistics / evaluate_performance, which drop prediction == nodata
      shift      tx, ty, tz, px of the total; count, sums, sigma0, cov of the last estimate
      history    per iteration: tx, ty, tz, px of the increment and its count
      converged  whether the last increment was below tol
    The options are estimate_shift's; the mask lives on the reference's grid."""
    who = "coregister"
    _, gsd_y, gsd_x, thr, tangent = _options(source, reference, gsd, mask, residual_threshold, max_slope, who)
    if int(max_iter) != max_iter or max_iter < 1:
        raise ValueError(f"{who}: max_iter {max_iter!r} must be a positive integer")
    if not 0.0 < float(tol) < math.inf:
        raise ValueError(f"{who}: tol {tol!r} must be positive and finite")
    dev = _first_device(source, reference, default=device)
    src, ref = _float_raster(source, dev), _float_raster(reference, dev)
    cls, nd = _mask_bytes(mask, dev), _nodata(nodata)
    px_x = px_y = tz = 0.0
    history, converged, last = [], False, None
    for _ in range(int(max_iter)):
        cur = _translate(src, nd, px_x, px_y, tz, float("nan"))
        last = solve_shift(_sums(cur, ref, cls, nd, gsd_y, gsd_x, thr, tangent), gsd_y, gsd_x)
        px_x, px_y, tz = px_x + last.px[0], px_y + last.px[1], tz + last.tz
        history.append(AttrDict(tx=last.tx, ty=last.ty, tz=last.tz, px=last.px, count=last.count))
        if abs(last.px[0]) < tol and abs(last.px[1]) < tol and abs(last.tz) < tol:
            converged = True
            break
    total = AttrDict(last, tx=px_x * gsd_x, ty=px_y * gsd_y, tz=tz, px=(px_x, px_y))
    return AttrDict(shifted=_translate(src, nd, px_x, px_y, tz, float(fill)), shift=total, history=history, converged=converged)
