"""Ortho-rectification of satellite views onto the grid of a DSM on the GPU (include/resdepth_hip_ortho.h): every DSM pixel is
taken to longitude / latitude (from a geographic or a UTM grid), projected into each image by its rational polynomial camera
model (RPC00B) in fp64 and the image resampled there.  The result is the `orthos = [V, H, W]` stack GpuPatchSampler and the tiled
sweep take.

The reference assumes "that the images have already been ortho-rectified with the help of the initial DSM" (README lines 56-58
and 68) and has none of this.  No CPU fallback: the projection and the resampling are one kernel of libresdepth_hip.so;
RPC.project is a host-side spot check in numpy.
"""
from __future__ import annotations

import math
import os
import re

import numpy as np
import torch

from ._lib import (ORTHO_CRS, ORTHO_DTYPES, ORTHO_MAX_VIEWS, ORTHO_RESAMPLING, ORTHO_VIEW_BYTES, check, load, ptr, stream_ptr)
from .evaluation import _first_device

_SCALARS = ("line_off", "samp_off", "lat_off", "lon_off", "height_off", "line_scale", "samp_scale", "lat_scale", "lon_scale",
            "height_scale")
_VECTORS = ("line_num", "line_den", "samp_num", "samp_den")
# GDAL's RPC metadata names / the names of the vendors' _RPC.TXT files, in the order of _SCALARS and _VECTORS
_GDAL_SCALARS = ("LINE_OFF", "SAMP_OFF", "LAT_OFF", "LONG_OFF", "HEIGHT_OFF", "LINE_SCALE", "SAMP_SCALE", "LAT_SCALE", "LONG_SCALE",
                 "HEIGHT_SCALE")
_GDAL_VECTORS = ("LINE_NUM_COEFF", "LINE_DEN_COEFF", "SAMP_NUM_COEFF", "SAMP_DEN_COEFF")
_NUMBER = re.compile(r"[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?")

# rd_ortho_view (include/resdepth_hip_ortho.h), 776 bytes
_VIEW_DESC = np.dtype([("image", "<u8"), ("pitch", "<i8"), ("rows", "<i4"), ("cols", "<i4"), ("dtype", "<i4"), ("reserved", "<i4"),
                       ("line0", "<f8"), ("samp0", "<f8"), ("image_nodata", "<f8")]
                      + [(name, "<f8") for name in _SCALARS] + [(name, "<f8", (20,)) for name in _VECTORS])
assert _VIEW_DESC.itemsize == ORTHO_VIEW_BYTES


def monomials(P, L, H):
    """the 20 monomials of RPC00B in its order, stacked on a new first axis"""
    one = np.ones_like(P)
    return np.stack([one, L, P, H, L * P, L * H, P * H, L * L, P * P, H * H, P * L * H, L * L * L, L * P * P, L * H * H, L * L * P,
                     P * P * P, P * H * H, L * L * H, P * P * H, H * H * H])


def _first_number(value, name):
    """'+004032.00 pixels' -> 4032.0: the number, whatever unit follows it"""
    if isinstance(value, str):
        m = _NUMBER.search(value)
        if not m:
            raise ValueError(f"RPC: no number in {name} = {value!r}")
        return float(m.group(0))
    return float(value)


class RPC:
    """An RPC00B camera model: ground (longitude, latitude in degrees on WGS84, ellipsoidal height in metres) -> image (line,
    sample).  Fields: line_off, samp_off, lat_off, lon_off, height_off, line_scale, samp_scale, lat_scale, lon_scale, height_scale
    (floats) and line_num, line_den, samp_num, samp_den (20 fp64 coefficients each, RPC00B order)."""

    def __init__(self, **fields):
        missing = [n for n in _SCALARS + _VECTORS if n not in fields]
        extra = [n for n in fields if n not in _SCALARS + _VECTORS]
        if missing or extra:
            raise ValueError(f"RPC: missing fields {missing}, unknown fields {extra}")
        for n in _SCALARS:
            setattr(self, n, float(fields[n]))
        for n in _VECTORS:
            v = np.array(fields[n], dtype=np.float64).reshape(-1)
            if v.size != 20:
                raise ValueError(f"RPC: {n} has {v.size} coefficients, 20 expected")
            setattr(self, n, v)
        self._check()

    def _check(self):
        for n in _SCALARS:
            if not math.isfinite(getattr(self, n)):
                raise ValueError(f"RPC: {n} = {getattr(self, n)!r} is not finite")
        for n in ("line_scale", "samp_scale", "lat_scale", "lon_scale", "height_scale"):
            if getattr(self, n) == 0.0:
                raise ValueError(f"RPC: {n} is zero")
        for n in _VECTORS:
            if not np.isfinite(getattr(self, n)).all():
                raise ValueError(f"RPC: {n} holds a value that is not finite")

    # ---- the two text forms ---------------------------------------------------------------------------------------------------
    @classmethod
    def from_dict(cls, d):
        """GDAL's RPC metadata domain: LINE_OFF ... HEIGHT_SCALE as numbers or strings, LINE_NUM_COEFF ... SAMP_DEN_COEFF as 20
        space-separated numbers or as sequences."""
        fields = {}
        for ours, key in zip(_SCALARS, _GDAL_SCALARS):
            if key not in d:
                raise ValueError(f"RPC.from_dict: {key} is missing")
            fields[ours] = _first_number(d[key], key)
        for ours, key in zip(_VECTORS, _GDAL_VECTORS):
            if key not in d:
                raise ValueError(f"RPC.from_dict: {key} is missing")
            v = d[key]
            fields[ours] = [float(t) for t in v.replace(",", " ").split()] if isinstance(v, str) else [float(t) for t in v]
        return cls(**fields)

    def to_dict(self):
        d = {key: repr(getattr(self, ours)) for ours, key in zip(_SCALARS, _GDAL_SCALARS)}
        d.update({key: " ".join(repr(float(c)) for c in getattr(self, ours)) for ours, key in zip(_VECTORS, _GDAL_VECTORS)})
        return d

    @classmethod
    def from_rpc_txt(cls, path_or_text):
        """The vendors' _RPC.TXT form: `LINE_OFF: +004032.00 pixels`, `LINE_NUM_COEFF_1: -1.2E-03`, ... -- a path, or the text
        itself (anything with a line break or a colon in it)."""
        text = os.fspath(path_or_text)
        if "\n" not in text and ":" not in text:
            with open(text) as f:
                text = f.read()
        seen = {}
        for line in text.splitlines():
            if ":" in line:
                key, value = line.split(":", 1)
                seen[key.strip().upper()] = value.strip().rstrip(";")
        d = {}
        for key in _GDAL_SCALARS:
            if key not in seen:
                raise ValueError(f"RPC.from_rpc_txt: {key} is missing")
            d[key] = seen[key]
        for key in _GDAL_VECTORS:
            try:
                d[key] = [_first_number(seen[f"{key}_{i}"], f"{key}_{i}") for i in range(1, 21)]
            except KeyError as e:
                raise ValueError(f"RPC.from_rpc_txt: {e.args[0]} is missing") from None
        return cls.from_dict(d)

    def to_rpc_txt(self):
        units = ("pixels", "pixels", "degrees", "degrees", "meters") * 2
        lines = [f"{key}: {getattr(self, ours)!r} {unit}" for ours, key, unit in zip(_SCALARS, _GDAL_SCALARS, units)]
        for ours, key in zip(_VECTORS, _GDAL_VECTORS):
            lines += [f"{key}_{i + 1}: {float(c)!r}" for i, c in enumerate(getattr(self, ours))]
        return "\n".join(lines) + "\n"

    # ---- the projection on the host --------------------------------------------------------------------------------------------
    def project(self, lon, lat, h):
        """numpy fp64 on the host, for spot checks -> (line, samp), broadcast over the arguments"""
        lon, lat, h = np.broadcast_arrays(np.asarray(lon, np.float64), np.asarray(lat, np.float64), np.asarray(h, np.float64))
        P, L, H = (lat - self.lat_off) / self.lat_scale, (lon - self.lon_off) / self.lon_scale, (h - self.height_off) / self.height_scale
        m = monomials(P, L, H)
        poly = lambda k: np.tensordot(k, m, axes=(0, 0))
        line = poly(self.line_num) / poly(self.line_den) * self.line_scale + self.line_off
        samp = poly(self.samp_num) / poly(self.samp_den) * self.samp_scale + self.samp_off
        return line, samp


# ---- arguments, checked on the host before a device is needed ---------------------------------------------------------------------
def _finite(v, who, name):
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: {name} {v!r} must be a number") from None
    if not math.isfinite(v):
        raise ValueError(f"{who}: {name} {v!r} must be finite")
    return v


def _grid(dsm, geotransform, crs, who):
    """-> (rows, cols, x0, dx, y0, dy, crs id, lon0_deg, false_northing)"""
    shape = tuple(np.shape(dsm))
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"{who}: dsm must be a non-empty 2-D raster, got shape {shape}")
    if shape[0] * shape[1] >= 1 << 31:
        raise ValueError(f"{who}: dsm of {shape[0]} x {shape[1]} pixels, fewer than 2^31 are taken")
    try:
        gt = [float(v) for v in geotransform]
    except (TypeError, ValueError):
        raise ValueError(f"{who}: geotransform {geotransform!r} must be GDAL's six numbers") from None
    if len(gt) != 6 or not all(math.isfinite(v) for v in gt):
        raise ValueError(f"{who}: geotransform {geotransform!r} must be six finite numbers")
    if gt[2] != 0.0 or gt[4] != 0.0:
        raise ValueError(f"{who}: geotransform {geotransform!r} is rotated (terms 2 and 4 must be zero)")
    if gt[1] == 0.0 or gt[5] == 0.0:
        raise ValueError(f"{who}: geotransform {geotransform!r} has a pixel size of zero")
    if crs == "geographic":
        return shape + (gt[0], gt[1], gt[3], gt[5], ORTHO_CRS["geographic"], 0.0, 0.0)
    if isinstance(crs, (tuple, list)) and len(crs) == 3 and crs[0] == "utm":
        zone, hemi = crs[1], crs[2]
        if isinstance(zone, (int, np.integer)) and not isinstance(zone, bool) and 1 <= zone <= 60 and hemi in ("N", "S"):
            return shape + (gt[0], gt[1], gt[3], gt[5], ORTHO_CRS["utm"], 6.0 * int(zone) - 183.0, 0.0 if hemi == "N" else 1.0e7)
    raise ValueError(f"{who}: crs {crs!r} must be \"geographic\" or (\"utm\", zone 1..60, \"N\" | \"S\")")


def _per_view(v, n, who, name):
    """a scalar for all views or one entry per view -> list of n"""
    if isinstance(v, (list, tuple)) and not (name == "image_window" and len(v) == 2 and not isinstance(v[0], (list, tuple))):
        if len(v) != n:
            raise ValueError(f"{who}: {name} has {len(v)} entries for {n} images")
        return list(v)
    return [v] * n


def _image_kind(im, who, i):
    """-> (dtype name, rows, cols, pitch in elements or None when the rows must be made contiguous)"""
    if torch.is_tensor(im):
        name = {torch.uint8: "uint8", torch.uint16: "uint16", torch.float32: "float32"}.get(im.dtype)
        shape, strides = tuple(im.shape), tuple(im.stride()) if im.dim() == 2 else None
    elif isinstance(im, np.ndarray):
        name = im.dtype.name if im.dtype.name in ORTHO_DTYPES else None
        shape, strides = im.shape, tuple(s // max(im.itemsize, 1) for s in im.strides) if im.ndim == 2 else None
    else:
        raise ValueError(f"{who}: images[{i}] must be a tensor or a numpy array, got {type(im).__name__}")
    if name is None:
        raise ValueError(f"{who}: images[{i}] has dtype {im.dtype}, expected uint8, uint16 or float32")
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"{who}: images[{i}] must be a non-empty 2-D array, got shape {shape}")
    direct = strides[1] == 1 and strides[0] >= shape[1]
    return name, shape[0], shape[1], (strides[0] if direct else None)


def _arguments(images, rpcs, dsm, geotransform, crs, nodata, height_offset, resampling, image_nodata, image_origin, image_window,
               fill, who):
    grid = _grid(dsm, geotransform, crs, who)
    if not isinstance(images, (list, tuple)) or not 1 <= len(images) <= ORTHO_MAX_VIEWS:
        raise ValueError(f"{who}: images must be a list of 1..{ORTHO_MAX_VIEWS} 2-D arrays")
    if not isinstance(rpcs, (list, tuple)) or len(rpcs) != len(images) or not all(isinstance(r, RPC) for r in rpcs):
        raise ValueError(f"{who}: rpcs must be a list of one RPC per image ({len(images)})")
    n = len(images)
    kinds = [_image_kind(im, who, i) for i, im in enumerate(images)]
    if resampling not in ORTHO_RESAMPLING:
        raise ValueError(f"{who}: resampling {resampling!r} must be one of {sorted(ORTHO_RESAMPLING)}")
    nd = float("nan") if nodata is None else float(nodata)
    hoff = _finite(height_offset, who, "height_offset")
    try:
        fill = float(fill)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: fill {fill!r} must be a number") from None
    inod = [float("nan") if v is None else float(v) for v in _per_view(image_nodata, n, who, "image_nodata")]
    origin = [_finite(v, who, "image_origin") for v in _per_view(image_origin, n, who, "image_origin")]
    window = []
    for wv in _per_view(image_window, n, who, "image_window"):
        if wv is None:
            wv = (0.0, 0.0)
        if not isinstance(wv, (list, tuple)) or len(wv) != 2:
            raise ValueError(f"{who}: image_window {wv!r} must be (row0, col0)")
        window.append((_finite(wv[0], who, "image_window"), _finite(wv[1], who, "image_window")))
    return grid, kinds, nd, hoff, ORTHO_RESAMPLING[resampling], fill, inod, origin, window


def _device_image(im, kind, dev):
    """-> (device tensor that owns the elements, pitch in elements)"""
    name, rows, cols, pitch = kind
    if torch.is_tensor(im):
        if pitch is None:
            im, pitch = im.contiguous(), cols
        if im.device != dev:                            # a copy keeps the elements only: it is contiguous
            im, pitch = im.contiguous().to(dev), cols
        return im, pitch
    a = np.ascontiguousarray(im)
    if name == "uint16":
        a = a.view(np.int16)                            # the bytes are what travels
    return torch.from_numpy(a).to(dev), cols


def _run(images, rpcs, dsm, args, want_valid, want_coords, device):
    (rows, cols, x0, dx, y0, dy, crs_id, lon0, fnorth), kinds, nd, hoff, rs, fill, inod, origin, window = args
    dev = _first_device(dsm, *images, default=device)
    z = (dsm if torch.is_tensor(dsm) else torch.from_numpy(np.ascontiguousarray(dsm))).to(dev, torch.float32).contiguous()
    n = len(images)
    held = []
    desc = np.zeros(n, dtype=_VIEW_DESC)
    for i, (im, rpc, kind) in enumerate(zip(images, rpcs, kinds)):
        t, pitch = _device_image(im, kind, dev)
        held.append(t)
        d = desc[i]
        d["image"], d["pitch"], d["rows"], d["cols"], d["dtype"] = t.data_ptr(), pitch, kind[1], kind[2], ORTHO_DTYPES[kind[0]]
        d["line0"], d["samp0"], d["image_nodata"] = origin[i] + window[i][0], origin[i] + window[i][1], inod[i]
        for name in _SCALARS + _VECTORS:
            d[name] = getattr(rpc, name)
    views = torch.from_numpy(desc.view(np.uint8).reshape(-1)).to(dev)
    # out is always written (the C ABI has no call without it); project_grid drops it
    out = torch.empty((n, rows, cols), dtype=torch.float32, device=dev)
    valid = torch.empty((n, rows, cols), dtype=torch.uint8, device=dev) if want_valid else None
    coords = torch.empty((n, rows, cols, 2), dtype=torch.float64, device=dev) if want_coords else None
    with torch.cuda.device(dev):
        check(load().rd_ortho_rpc(ptr(z), rows, cols, x0, dx, y0, dy, crs_id, lon0, fnorth, nd, hoff, ptr(views), n, rs, fill,
                                  ptr(out), ptr(valid), ptr(coords), stream_ptr()), "ortho_rpc")
    del held                                            # the launch is queued on this stream: the allocator orders the reuse
    return out, valid, coords


# ---- the front end ------------------------------------------------------------------------------------------------------------------
def orthorectify(images, rpcs, dsm, geotransform, crs, *, nodata=-9999.0, height_offset=0.0, resampling="bilinear",
                 image_nodata=None, image_origin=0.0, image_window=None, fill=0.0, return_valid=False, return_coords=False,
                 device="cuda"):
    """Raw views -> ortho-images on the grid of `dsm` (rd_ortho_rpc, include/resdepth_hip_ortho.h): [P, H, W] float32 on the DSM's
    device, the layout GpuPatchSampler(orthos=...) takes.  Rendering again over a refined DSM is the same call with dsm=refined.

    images        list of 1..16 2-D tensors / numpy arrays, uint8 / uint16 / float32, of any shapes; a tensor already on the
                  device is read in place, rows that are not contiguous through their pitch
    rpcs          one RPC per image
    dsm           [H, W] heights (ellipsoidal metres after height_offset), read as float32; `nodata` (None: none) and NaN
                  pixels are undefined in every view
    geotransform  GDAL's six numbers (x of the left edge, pixel width, 0, y of the top edge, 0, pixel height: usually negative);
                  rotation terms are refused
    crs           "geographic" (degrees on WGS84) or ("utm", zone, "N" | "S")
    height_offset a constant added to the DSM: the geoid undulation when the DSM is orthometric
    resampling    "nearest", "bilinear" or "bicubic" (Catmull-Rom)
    image_nodata  image values that are no data (one for all or one per image; None: none)
    image_origin  the line / sample coordinate of the CENTRE of a scene's first pixel: 0.0 as in the vendors' files, 0.5 for
                  corner-based models
    image_window  (row0, col0) of a crop in its scene, or one pair per image
    fill          what undefined pixels hold
    -> out, or (out[, valid [P, H, W] bool][, coords [P, H, W, 2] fp64 = (row, column) in the image])
    ValueError for bad arguments, the argument named, before any launch."""
    who = "orthorectify"
    args = _arguments(images, rpcs, dsm, geotransform, crs, nodata, height_offset, resampling, image_nodata, image_origin,
                      image_window, fill, who)
    out, valid, coords = _run(images, rpcs, dsm, args, bool(return_valid), bool(return_coords), device)
    res = (out,) + ((valid.view(torch.bool),) if return_valid else ()) + ((coords,) if return_coords else ())
    return res if len(res) > 1 else out


def project_grid(images, rpcs, dsm, geotransform, crs, *, nodata=-9999.0, height_offset=0.0, image_origin=0.0, image_window=None,
                 device="cuda"):
    """Where every DSM pixel falls in every image -> coords [P, H, W, 2] fp64 = (row, column) in elements from the centre of the
    image's first element, NaN where the DSM is undefined.  The arguments are orthorectify's; the images give their shapes only
    as far as the result goes."""
    who = "project_grid"
    args = _arguments(images, rpcs, dsm, geotransform, crs, nodata, height_offset, "nearest", None, image_origin, image_window,
                      0.0, who)
    return _run(images, rpcs, dsm, args, False, True, device)[2]
