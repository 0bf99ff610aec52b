"""Masked residual statistics on the GPU: the reference's `compute_residuals` + `get_statistics`
(lib/evaluation.py:11-131) for rasters resident in HBM (a city-scale DSM is 10^8 pixels; the reference does this with
numpy masked arrays and three full sorts on the CPU).  Returns the reference's statistic names as python floats."""
from __future__ import annotations

import ctypes
import logging
import os

import numpy as np
import torch

from ._lib import check, load, ptr, stream_ptr, workspace

_KEYS = ["count_total", "diff_max", "diff_min", "MAE", "RMSE", "absolute_median", "median", "NMAD"]


def _stats(raster, gt, mask, nodata, thr, out):
    """rd_residual_stats (the single-set engine) into `out`, a device row of eight, enqueued only."""
    n = raster.numel()
    ws = workspace(load().rd_residual_stats_ws_bytes(n), out.device, slot=2)
    check(load().rd_residual_stats(ptr(raster), ptr(gt), ptr(mask), n, float(nodata), float(thr if thr else -1.0), ptr(out),
                                   ws.data_ptr(), ws.numel(), stream_ptr()), "residual_stats")


def get_statistics(raster, raster_gt, nodata, mask_gt=None, residual_threshold=None, device="cuda", *, abs_quantiles=None,
                   quantiles=None, within=None):
    """raster: refined DSM (any float dtype, e.g. the float64 output of predict_linear_blend), raster_gt: reference DSM,
    mask_gt: optional boolean validity mask.  -> dict as lib/evaluation.py:get_statistics (incl. 'truncated' sub-dict
    when residual_threshold is given).  abs_quantiles / quantiles / within: see evaluate_statistics."""
    dev = _device(device, "resdepth_amd.evaluation.get_statistics")
    dist = _dist_options(abs_quantiles, quantiles, within)
    r, g = _on(raster, dev, torch.float64), _on(raster_gt, dev, torch.float32)
    m = None if mask_gt is None else _on(mask_gt, dev).to(torch.uint8).contiguous()
    thr = residual_threshold
    sets = [(0, 1, t) for t in _variants(thr)]
    rows = _Rows(len(sets), dist, r.device)
    with torch.cuda.device(r.device):              # raw launches go to the current device's stream
        for out, (_, _, t) in zip(rows.stats, sets):
            _stats(r, g, m, nodata, t, out)        # the eight numbers stay with the single-set engine
        if dist is not None:
            # the sets form over the residual and validity of residual_kernel (d = a - (double)g; valid = both != nodata,
            # under the mask), built here; the truncated set is its second set
            gd = g.to(torch.float64)
            ok = (r != nodata) & (gd != nodata)
            if m is not None:
                ok &= m != 0
            rows.sets((r - gd).reshape(-1), None, ok.to(torch.uint8).reshape(-1), sets, quantiles_only=True)
    full, trunc = _full_and_truncated(rows.host(), 0, thr)
    stats = {"truncation": bool(thr)}              # a plain dict in the reference's key order, not _stats_dict's
    stats.update(zip(_KEYS, (float(v) for v in full)))
    if thr:
        stats["truncated"] = dict(_truncated_dict(trunc, thr, dist))
    _fill(dist, stats, full)
    return stats


# ---- class-partitioned evaluation (lib/evaluation.py:134-457: print_statistics, evaluate_performance) ----------------
VALID_BEFORE, VALID_AFTER = 1, 2                      # class bits of rd_eval_classify (include/resdepth_hip.h RD_CLS_*)
CLASS_BITS = {"all": 0, "building": 4, "terrain": 8, "terrain_nowater": 16, "terrain_nowater_noforest": 32}
MAX_SETS = 20                                         # RD_STATS_MAX_SETS
MAX_DILATE = 8                                        # RD_DILATE_MAX_ITER: larger radii chain launches


class AttrDict(dict):
    """dict with attribute access (the reference's EasyDict): `stats.MAE`, `residuals.all`."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k) from None

    __setattr__ = dict.__setitem__


def _device(dev, who="resdepth_amd.evaluation"):
    dev = torch.device(dev)
    if dev.type != "cuda":
        raise RuntimeError(f"{who} needs a HIP device (no CPU fallback)")
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


def _first_device(*xs, default):
    """The device of the first CUDA tensor among xs, else `default`."""
    return _device(next((x.device for x in xs if torch.is_tensor(x) and x.is_cuda), default))


def _on(x, dev, dtype=None):
    """numpy array / tensor -> contiguous tensor on `dev` (dtype kept unless given)."""
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    return t.to(dev, dtype).contiguous() if dtype is not None else t.to(dev).contiguous()


def _dilate_u8(m, iterations):
    """uint8 0/1 device raster -> dilated uint8 0/1 raster (rd_dilate_mask, radius chained in steps of <= 8)."""
    rows, cols = m.shape
    lib = load()
    with torch.cuda.device(m.device):
        while iterations > 0:
            k = min(iterations, MAX_DILATE)
            out = torch.empty_like(m)
            check(lib.rd_dilate_mask(ptr(m), ptr(out), rows, cols, k, stream_ptr()), "dilate_mask")
            m, iterations = out, iterations - k
    return m


def dilate_mask(mask, iterations=1, device="cuda"):
    """GPU counterpart of lib/rasterutils.py:88 dilate_mask: scipy.ndimage.binary_dilation(mask, iterations=k) with the
    default cross structure (the L1 ball of radius k; pixels outside the raster count as unset), k >= 1.  Takes a 2-D
    numpy array or tensor (nonzero = set) and returns the same kind: a bool ndarray, or a bool tensor on the input's
    device."""
    iterations = int(iterations)
    if iterations < 1:
        raise ValueError(f"dilate_mask: iterations must be >= 1 (got {iterations})")
    if len(mask.shape) != 2 or min(mask.shape) == 0:
        raise ValueError(f"dilate_mask: expected a non-empty 2-D raster, got shape {tuple(mask.shape)}")
    dev = _device(mask.device if torch.is_tensor(mask) and mask.is_cuda else device)
    m = _on(mask, dev)
    m = (m != 0).to(torch.uint8).contiguous()
    out = _dilate_u8(m, iterations).bool()
    if torch.is_tensor(mask):
        return out.to(mask.device)
    return out.cpu().numpy()


def _mask_pair(spec, dev):
    """A mask argument -> (mask, nodata_mask) uint8 device rasters, converted like lib/rasterutils.py:23
    load_mask_raster: set where the value is 1 and not the nodata value.  `spec`: an array / tensor, a
    (values, nodata) tuple or a dataset-like object (ReadAsArray(), GetRasterBand(1).GetNoDataValue())."""
    if hasattr(spec, "ReadAsArray"):
        values, nd = spec.ReadAsArray(), spec.GetRasterBand(1).GetNoDataValue()
    elif isinstance(spec, tuple):
        values, nd = spec
    else:
        values, nd = spec, None
    v = _on(values, dev)
    if v.dtype == torch.bool:
        v = v.to(torch.uint8)
    nodata = torch.zeros(v.shape, dtype=torch.bool, device=dev) if nd is None else (v == nd)
    return ((v == 1) & ~nodata).to(torch.uint8).contiguous(), nodata.to(torch.uint8).contiguous()


def _rects(area_defn, rows, cols):
    """area_defn (inclusive x / y extents per stripe) -> half-open [y0, y1, x0, x1) rows, numpy slicing semantics."""
    if area_defn is None:
        return None
    out = []
    for x, y in zip(area_defn["x_extent"], area_defn["y_extent"]):
        y0, y1, _ = slice(int(y[0]), int(y[1]) + 1).indices(rows)
        x0, x1, _ = slice(int(x[0]), int(x[1]) + 1).indices(cols)
        out.append((y0, max(y0, y1), x0, max(x0, x1)))
    return out


def _set_arrays(sets):
    """[([source,] need bits, threshold or None)] -> the ctypes arrays (need, thr[, src]) of a statistics call."""
    ns = len(sets)
    need_a = (ctypes.c_int * ns)(*[s[-2] for s in sets])
    thr_a = (ctypes.c_double * ns)(*[float(s[-1]) if s[-1] else -1.0 for s in sets])
    return (need_a, thr_a) if len(sets[0]) == 2 else (need_a, thr_a, (ctypes.c_int * ns)(*[s[0] for s in sets]))


# ---- error quantiles and within-tolerance shares (include/resdepth_hip_dist.h) -------------------------------------------
LE = (0.68, 0.90, 0.95)                               # the usual linear-error levels: abs_quantiles=LE gives LE68, LE90, LE95
MAX_Q = MAX_T = 8                                     # RD_DIST_MAX_Q, RD_DIST_MAX_T


class _Dist:
    """The quantile / share options of one call: the ctypes arrays of rd_residual_dist_*, the width of an output row
    (count, quantiles, shares) and the way from such a row into a statistics dict."""

    def __init__(self, abs_q, q, within):
        self.abs_q, self.q, self.within = abs_q, q, within
        levels = [(v, 1) for v in abs_q] + [(v, 0) for v in q]
        if len(levels) > MAX_Q or len(within) > MAX_T:
            raise ValueError(f"evaluate: {len(levels)} quantiles (at most {MAX_Q}) and {len(within)} tolerances (at most "
                             f"{MAX_T}) in one call")
        for v, _ in levels:
            if not 0.0 <= v <= 1.0:
                raise ValueError(f"evaluate: quantile level {v} outside [0, 1]")
        for t in within:
            if not 0.0 <= t < float("inf"):
                raise ValueError(f"evaluate: tolerance {t} must be finite and >= 0")
        self.n_q, self.n_t = len(levels), len(within)
        self.width = 1 + self.n_q + self.n_t
        self.q_a = (ctypes.c_double * max(self.n_q, 1))(*[v for v, _ in levels])
        self.mode_a = (ctypes.c_int * max(self.n_q, 1))(*[m for _, m in levels])
        self.tau_a = (ctypes.c_double * max(self.n_t, 1))(*within)

    def fill(self, st, row):
        """row (count, quantiles, shares) of one set -> the keys of the options that were given"""
        v = [float(x) for x in row[1:]]
        na = len(self.abs_q)
        if self.abs_q:
            st["abs_quantile"] = dict(zip(self.abs_q, v[:na]))
        if self.q:
            st["quantile"] = dict(zip(self.q, v[na:self.n_q]))
        if self.within:
            st["within"] = dict(zip(self.within, v[self.n_q:]))


def _dist_options(abs_quantiles, quantiles, within):
    """-> a _Dist, or None when no option is given (the call then does exactly what it did without them)."""
    abs_q, q, w = (tuple(float(v) for v in (x if x is not None else ())) for x in (abs_quantiles, quantiles, within))
    return _Dist(abs_q, q, w) if abs_q or q or w else None


def _variants(thr):
    """The thresholds of a set and, under a threshold, of its truncated set: sets are built, and their rows walked, in such
    (full, truncated) steps."""
    return (None, thr) if thr else (None,)


def _full_and_truncated(rows, q, thr):
    """-> (the full row, the truncated row or None) of the q-th set of rows laid out in _variants steps"""
    step = len(_variants(thr))
    return rows[q * step], (rows[q * step + 1] if thr else None)


class _Rows:
    """The result rows of one evaluation call: ONE float64 device buffer -- the [n_rows, 8] block the statistics kernels write
    and behind it the [n_rows, dist.width] block of the quantile kernels (width 0 without options, and then nothing is
    queued for it) -- filled in the order the sets are queued and read back once."""

    def __init__(self, n_rows, dist, dev):
        self.dist, self.dev, self.n_rows, self.used = dist, dev, n_rows, 0
        self.width = dist.width if dist is not None else 0
        self.buf = torch.empty(n_rows * (8 + self.width), dtype=torch.float64, device=dev)
        self.stats = self.buf[:n_rows * 8].view(n_rows, 8)
        self.quant = self.buf[n_rows * 8:].view(n_rows, self.width)

    def _queue(self, stats, quant, n, args):
        """Entry point rd_<stats> (None: left out) and, with options, rd_<quant> with `args`, which end in the set arrays and the
        number of sets, into the next rows; enqueued only."""
        lib, dist, ns = load(), self.dist, args[-1]
        r0, self.used = self.used, self.used + ns
        if self.used > self.n_rows:
            raise RuntimeError(f"evaluate: {self.used} result rows queued into a buffer of {self.n_rows}")
        with torch.cuda.device(self.dev):
            if stats is not None:
                ws = workspace(getattr(lib, f"rd_{stats}_ws_bytes")(n, ns), self.dev, slot=3)
                check(getattr(lib, "rd_" + stats)(*args, ptr(self.stats[r0:self.used]), ws.data_ptr(), ws.numel(), stream_ptr()),
                      stats)
            if dist is not None:
                ws = workspace(getattr(lib, f"rd_{quant}_ws_bytes")(n, ns, dist.n_q, dist.n_t), self.dev, slot=4)
                check(getattr(lib, "rd_" + quant)(*args, dist.q_a, dist.mode_a, dist.n_q, dist.tau_a, dist.n_t,
                                                  ptr(self.quant[r0:self.used]), ws.data_ptr(), ws.numel(), stream_ptr()), quant)

    def sets(self, src0, src1, cls, sets, quantiles_only=False):
        """sets: [(source, need bits, threshold or None)] over the sources and the class byte -> len(sets) rows
        (rd_residual_stats_sets, rd_residual_dist_sets), in calls of at most MAX_SETS sets."""
        n = cls.numel()
        for k in range(0, len(sets), MAX_SETS):
            need_a, thr_a, src_a = _set_arrays(sets[k:k + MAX_SETS])
            self._queue(None if quantiles_only else "residual_stats_sets", "residual_dist_sets", n,
                        (ptr(src0), ptr(src1), ptr(cls), n, src_a, need_a, thr_a, len(need_a)))

    def pooled(self, res, n_planes, p0, p1, cls, valid, sets):
        """sets: [(need bits, threshold or None)] over planes p0 .. p1 - 1 of `res` [P, rows, cols] -> len(sets) rows
        (rd_residual_stats_pooled, rd_residual_dist_pooled)."""
        n = cls.numel()
        need_a, thr_a = _set_arrays(sets)
        self._queue("residual_stats_pooled", "residual_dist_pooled", n,
                    (ptr(res), n, n_planes, p0, p1, ptr(cls), ptr(valid), n, need_a, thr_a, len(sets)))

    def host(self):
        """The one read-back -> [n_rows, 8 + width]: a row carries its eight numbers and behind them its (count, quantiles,
        shares)."""
        h, n = self.buf.cpu().numpy(), self.n_rows
        return np.concatenate((h[:n * 8].reshape(n, 8), h[n * 8:].reshape(n, self.width)), axis=1)


def _fill(dist, st, row):
    """The quantile part of a host row of _Rows into st, under the keys of the options given (none: nothing)."""
    if dist is not None:
        dist.fill(st, row[8:])


def _truncated_dict(row, thr, dist):
    """The 'truncated' sub-dict of the reference's get_statistics from the row of a truncated set."""
    st = AttrDict(count_total=float(row[0]), threshold=thr, MAE=float(row[3]), RMSE=float(row[4]),
                  absolute_median=float(row[5]), median=float(row[6]), NMAD=float(row[7]))
    _fill(dist, st, row)
    return st


def _stats_dict(full, trunc, thr, dist=None):
    """host rows of _Rows (or rows of eight) -> the reference's get_statistics dict [with the abs_quantile / quantile / within keys
    of the options given, in the truncated sub-dict too]."""
    st = AttrDict(truncation=bool(thr))
    if thr:
        st.truncated = _truncated_dict(trunc, thr, dist)
    st.update(zip(_KEYS, (float(v) for v in full)))        # the zip ends with the eight names
    _fill(dist, st, full)
    return st


def _class_stats(rows, classes, thr, dist=None):
    """host rows [len(classes) * (2 if thr else 1), 8 + width] in class order (full, truncated) -> {class: stats}"""
    return AttrDict((c, _stats_dict(*_full_and_truncated(rows, q, thr), thr, dist)) for q, c in enumerate(classes))


def _float_raster(x, dev):
    """DSM as given when f32 / f64 (never rounded), anything else as f64."""
    t = _on(x, dev)
    return t if t.dtype in (torch.float32, torch.float64) else t.to(torch.float64)


def _eval_inputs(rows, cols, area_defn, mask_gt, mask_building, mask_water, mask_forest, nodata, dev):
    """What a classification pass needs besides the DSMs -> (classes, masks, grid): the classes the masks define; the uint8
    device masks gm, bdil (building, already dilated), bnod, water, forest, which the caller holds until its launch is queued;
    and the area rectangles as a ctypes array, their number, the raster shape and the nodata value.  `*map(ptr, masks), *grid`
    is the run of arguments rd_eval_classify and rd_eval_classify_planes take in the same order."""
    gm = None if mask_gt is None else _mask_pair(mask_gt, dev)[0]
    bdil = bnod = water = forest = None
    classes = ["all"]
    if mask_building is not None:
        b, bnod = _mask_pair(mask_building, dev)
        bdil = _dilate_u8(b, 2)                        # lib/evaluation.py:282: dilated on the whole raster
        classes += ["building", "terrain"]
        if mask_water is not None:
            water = _mask_pair(mask_water, dev)[0]
            classes.append("terrain_nowater")
        if mask_forest is not None:
            forest = _mask_pair(mask_forest, dev)[0]
            classes.append("terrain_nowater_noforest")
    for name, m in (("gt mask", gm), ("building mask", bdil), ("water mask", water), ("forest mask", forest)):
        if m is not None and tuple(m.shape) != (rows, cols):
            raise ValueError(f"evaluate: {name} shape {tuple(m.shape)} != raster shape {(rows, cols)}")
    rects = _rects(area_defn, rows, cols)
    rect_a = None if rects is None else (ctypes.c_int * (4 * max(len(rects), 1)))(*[v for r in rects for v in r])
    nd = float("nan") if nodata is None else float(nodata)
    return classes, (gm, bdil, bnod, water, forest), (rect_a, -1 if rects is None else len(rects), rows, cols, nd)


def _classified(prediction, initial, gt, area_defn, mask_gt, mask_building, mask_water, mask_forest, nodata, dev, who):
    """The classification pass (rd_eval_classify) -> (r_before, r_after, cls, classes), all on the device.  initial None: the
    prediction stands in for it (r_before is then r_after and RD_CLS_VALID_BEFORE equals RD_CLS_VALID_AFTER)."""
    pred = _on(prediction, dev, torch.float64)
    init = pred if initial is None else _float_raster(initial, dev)
    g = _float_raster(gt, dev)
    if pred.dim() != 2 or pred.numel() == 0 or pred.shape != init.shape or pred.shape != g.shape:
        raise ValueError(f"{who}: prediction {tuple(pred.shape)}, initial {tuple(init.shape)} and ground truth "
                         f"{tuple(g.shape)} must be equal 2-D rasters")
    rows, cols = pred.shape
    classes, masks, grid = _eval_inputs(rows, cols, area_defn, mask_gt, mask_building, mask_water, mask_forest, nodata, dev)
    r_before = torch.empty((rows, cols), dtype=torch.float64, device=dev)
    r_after = torch.empty_like(r_before)
    cls = torch.empty((rows, cols), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(load().rd_eval_classify(ptr(pred), ptr(init), int(init.dtype == torch.float64), ptr(g),
                                      int(g.dtype == torch.float64), *map(ptr, masks), *grid, ptr(r_before), ptr(r_after),
                                      ptr(cls), stream_ptr()), "eval_classify")
    return r_before, r_after, cls, classes


def _evaluate(prediction, initial, gt, area_defn, mask_gt, mask_building, mask_water, mask_forest, residual_threshold,
              nodata, dev, dist=None):
    """-> (stats {'before', 'after'}, r_after, cls, classes) with r_after / cls on the device."""
    r_before, r_after, cls, classes = _classified(prediction, initial, gt, area_defn, mask_gt, mask_building, mask_water,
                                                  mask_forest, nodata, dev, "evaluate")
    thr = residual_threshold
    sets = [(src, valid | CLASS_BITS[c], t) for src, valid in ((0, VALID_BEFORE), (1, VALID_AFTER)) for c in classes
            for t in _variants(thr)]
    rows = _Rows(len(sets), dist, dev)
    rows.sets(r_before, r_after, cls, sets)
    host = rows.host()
    half = len(sets) // 2                              # source-major: the initial DSM's rows, then the refined DSM's
    stats = AttrDict(before=_class_stats(host[:half], classes, thr, dist), after=_class_stats(host[half:], classes, thr, dist))
    return stats, r_after, cls, classes


def evaluate_statistics(prediction, initial, gt, area_defn=None, mask_gt=None, mask_building=None, mask_water=None,
                        mask_forest=None, residual_threshold=None, *, nodata=None, device="cuda", abs_quantiles=None,
                        quantiles=None, within=None):
    """The statistics of lib/evaluation.py:163-457 evaluate_performance on the GPU: one classification pass, then every
    statistics set (initial / refined DSM x all / building / terrain / terrain without water / terrain without water and
    forest, each with its truncated variant) out of one shared set of radix-select passes.

    prediction: refined DSM; initial: initial DSM; gt: ground-truth DSM (numpy arrays or tensors; f32 / f64 DSMs are
    read as given).  nodata: the ground truth's nodata value (None: none).  Masks: arrays / tensors (value 1 = set),
    (values, nodata) tuples or dataset-like objects; water and forest only count with a building mask.
    -> {'before': {class: stats}, 'after': {class: stats}} in the reference's get_statistics format, attribute access.

    Beyond the reference, three keyword options add what accuracy specifications quote, for every set (the truncated ones
    too), by one rd_residual_dist_sets call over the same sets -- no sort, nothing but the results read back:
      abs_quantiles=  levels of |residual| (evaluation.LE = 0.68, 0.90, 0.95 gives LE68, LE90, LE95) -> stats.abs_quantile
      quantiles=      levels of the signed residual                                                  -> stats.quantile
      within=         tolerances in metres: the share of pixels with |residual| <= tolerance, 0..1   -> stats.within
    each a dict keyed by the level / tolerance as given; numpy's `linear` quantile rule (include/resdepth_hip_dist.h); at most
    8 levels and 8 tolerances.  Without them the dicts and the library calls are exactly what they were."""
    dev = _first_device(prediction, initial, gt, default=device)
    return _evaluate(prediction, initial, gt, area_defn, mask_gt, mask_building, mask_water, mask_forest,
                     residual_threshold, nodata, dev, _dist_options(abs_quantiles, quantiles, within))[0]


def _print_dist(st, logger, prefix=""):
    """One line per quantile / share present in st, in the block's number format."""
    name = (lambda text: prefix + text[0].lower() + text[1:]) if prefix else (lambda text: text)
    lines = []
    for q, v in st.get("abs_quantile", {}).items():
        lines.append((name("Linear error LE{:g} (|residual| quantile) [m]:".format(100 * q)), v, "m"))
    for q, v in st.get("quantile", {}).items():
        lines.append((name("Residual quantile q={:g} [m]:".format(q)), v, "m"))
    for tau, v in st.get("within", {}).items():
        lines.append((name("Share of pixels within {:.2f} m [%]:".format(tau)), 100.0 * v, "%"))
    for k, (text, v, unit) in enumerate(lines):
        tabs = "\t" * max(1, 9 - len(text) // 8)             # the value column of the reference's block (tab stop 72)
        logger.info("{}{}{:10.3f} {}{}".format(text, tabs, v, unit, "\n" if k == len(lines) - 1 else ""))


def print_statistics(stats, logger, print_min_max=True):
    """The report block of lib/evaluation.py:134-160, line for line; after it (and after the truncated block) one line per
    abs_quantile / quantile / within value, when the statistics carry those keys."""
    if print_min_max:
        logger.info("Maximum residual error [m]:\t\t\t\t\t\t{:10.3f} m".format(stats.diff_max))
        logger.info("Minimum residual error [m]:\t\t\t\t\t\t{:10.3f} m".format(stats.diff_min))
    logger.info("Mean absolute residual error (MAE) [m]:\t\t\t\t\t{:10.3f} m".format(stats.MAE))
    logger.info("RMSE residual error [m]:\t\t\t\t\t\t{:10.3f} m".format(stats.RMSE))
    logger.info("Absolute median residual error [m]:\t\t\t\t\t{:10.3f} m".format(stats.absolute_median))
    logger.info("Median residual error [m]:\t\t\t\t\t\t{:10.3f} m".format(stats.median))
    logger.info("Normalized median absolute deviation (NMAD) [m]:\t\t\t{:10.3f} m\n".format(stats.NMAD))
    _print_dist(stats, logger)
    if stats.truncation:
        t = stats.truncated
        logger.info("Truncated mean absolute residual error (MAE) [m]:\t\t\t{:10.3f} m".format(t.MAE))
        logger.info("Truncated RMSE residual error [m]:\t\t\t\t\t{:10.3f} m".format(t.RMSE))
        logger.info("Truncated absolute median residual error [m]:\t\t\t\t{:10.3f} m".format(t.absolute_median))
        logger.info("Truncated median residual error [m]:\t\t\t\t\t{:10.3f} m".format(t.median))
        logger.info("Truncated normalized median absolute deviation (NMAD) [m]:\t\t{:10.3f} m\n".format(t.NMAD))
        _print_dist(t, logger, "Truncated ")


def _gdal():
    try:
        from osgeo import gdal
    except ImportError as e:
        raise ImportError("resdepth_amd.evaluation: opening a raster from a path needs GDAL (osgeo.gdal), which is not "
                          "installed; pass arrays or opened datasets instead") from e
    return gdal


def _open(path):
    ds = _gdal().Open(path, 0)
    if ds is None:
        raise ValueError("Could not open {}".format(path))
    return ds


def _mask_arg(arg, what, logger_root):
    """A mask argument of evaluate_performance -> something _mask_pair takes, or None (absent / missing file)."""
    if arg is None or (isinstance(arg, str) and not arg):
        return None
    if isinstance(arg, str):
        if not os.path.exists(arg):
            logger_root.info("Cannot find the {}: {}".format(what, arg))
            return False
        logger_root.info("\tLoad the {}...".format(what))
        return _open(arg)
    return arg


# (class, report heading) in the reference's report order; the forest heading depends on whether water was given
_HEADINGS = {"all": "OVERALL", "building": "BUILDING PIXELS", "terrain": "TERRAIN PIXELS",
             "terrain_nowater": "TERRAIN PIXELS WITHOUT WATER",
             "terrain_nowater_noforest": ("TERRAIN PIXELS WITHOUT WATER/FOREST", "TERRAIN PIXELS WITHOUT FOREST")}


def _default_stats_logger(name="stats_logger"):
    logger_stats = logging.getLogger(name)
    logger_stats.setLevel(logging.INFO)
    if not logger_stats.handlers:
        logger_stats.addHandler(logging.StreamHandler())
    return logger_stats


def _raster_arg(x, what, logger_root):
    """A DSM argument -> (array, dataset or None): paths are opened, datasets read."""
    if isinstance(x, str):
        logger_root.info("\tLoad the {}...".format(what))
        x = _open(x)
    return (x.GetRasterBand(1).ReadAsArray(), x) if hasattr(x, "GetRasterBand") else (x, None)


def _performance_inputs(ds_raster_input, ds_raster_gt, logger_root, path_gt_mask, path_building_mask, path_water_mask,
                        path_forest_mask, nodata, gsd, who):
    """The arguments evaluate_performance shares with evaluate_pairs_performance, resolved in the reference's order
    -> (gt, init, nodata, gsd, mask_gt, mask_building, mask_water, mask_forest)."""
    gt, ds_gt = _raster_arg(ds_raster_gt, "ground truth DSM", logger_root)
    init, ds_in = _raster_arg(ds_raster_input, "initial DSM", logger_root)
    if ds_gt is not None:
        nodata = ds_gt.GetRasterBand(1).GetNoDataValue()
    if ds_in is not None:
        gsd = ds_in.GetGeoTransform()[1]
    if gsd is None:
        raise ValueError("{}: pass gsd= when the initial DSM is an array".format(who))

    mask_gt = _mask_arg(path_gt_mask, "ground truth mask", logger_root)
    if mask_gt is False:
        logger_root.info("Evaluating the performance by using all ground truth DSM pixels with a valid height.")
        mask_gt = None
    mask_b = _mask_arg(path_building_mask, "building mask", logger_root)
    mask_w = mask_f = None
    if mask_b is False:
        logger_root.info("Evaluating the performance over all pixels.")
        mask_b = None
    if path_building_mask is not None and not (isinstance(path_building_mask, str) and not path_building_mask):
        # the reference reads the water / forest masks only under a building mask
        mask_w = _mask_arg(path_water_mask, "water mask", logger_root)
        if mask_w is False:
            logger_root.info("Evaluating the performance without excluding water pixels.")
            mask_w = None
        mask_f = _mask_arg(path_forest_mask, "forest mask", logger_root)
        if mask_f is False:
            logger_root.info("Evaluating the performance without excluding forest pixels.")
            mask_f = None
    return gt, init, nodata, gsd, mask_gt, mask_b, mask_w, mask_f


def _heading(c, classes):
    head = _HEADINGS[c]
    if isinstance(head, tuple):
        head = head[0] if "terrain_nowater" in classes else head[1]
    return head


def _write_report(stats, classes, gsd, residual_threshold, logger_stats):
    """The report of lib/evaluation.py:361-449 on `logger_stats` from stats.before / stats.after."""
    area_size = float(stats.before.all["count_total"] * gsd * gsd) / 1000000
    logger_stats.info("\n\nPerformance Evaluation\n----------------------\n")
    logger_stats.info("Number of pixels:\t\t\t{}".format(int(stats.before.all["count_total"])))
    logger_stats.info("Area [km^2]:\t\t\t\t{:.2f}\n".format(area_size))
    if residual_threshold:
        logger_stats.info("Truncation threshold:\t\t\t{:.2f} m\n".format(residual_threshold))
    for c in classes:
        head = _heading(c, classes)
        for when, dsm in (("before", "INITIAL"), ("after", "REFINED")):
            title = "STATISTICS, {}: {} DSM".format(head, dsm)
            rule = len(title) + (c == "all" and when == "before")     # the reference's first rule is one dash longer
            logger_stats.info("\n{}\n{}\n".format(title, "-" * rule))
            print_statistics(stats[when][c], logger_stats)


def evaluate_performance(raster_prediction, ds_raster_input, ds_raster_gt, logger_root, area_defn=None,
                         path_gt_mask=None, path_building_mask=None, path_water_mask=None, path_forest_mask=None,
                         logger_stats=None, residual_threshold=None, *, nodata=None, gsd=None, device="cuda",
                         abs_quantiles=None, quantiles=None, within=None):
    """Drop-in for lib/evaluation.py:163 evaluate_performance: the same report on `logger_stats` and the same return
    value, the attribute dict `residuals.after` of host np.ma.MaskedArrays (class -> residuals of the refined DSM).

    The DSMs are arrays / tensors or dataset-like objects (GetRasterBand(1).ReadAsArray(), GetNoDataValue(),
    GetGeoTransform()); for arrays the ground truth's nodata value and the GSD come from `nodata=` / `gsd=`.  Mask
    arguments: arrays (value 1 = set), (values, nodata) tuples, dataset-like objects or paths (paths need osgeo.gdal; a
    path that does not exist is logged and skipped; a missing ground-truth mask means all ground-truth pixels).
    abs_quantiles / quantiles / within (see evaluate_statistics) add their lines to every block of the report."""
    if logger_stats is None:
        logger_stats = _default_stats_logger()
    pred, _ = _raster_arg(raster_prediction, "refined DSM", logger_root)
    gt, init, nodata, gsd, mask_gt, mask_b, mask_w, mask_f = _performance_inputs(
        ds_raster_input, ds_raster_gt, logger_root, path_gt_mask, path_building_mask, path_water_mask, path_forest_mask,
        nodata, gsd, "evaluate_performance")

    dev = _device(device)
    logger_root.info("\tCompute residual errors and statistics before and after the refinement...")
    stats, r_after, cls, classes = _evaluate(pred, init, gt, area_defn, mask_gt, mask_b, mask_w, mask_f,
                                             residual_threshold, nodata, dev,
                                             _dist_options(abs_quantiles, quantiles, within))
    _write_report(stats, classes, gsd, residual_threshold, logger_stats)

    data = r_after.cpu().numpy()
    bits = cls.cpu().numpy()
    valid = (bits & VALID_AFTER) != 0
    residuals = AttrDict()
    for c in classes:
        ok = valid if c == "all" else valid & ((bits & CLASS_BITS[c]) != 0)
        residuals[c] = np.ma.MaskedArray(data, mask=~ok, copy=False)
    return residuals


def get_statistics_masked(residuals_masked, residual_threshold=None, device="cuda", *, abs_quantiles=None, quantiles=None,
                          within=None):
    """The reference's get_statistics(residuals_masked, residual_threshold) (lib/evaluation.py:50): statistics of the
    unmasked values of an np.ma array (or of every value of an ndarray / tensor), any shape -- e.g. residuals pooled
    over several image pairs as in test.py.  -> the reference's statistics dict (attribute access); abs_quantiles / quantiles /
    within as in evaluate_statistics."""
    dist = _dist_options(abs_quantiles, quantiles, within)
    if torch.is_tensor(residuals_masked):
        dev = _device(residuals_masked.device if residuals_masked.is_cuda else device)
        r = residuals_masked.to(dev, torch.float64).reshape(-1).contiguous()
        valid = torch.ones(r.shape, dtype=torch.uint8, device=dev)
    else:
        dev = _device(device)
        a = np.ma.asarray(residuals_masked)
        r = _on(np.ma.getdata(a).astype(np.float64, copy=False).reshape(-1), dev)
        valid = _on((~np.ma.getmaskarray(a)).reshape(-1).astype(np.uint8), dev)
    if r.numel() == 0:                                 # nothing to read: the statistics of an empty set
        r = torch.zeros(1, dtype=torch.float64, device=dev)
        valid = torch.zeros(1, dtype=torch.uint8, device=dev)
    sets = [(0, 1, t) for t in _variants(residual_threshold)]
    rows = _Rows(len(sets), dist, dev)
    rows.sets(r, None, valid, sets)
    return _stats_dict(*_full_and_truncated(rows.host(), 0, residual_threshold), residual_threshold, dist)


# ---- every pair plane of a sweep, and the pool of all pairs (test.py:191-357) ----------------------------------------------
VALID_EXTRA = 64                                      # RD_CLS_VALID_EXTRA (include/resdepth_hip_eval.h)
MAX_PLANES = 16                                       # RD_EVAL_MAX_PLANES


def _is_sweep(x):
    return hasattr(x, "image_pairs") and hasattr(x, "pairs") and hasattr(x, "fused")


def _private_f64(x, dev):
    """-> (contiguous fp64 tensor on dev, whether it is a buffer of this call that may be overwritten)."""
    t = _on(x, dev, torch.float64)
    return t, not (torch.is_tensor(x) and t.data_ptr() == x.data_ptr())


def _evaluate_pairs(pairs, initial, gt, area_defn, mask_gt, mask_building, mask_water, mask_forest, residual_threshold,
                    fused, nodata, device, dist=None):
    """-> (stats {'before', 'pairs', 'pooled'[, 'fused']}, classes)"""
    if _is_sweep(pairs):
        sweep, pairs = pairs, getattr(pairs, "device_pairs", None)
        if pairs is None:
            pairs = sweep.pairs
        if pairs is None:
            raise ValueError("evaluate_pairs: the PairSweep holds no planes (predict_pairs_linear_blend(..., "
                             "return_pairs=False) without keep_device=True)")
        if fused is None:
            fused = getattr(sweep, "device_fused", None)
            fused = sweep.fused if fused is None else fused
    dev = _first_device(pairs, fused, initial, gt, default=device)
    if len(pairs.shape) != 3:
        raise ValueError(f"evaluate_pairs: pairs must be [P, rows, cols] (got shape {tuple(pairs.shape)})")
    n_planes = int(pairs.shape[0])
    if not 1 <= n_planes <= MAX_PLANES:
        raise ValueError(f"evaluate_pairs: {n_planes} planes (1..{MAX_PLANES})")
    init, g = _float_raster(initial, dev), _float_raster(gt, dev)
    if tuple(pairs.shape[1:]) != tuple(init.shape) or init.dim() != 2 or init.shape != g.shape:
        raise ValueError(f"evaluate: pair planes {tuple(pairs.shape[1:])}, initial {tuple(init.shape)} and ground truth "
                         f"{tuple(g.shape)} must be equal 2-D rasters")
    if fused is not None and tuple(fused.shape) != tuple(init.shape):
        raise ValueError(f"evaluate: fused surface {tuple(fused.shape)} != raster shape {tuple(init.shape)}")
    rows, cols = init.shape
    classes, masks, grid = _eval_inputs(rows, cols, area_defn, mask_gt, mask_building, mask_water, mask_forest, nodata, dev)
    # host planes are uploaded once into a buffer of this call and turned into residuals in place; a device tensor of the
    # caller is read where it is and the residuals go to a buffer of their own
    planes, own = _private_f64(pairs, dev)
    res = planes if own else torch.empty_like(planes)
    fz = r_fused = None
    if fused is not None:
        fz, own = _private_f64(fused, dev)
        r_fused = fz if own else torch.empty_like(fz)
    r_before = torch.empty((rows, cols), dtype=torch.float64, device=dev)
    cls = torch.empty((rows, cols), dtype=torch.uint8, device=dev)
    valid = torch.empty((rows, cols), dtype=torch.int16, device=dev)
    thr = residual_threshold
    with torch.cuda.device(dev):
        check(load().rd_eval_classify_planes(ptr(planes), rows * cols, n_planes, ptr(fz), ptr(init),
                                             int(init.dtype == torch.float64), ptr(g), int(g.dtype == torch.float64),
                                             *map(ptr, masks), *grid, ptr(r_before), ptr(res), ptr(r_fused), ptr(cls),
                                             ptr(valid), stream_ptr()), "eval_classify_planes")
    psets = [(CLASS_BITS[c], t) for c in classes for t in _variants(thr)]
    # the initial DSM and the fused surface: two sources of the sets kernel, off the same class byte
    sets = [(0, VALID_BEFORE | b, t) for b, t in psets]
    if fz is not None:
        sets += [(1, VALID_EXTRA | b, t) for b, t in psets]
    out = _Rows((n_planes + 1) * len(psets) + len(sets), dist, dev)      # one buffer for all of them: one read-back
    for p in range(n_planes + 1):                      # the pairs, then the pool of all of them
        p0, p1 = (p, p + 1) if p < n_planes else (0, n_planes)
        out.pooled(res, n_planes, p0, p1, cls, valid, psets)
    out.sets(r_before, r_fused, cls, sets)
    host = out.host()
    blocks = [_class_stats(host[k:k + len(psets)], classes, thr, dist) for k in range(0, len(host), len(psets))]
    stats = AttrDict(before=blocks[n_planes + 1], pairs=blocks[:n_planes], pooled=blocks[n_planes])
    if fz is not None:
        stats.fused = blocks[n_planes + 2]
    return stats, classes


def evaluate_pairs_statistics(pairs, initial, gt, area_defn=None, mask_gt=None, mask_building=None, mask_water=None,
                              mask_forest=None, residual_threshold=None, *, fused=None, nodata=None, device="cuda",
                              abs_quantiles=None, quantiles=None, within=None):
    """The statistics of test.py:191-357 for the P predictions of a pair sweep, scored where the sweep left them: ONE
    dilation and ONE classification pass whatever P is (rd_eval_classify_planes), then every pair's statistics sets and the
    sets of the pool of all pairs' residuals (rd_residual_stats_pooled), and the initial DSM and the fused surface from the
    same class byte (rd_residual_stats_sets).

    pairs: [P, rows, cols] array / tensor (1 <= P <= 16), or the PairSweep of predict_pairs_linear_blend -- its device planes
    are used when it carries them (keep_device=True), and its fused surface when `fused` is not given.  Device tensors are
    scored in place of residence and never written; host arrays are uploaded once.  Everything else as evaluate_statistics.
    -> {'before': {class: stats}, 'pairs': [P x {class: stats}], 'pooled': {class: stats}[, 'fused': {class: stats}]}, every
    stats dict in the reference's get_statistics format (attribute access).  abs_quantiles / quantiles / within as in
    evaluate_statistics: per pair and for the pool from rd_residual_dist_pooled (a quantile of the pool ranks the residuals of
    all pairs together), for the initial DSM and the fused surface from rd_residual_dist_sets."""
    return _evaluate_pairs(pairs, initial, gt, area_defn, mask_gt, mask_building, mask_water, mask_forest,
                           residual_threshold, fused, nodata, device, _dist_options(abs_quantiles, quantiles, within))[0]


def evaluate_pairs_performance(pairs, ds_raster_input, ds_raster_gt, logger_root, area_defn=None, path_gt_mask=None,
                               path_building_mask=None, path_water_mask=None, path_forest_mask=None, loggers_stats=None,
                               logger_stats_pooled=None, residual_threshold=None, *, fused=None, nodata=None, gsd=None,
                               device="cuda", abs_quantiles=None, quantiles=None, within=None):
    """Drop-in for the evaluation of test.py:191-357: on loggers_stats[p] the report evaluate_performance writes for
    prediction p, and on logger_stats_pooled the "statistics over all predictions" block (test.py:326-357; written when
    there is more than one pair, as in the reference, or when the logger is given).  pairs / fused as
    evaluate_pairs_statistics, every other argument as evaluate_performance.  -> the statistics object of
    evaluate_pairs_statistics; the residual rasters are not returned (evaluate_performance per plane gives them).
    abs_quantiles / quantiles / within (see evaluate_statistics) add their lines to every block of every report."""
    gt, init, nodata, gsd, mask_gt, mask_b, mask_w, mask_f = _performance_inputs(
        ds_raster_input, ds_raster_gt, logger_root, path_gt_mask, path_building_mask, path_water_mask, path_forest_mask,
        nodata, gsd, "evaluate_pairs_performance")
    logger_root.info("\tCompute residual errors and statistics before and after the refinement...")
    stats, classes = _evaluate_pairs(pairs, init, gt, area_defn, mask_gt, mask_b, mask_w, mask_f, residual_threshold,
                                     fused, nodata, device, _dist_options(abs_quantiles, quantiles, within))
    n_planes = len(stats.pairs)
    if loggers_stats is None:
        loggers_stats = [_default_stats_logger()] * n_planes
    if len(loggers_stats) != n_planes:
        raise ValueError(f"evaluate_pairs_performance: {len(loggers_stats)} loggers for {n_planes} pairs")
    for p, logger_stats in enumerate(loggers_stats):
        _write_report(AttrDict(before=stats.before, after=stats.pairs[p]), classes, gsd, residual_threshold, logger_stats)
    if logger_stats_pooled is None and n_planes > 1:
        logger_stats_pooled = _default_stats_logger("stats_logger_overall")
    if logger_stats_pooled is not None:
        logger_root.info("\nCompute residual errors averaged over all predictions...")
        title = "Performance Evaluation: Statistics over all predictions"
        logger_stats_pooled.info("\n{}\n{}\n".format(title, "-" * len(title)))
        if residual_threshold:
            logger_stats_pooled.info("Truncation threshold:\t\t\t{:.2f} m\n".format(residual_threshold))
        for c in classes:
            title = "STATISTICS, {}: REFINED DSM".format(_heading(c, classes))
            logger_stats_pooled.info("\n{}\n{}\n".format(title, "-" * len(title)))
            print_statistics(stats.pooled[c], logger_stats_pooled)
    return stats


# ---- where the error is and on what ground: cell grids, slope, covariate bins (include/resdepth_hip_errmap.h) -----------------
CELL_MIN, CELL_MAX, BIN_MAX = 4, 256, 24              # RD_CELL_MIN, RD_CELL_MAX, RD_BIN_MAX
MAX_CELLS = 1 << 24                                   # RD_CELL_MAX_CELLS
BINS_PER_PLANE = 6                                    # bin bits of one class-byte plane of rd_bin_classes (bits 2..7)


def _pair_of(v, what, cast):
    """scalar or (first, second) -> (first, second)"""
    if isinstance(v, (tuple, list)) or (hasattr(v, "shape") and len(getattr(v, "shape")) == 1):
        if len(v) != 2:
            raise ValueError(f"{what}: expected a scalar or a pair, got {v!r}")
        return cast(v[0]), cast(v[1])
    return cast(v), cast(v)


def _slope_tangent(d, gsd, nodata, who):
    """device f32 / f64 raster -> device fp64 raster of rd_dsm_slope (rise over run); the arguments checked on the host"""
    if gsd is None:
        raise ValueError(f"{who}: the slope needs gsd= (a scalar or (gsd_y, gsd_x))")
    gsd_y, gsd_x = _pair_of(gsd, f"{who}: gsd", float)
    if not (0.0 < gsd_x < float("inf") and 0.0 < gsd_y < float("inf")):
        raise ValueError(f"{who}: gsd {gsd!r} must be positive and finite")
    if d.dim() != 2 or d.numel() == 0:
        raise ValueError(f"{who}: expected a non-empty 2-D raster, got shape {tuple(d.shape)}")
    rows, cols = d.shape
    out = torch.empty((rows, cols), dtype=torch.float64, device=d.device)
    nd = float("nan") if nodata is None else float(nodata)
    with torch.cuda.device(d.device):
        check(load().rd_dsm_slope(ptr(d), int(d.dtype == torch.float64), rows, cols, nd, gsd_x, gsd_y, ptr(out), stream_ptr()),
              "dsm_slope")
    return out


def dsm_slope(dsm, gsd, nodata=-9999, degrees=True, device="cuda"):
    """Horn's 3 x 3 slope of a DSM (rd_dsm_slope, include/resdepth_hip_errmap.h) -> device fp64 raster: the slope angle in
    degrees, or with degrees=False its tangent (rise over run) exactly as the kernel leaves it.  dsm: 2-D array / tensor, f32 and
    f64 read as given; gsd: a scalar or (gsd_y, gsd_x).  NaN where any pixel of the 3 x 3 neighbourhood is nodata, NaN or outside
    the raster (so on the border ring)."""
    dev = _first_device(dsm, default=device)
    slope = _slope_tangent(_float_raster(dsm, dev), gsd, nodata, "dsm_slope")
    return torch.rad2deg(torch.atan(slope)) if degrees else slope


def _threshold(thr, who):
    """residual_threshold -> the thr of the C ABI (0: none)"""
    if not thr:
        return 0.0
    thr = float(thr)
    if not 0.0 < thr < float("inf"):
        raise ValueError(f"{who}: residual_threshold {thr} must be positive and finite")
    return thr


def error_map(prediction, gt, cell, *, initial=None, area_defn=None, mask_gt=None, mask_building=None, mask_water=None,
              mask_forest=None, nodata=-9999, residual_threshold=None, klass=None, device="cuda"):
    """The accuracy map of a refined DSM: the eight statistics of evaluate_statistics for every cell of a grid of cell x cell
    pixels (cell: an int or (cell_h, cell_w), 4..256; the ragged border cells included), by one rd_cell_stats launch on the
    residuals and class bytes of the classification pass evaluate_statistics runs (same masks, same area, same nodata rule).

    klass: one of the report's classes ("building", "terrain", "terrain_nowater", "terrain_nowater_noforest"; the masks that
    define it must be given), None or "all": every valid pixel.  residual_threshold: only |residual| <= threshold counts.
    -> AttrDict: refined [ncy, ncx, 8] (device fp64; an empty cell holds count 0 and NaN), initial (the same for the initial DSM,
    when given), keys (the eight names in order), cell (cell_h, cell_w) and origin (0, 0): cell (cy, cx) covers rows
    cy * cell_h .. and columns cx * cell_w .. of the raster."""
    cell_h, cell_w = _pair_of(cell, "error_map: cell", int)
    if not (CELL_MIN <= cell_h <= CELL_MAX and CELL_MIN <= cell_w <= CELL_MAX):
        raise ValueError(f"error_map: cell {cell_h} x {cell_w}, sides must be in {CELL_MIN}..{CELL_MAX}")
    thr = _threshold(residual_threshold, "error_map")
    dev = _first_device(prediction, initial, gt, default=device)
    r_before, r_after, cls, classes = _classified(prediction, initial, gt, area_defn, mask_gt, mask_building, mask_water,
                                                  mask_forest, nodata, dev, "error_map")
    klass = "all" if klass is None else klass
    if klass not in classes:
        raise ValueError(f"error_map: class {klass!r} is not defined by the masks given (have {classes})")
    rows, cols = cls.shape
    ncy, ncx = -(-rows // cell_h), -(-cols // cell_w)
    if ncy * ncx >= MAX_CELLS:
        raise ValueError(f"error_map: {ncy} x {ncx} cells, a call takes fewer than {MAX_CELLS}")
    res = AttrDict(keys=list(_KEYS), cell=(cell_h, cell_w), origin=(0, 0))
    lib = load()
    with torch.cuda.device(dev):
        for name, r, valid in (("refined", r_after, VALID_AFTER),) + ((("initial", r_before, VALID_BEFORE),)
                                                                      if initial is not None else ()):
            out = torch.empty((ncy, ncx, 8), dtype=torch.float64, device=dev)
            check(lib.rd_cell_stats(ptr(r), ptr(cls), rows, cols, cell_h, cell_w, valid | CLASS_BITS[klass], thr, ptr(out),
                                    stream_ptr()), "cell_stats")
            res[name] = out
    return res


def _bin_edges(edges, who):
    e = [float(v) for v in edges]
    if not 1 <= len(e) - 1 <= BIN_MAX:
        raise ValueError(f"{who}: {len(e)} edges, expected 2..{BIN_MAX + 1} ({BIN_MAX} bins at most)")
    if any(v != v for v in e) or any(not a < b for a, b in zip(e, e[1:])):
        raise ValueError(f"{who}: edges must increase strictly and hold no NaN (got {e})")
    return e


def _degrees_to_tangent(e):
    """an edge in degrees -> the tangent the slope raster stores, in fp64 on the host (the infinities stay)"""
    import math
    return e if math.isinf(e) else math.tan(math.radians(e))


def evaluate_binned(prediction, initial, gt, by, edges, *, gsd=None, area_defn=None, mask_gt=None, nodata=-9999,
                    residual_threshold=None, device="cuda"):
    """The statistics of evaluate_statistics (class "all") as a function of a covariate: one statistics dict for the initial and
    one for the refined DSM per bin [edges[b], edges[b + 1]) of `by` (at most 24 bins, -inf / +inf allowed at the ends; a pixel
    whose covariate is NaN or outside the edges is in no bin).

    by: a raster of the DSMs' shape (array / tensor, f32 / f64 read as given), or "slope": Horn's slope of `gt` (rd_dsm_slope;
    needs gsd= as a scalar or (gsd_y, gsd_x)) with the edges in DEGREES -- they are converted on the host, tan(radians(e)) in
    fp64, and the pixels are binned on the stored tangent raster, so by="slope" and by=dsm_slope(gt, gsd, nodata,
    degrees=False) with those converted edges give the same bits.
    rd_bin_classes writes the bins as class bytes, six bins to a plane, in one pass; every bin is then an ordinary set (validity
    bit | bin bit) of rd_residual_stats_sets, up to 20 sets per call, all enqueued before the one read-back.
    -> [AttrDict(lo, hi, initial, refined)] per bin, lo / hi the edges as given, initial / refined in the get_statistics format
    (with the truncated sub-dict when residual_threshold is given)."""
    who = "evaluate_binned"
    e = _bin_edges(edges, who)
    n_bins = len(e) - 1
    thr = _threshold(residual_threshold, who) or None
    slope = isinstance(by, str)
    if slope and by != "slope":
        raise ValueError(f"{who}: by={by!r}: expected a raster or \"slope\"")
    if slope and gsd is None:
        raise ValueError(f"{who}: by=\"slope\" needs gsd=")
    if slope:
        _pair_of(gsd, f"{who}: gsd", float)
        cut = [_degrees_to_tangent(v) for v in e]
        if any(not a < b for a, b in zip(cut, cut[1:])):
            raise ValueError(f"{who}: the slope edges {e} do not increase as tangents (degrees within (-90, 90))")
    else:
        cut = e
        if tuple(by.shape) != tuple(gt.shape):
            raise ValueError(f"{who}: covariate shape {tuple(by.shape)} != raster shape {tuple(gt.shape)}")
    dev = _first_device(prediction, initial, gt, default=device)
    r_before, r_after, cls, _ = _classified(prediction, initial, gt, area_defn, mask_gt, None, None, None, nodata, dev, who)
    cov = _slope_tangent(_float_raster(gt, dev), gsd, nodata, who) if slope else _float_raster(by, dev)
    n = cls.numel()
    groups = -(-n_bins // BINS_PER_PLANE)
    planes = torch.empty((groups, n), dtype=torch.uint8, device=dev)
    lib = load()
    edge_a = (ctypes.c_double * (n_bins + 1))(*cut)
    with torch.cuda.device(dev):
        check(lib.rd_bin_classes(ptr(cov), int(cov.dtype == torch.float64), ptr(cls), n, edge_a, n_bins, ptr(planes),
                                 stream_ptr()), "bin_classes")
    # the sets of a bin: initial, refined (each with its truncated set), so two _variants steps of rows per bin
    sides = ((0, VALID_BEFORE), (1, VALID_AFTER))
    rows = _Rows(n_bins * len(sides) * len(_variants(thr)), None, dev)
    for g in range(groups):
        bins = range(g * BINS_PER_PLANE, min(n_bins, (g + 1) * BINS_PER_PLANE))
        rows.sets(r_before, r_after, planes[g], [(src, valid | (4 << (b - g * BINS_PER_PLANE)), t) for b in bins
                                                 for src, valid in sides for t in _variants(thr)])
    host = rows.host()
    return [AttrDict(lo=e[b], hi=e[b + 1], initial=_stats_dict(*_full_and_truncated(host, 2 * b, thr), thr),
                     refined=_stats_dict(*_full_and_truncated(host, 2 * b + 1, thr), thr)) for b in range(n_bins)]


def print_binned(stats, logger, unit=""):
    """One table for the list evaluate_binned returns, in the number format of print_statistics: per bin its interval, the pixel
    count of the refined DSM and MAE, RMSE, median and NMAD of the initial -> the refined DSM [m]."""
    logger.info("{:>21s}\t{:>10s}\t{:>23s}\t{:>23s}\t{:>23s}\t{:>23s}".format(
        "Bin" + (" [{}]".format(unit) if unit else ""), "Pixels", "MAE [m]", "RMSE [m]", "Median [m]", "NMAD [m]"))
    for k, b in enumerate(stats):
        cols = "\t".join("{:10.3f} ->{:10.3f}".format(b.initial[key], b.refined[key]) for key in ("MAE", "RMSE", "median", "NMAD"))
        logger.info("[{:9.3f},{:9.3f})\t{:10d}\t{}{}".format(b.lo, b.hi, int(b.refined["count_total"]), cols,
                                                            "\n" if k == len(stats) - 1 else ""))
