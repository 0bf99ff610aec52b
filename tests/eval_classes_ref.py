"""numpy restatement of the class-partitioned evaluation (TEST INFRASTRUCTURE ONLY): the class semantics of
lib/evaluation.py:163-457 evaluate_performance on top of oracle.stats_oracle, with a pure-numpy L1-ball dilation (scipy
may be absent where the GPU tests run).  Pinned by tests/golden/g18_eval.npz (produced by the reference function)."""
import numpy as np

from oracle import stats_oracle as E

CLASSES = ["all", "building", "terrain", "terrain_nowater", "terrain_nowater_noforest"]
KEYS = ["count_total", "diff_max", "diff_min", "MAE", "RMSE", "absolute_median", "median", "NMAD"]
TKEYS = ["count_total", "MAE", "RMSE", "absolute_median", "median", "NMAD"]


def dilate(mask, k):
    """scipy.ndimage.binary_dilation(mask, iterations=k): OR over the L1 ball of radius k, outside pixels unset."""
    m = np.asarray(mask) != 0
    h, w = m.shape
    p = np.zeros((h + 2 * k, w + 2 * k), bool)
    p[k:k + h, k:k + w] = m
    out = np.zeros_like(m)
    for dy in range(-k, k + 1):
        r = k - abs(dy)
        for dx in range(-r, r + 1):
            out |= p[k + dy:k + dy + h, k + dx:k + dx + w]
    return out


def mask_of(values, nodata=None):
    """load_mask_raster: (set, nodata) = (value == 1 and not nodata, value == nodata)."""
    v = np.asarray(values)
    nd = np.zeros(v.shape, bool) if nodata is None else (v == nodata)
    return (v == 1) & ~nd, nd


def area_mask(area, shape):
    """area rows [x0, x1, y0, y1] (inclusive) -> bool raster; None -> everything."""
    if area is None:
        return np.ones(shape, bool)
    a = np.zeros(shape, bool)
    for x0, x1, y0, y1 in area:
        a[y0:y1 + 1, x0:x1 + 1] = True
    return a


def classify(pred, init, gt, nodata, area=None, gt_mask=None, building=None, water=None, forest=None):
    """-> (r_before, r_after, {class: (valid_before, valid_after)}) with f64 residuals.  Masks are (values, nodata)."""
    a = area_mask(area, gt.shape)
    g = gt.astype(np.float64)
    ok = a & (g != nodata)
    if gt_mask is not None:
        ok &= mask_of(*gt_mask)[0]
    vb, va = ok & (init.astype(np.float64) != nodata), ok & (pred.astype(np.float64) != nodata)
    cls = {"all": np.ones(gt.shape, bool)}
    if building is not None:
        b, bnd = mask_of(*building)
        bd = dilate(b, 2)
        cls["building"] = bd & a
        t = ~bd & ~bnd & a
        cls["terrain"] = t
        tw = t
        if water is not None:
            tw = t & ~mask_of(*water)[0]
            cls["terrain_nowater"] = tw
        if forest is not None:
            cls["terrain_nowater_noforest"] = tw & ~mask_of(*forest)[0]
    rb = init.astype(np.float64) - g
    ra = pred.astype(np.float64) - g
    return rb, ra, {c: (vb & m, va & m) for c, m in cls.items()}


def stats_row(r, valid, thr=None):
    """one recorded get_statistics call: 8 statistics + 6 truncated ones (NaN without a threshold)."""
    st = E.statistics(r.ravel(), valid.ravel())
    row = [st[k] for k in KEYS]
    if thr:
        tt = E.statistics(r.ravel(), valid.ravel(), thr)
        row += [tt[k] for k in TKEYS]
    else:
        row += [np.nan] * len(TKEYS)
    return row


def evaluate_calls(rb, ra, classes, thr=None):
    """the statistics in the reference's call order: per class, before then after."""
    rows = []
    for c in CLASSES:
        if c in classes:
            vb, va = classes[c]
            rows += [stats_row(rb, vb, thr), stats_row(ra, va, thr)]
    return np.array(rows)


def golden_case(g, i):
    """the inputs of g18 case i as restatement arguments."""
    p = f"c{i}/"
    masks = {k: ((g[p + "mask_" + k], 255.0) if p + "mask_" + k in g else None) for k in "gbwf"}
    thr = float(g[p + "thr"])
    return dict(pred=g[p + "pred"], init=g[p + "init"], gt=g[p + "gt"], nodata=float(g["nodata"]),
                area=g.get(p + "area"), gt_mask=masks["g"], building=masks["b"],
                water=masks["w"] if masks["b"] is not None else None,
                forest=masks["f"] if masks["b"] is not None else None), (thr if thr > 0 else None)
