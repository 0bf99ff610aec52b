"""numpy restatements of include/resdepth_hip_errmap.h (TEST INFRASTRUCTURE ONLY): the statistics of every cell of a grid on top
of oracle.stats_oracle (pinned on the reference's get_statistics by tests/golden/g10_stats.npz), Horn's slope operation for
operation in fp64, and the bins of a covariate as class bytes."""
import numpy as np

from oracle import stats_oracle as E

KEYS = ["count_total", "diff_max", "diff_min", "MAE", "RMSE", "absolute_median", "median", "NMAD"]
EXACT = [0, 1, 2, 5, 6, 7]              # count, max, min and the three medians
SUMS = [3, 4]                           # MAE, RMSE


def members_mask(r, cls, need, thr):
    """the set definition of the engine: all bits of need, |r| <= thr when thr > 0 (a NaN then never is a member)"""
    ok = (cls.astype(np.int64) & need) == need
    if thr and thr > 0:
        with np.errstate(invalid="ignore"):
            ok &= np.abs(r) <= thr
    return ok


def stats_row(r, valid):
    """the eight numbers of the members r[valid] through the oracle; an empty set: count 0 and NaN elsewhere"""
    if not valid.any():
        return np.array([0.0] + [np.nan] * 7)
    st = E.statistics(r.ravel(), valid.ravel())
    return np.array([st[k] for k in KEYS])


def cell_stats(r, cls, cell_h, cell_w, need=0, thr=0.0):
    """-> [ncy, ncx, 8]: a loop over the cells (the ragged border cells included) of the oracle's statistics"""
    r, cls = np.asarray(r, np.float64), np.asarray(cls)
    rows, cols = r.shape
    ncy, ncx = -(-rows // cell_h), -(-cols // cell_w)
    ok = members_mask(r, cls, need, thr)
    out = np.empty((ncy, ncx, 8))
    for cy in range(ncy):
        for cx in range(ncx):
            win = (slice(cy * cell_h, min(rows, (cy + 1) * cell_h)), slice(cx * cell_w, min(cols, (cx + 1) * cell_w)))
            out[cy, cx] = stats_row(r[win], ok[win])
    return out


def slope(dsm, gsd_y, gsd_x, nodata=None):
    """Horn's slope as rise over run, every operation one fp64 operation of numpy (which never contracts); NaN where any of the
    nine pixels is nodata, NaN or outside the raster.  f32 rasters are widened, not rounded."""
    z = np.asarray(dsm).astype(np.float64)
    rows, cols = z.shape
    bad = np.isnan(z) if nodata is None else (np.isnan(z) | (z == nodata))
    out = np.full((rows, cols), np.nan)
    if rows < 3 or cols < 3:
        return out
    w = lambda dy, dx: z[1 + dy:rows - 1 + dy, 1 + dx:cols - 1 + dx]
    a, b, c = w(-1, -1), w(-1, 0), w(-1, 1)
    d, f = w(0, -1), w(0, 1)
    g, h, i = w(1, -1), w(1, 0), w(1, 1)
    two = np.float64(2.0)
    with np.errstate(invalid="ignore", over="ignore"):
        p = (((c + two * f) + i) - ((a + two * d) + g)) / (np.float64(8.0) * np.float64(gsd_x))
        q = (((g + two * h) + i) - ((a + two * b) + c)) / (np.float64(8.0) * np.float64(gsd_y))
        s = np.sqrt((p * p) + (q * q))
    any_bad = np.zeros((rows - 2, cols - 2), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            any_bad |= bad[1 + dy:rows - 1 + dy, 1 + dx:cols - 1 + dx]
    s[any_bad] = np.nan
    out[1:-1, 1:-1] = s
    return out


def bin_index(by, edges):
    """-> the bin of every value, -1 for none: searchsorted(edges, by, "right") - 1, in range"""
    e = np.asarray(edges, np.float64)
    b = np.searchsorted(e, np.asarray(by).astype(np.float64).ravel(), "right") - 1
    b[(b < 0) | (b >= len(e) - 1)] = -1
    return b


def bin_classes(by, cls, edges):
    """-> [G, n] uint8 planes: the two validity bits and the bin bit 1 << (2 + b - 6 g) in the plane g = b // 6 of the bin"""
    b = bin_index(by, edges)
    n_bins = len(edges) - 1
    base = np.asarray(cls).ravel().astype(np.uint8) & 3
    planes = np.repeat(base[None], -(-n_bins // 6), axis=0)
    idx = np.nonzero(b >= 0)[0]
    planes[b[idx] // 6, idx] |= (4 << (b[idx] % 6)).astype(np.uint8)
    return planes
