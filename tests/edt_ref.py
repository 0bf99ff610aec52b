"""numpy oracles of include/resdepth_hip_edt.h (test infrastructure only).  Both restate the header, neither the kernels:

  brute(mask)      ranks ALL set pixels by (d2, |dx|, column, row) for every pixel: O(pixels x set pixels), for rasters of a few
                   thousand pixels or masks with a handful of set pixels
  separable(mask)  exact and separable, for larger rasters: per column the nearest set row (the smaller row on a tie, which is
                   the header's last criterion), then per row min over c of (x - c)^2 + g[c]^2 by broadcasting, ranked by
                   (d2, |dx|, column)

-> (d2, idx) int32 arrays of the mask's shape: RD_EDT_NONE and -1 where the mask has no set pixel."""
import math

import numpy as np

NONE = 2147483647
MAX_ROWS, MAX_COLS, BAND_ROWS = 32768, 16384, 128


def is_set(mask, invert=False):
    m = np.asarray(mask) != 0
    return ~m if invert else m


def brute(mask, invert=False):
    s = is_set(mask, invert)
    rows, cols = s.shape
    assert (rows ** 2 + cols ** 2) * cols * cols * rows < 2 ** 63, "the ranking key of brute() needs a smaller raster"
    d2 = np.full((rows, cols), NONE, np.int32)
    idx = np.full((rows, cols), -1, np.int32)
    ys, xs = (a.astype(np.int64) for a in np.nonzero(s))
    if ys.size == 0:
        return d2, idx
    py, px = (a.reshape(-1).astype(np.int64) for a in np.mgrid[0:rows, 0:cols])
    step = max(1, (1 << 22) // ys.size)
    for a in range(0, py.size, step):
        y, x = py[a:a + step, None], px[a:a + step, None]
        dx = np.abs(xs[None, :] - x)
        dist = (ys[None, :] - y) ** 2 + dx ** 2
        key = ((dist * cols + dx) * cols + xs[None, :]) * rows + ys[None, :]      # (d2, |dx|, column, row) in one int64
        k = np.argmin(key, axis=1)
        d2.reshape(-1)[a:a + step] = dist[np.arange(k.size), k]
        idx.reshape(-1)[a:a + step] = ys[k] * cols + xs[k]
    return d2, idx


def column_offsets(s):
    """-> int64 [rows, cols]: the signed row offset to the nearest set pixel of the column, the upper one on a tie; NONE: none"""
    rows, cols = s.shape
    r = np.arange(rows, dtype=np.int64)[:, None]
    up = np.maximum.accumulate(np.where(s, r, -1), axis=0)                        # the last set row <= r
    down = np.minimum.accumulate(np.where(s, r, 1 << 40)[::-1], axis=0)[::-1]     # the first set row >= r
    du = np.where(up >= 0, r - up, 1 << 40)
    dd = np.where(down < (1 << 40), down - r, 1 << 40)
    off = np.where(du <= dd, -du, dd)
    return np.where((du == 1 << 40) & (dd == 1 << 40), NONE, off)


def separable(mask, invert=False):
    s = is_set(mask, invert)
    rows, cols = s.shape
    d2 = np.full((rows, cols), NONE, np.int32)
    idx = np.full((rows, cols), -1, np.int32)
    if not s.any():
        return d2, idx
    g = column_offsets(s)
    c = np.arange(cols, dtype=np.int64)
    dx = np.abs(c[:, None] - c[None, :])                                          # [x, c]
    dx2 = dx * dx
    for r in range(rows):
        have = g[r] != NONE
        cost = np.where(have[None, :], dx2 + np.where(have, g[r], 0)[None, :] ** 2, 1 << 40)
        k = np.argmin((cost * cols + dx) * cols + c[None, :], axis=1)             # (d2, |dx|, column)
        d2[r] = cost[c, k]
        idx[r] = (r + g[r, k]) * cols + k
    return d2, idx


def one_pixel(rows, cols, y, x):
    """the transform of a mask whose only set pixel is (y, x)"""
    r, c = np.mgrid[0:rows, 0:cols].astype(np.int64)
    return ((r - y) ** 2 + (c - x) ** 2).astype(np.int32), np.full((rows, cols), y * cols + x, np.int32)


def attains(mask, d2, idx, invert=False):
    """the index names a set pixel at exactly the distance claimed (or -1 beside NONE)"""
    s = is_set(mask, invert)
    rows, cols = s.shape
    if not s.any():
        return bool((d2 == NONE).all() and (idx == -1).all())
    y, x = np.divmod(idx.astype(np.int64), cols)
    r, c = np.mgrid[0:rows, 0:cols]
    return bool((idx >= 0).all() and s[y, x].all() and ((y - r) ** 2 + (x - c) ** 2 == d2).all())


def threshold(distance, gsd):
    """t = floor((distance / gsd)^2 + 1e-9), at most NONE - 1: the formula of resdepth_amd.morphology.squared_threshold"""
    q = (float(distance) / float(gsd)) ** 2 + 1e-9
    return NONE - 1 if q >= NONE - 1 else int(math.floor(q))


def fill_nearest(dsm, d2, idx, max_d2):
    """out[i] = (d2[i] > 0 && d2[i] <= max_d2 && 0 <= idx[i] < n) ? dsm[idx[i]] : dsm[i], as bit patterns"""
    flat = np.ascontiguousarray(dsm).reshape(-1)
    bits = flat.view(np.uint32 if flat.dtype == np.float32 else np.uint64)
    d, j = np.asarray(d2).reshape(-1), np.asarray(idx).reshape(-1).astype(np.int64)
    take = (d > 0) & (d <= max_d2) & (j >= 0) & (j < flat.size)
    out = np.where(take, bits[np.where(take, j, 0)], bits)
    return out.view(flat.dtype).reshape(np.shape(dsm))


def fill_voids(dsm, nodata, max_distance=None, gsd=1.0):
    """-> (filled, the voids that were filled), by the brute-force oracle"""
    z = np.asarray(dsm)
    void = np.isnan(z) | (z == nodata)
    d2, idx = brute(void, invert=True)
    cap = NONE - 1 if max_distance is None else threshold(max_distance, gsd)
    return fill_nearest(z, d2, idx, cap), void & (d2 <= cap)


def cross_dilation(mask, iterations):
    """scipy.ndimage.binary_dilation(mask, iterations=k) with the default cross, outside unset: the L1 ball of radius k"""
    m = np.asarray(mask) != 0
    for _ in range(iterations):
        n = m.copy()
        n[1:] |= m[:-1]
        n[:-1] |= m[1:]
        n[:, 1:] |= m[:, :-1]
        n[:, :-1] |= m[:, 1:]
        m = n
    return m


def random_mask(rows, cols, density, seed):
    return (np.random.default_rng(seed).random((rows, cols)) < density).astype(np.uint8)
