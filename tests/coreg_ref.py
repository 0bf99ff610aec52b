"""numpy fp64 restatement of include/resdepth_hip_coreg.h and of the iteration on top of it (TEST INFRASTRUCTURE ONLY), written from
the definitions and not from the kernels: Horn's gradient and the residual with every operation separately rounded (numpy's
element-wise operations are), the membership rule, the ten sums by math.fsum, the bilinear translate, the 3 x 3 solve and the
iteration.  Also the analytic test surface and its shifted copies."""
import math

import numpy as np

NAN_BITS = 0x7FF8000000000000
NSUMS = 10
COND_MAX = 1e12


def _canonical_nan():
    return np.array([NAN_BITS], dtype=np.uint64).view(np.float64)[0]


def terms(src, ref, cls, need, nodata, gsd_x, gsd_y, thr=0.0, slope_max=0.0):
    """-> (member [rows, cols] bool, the nine term rasters p, q, d, pp, pq, qq, pd, qd, dd as fp64 [rows, cols])"""
    s = np.asarray(src).astype(np.float64)
    g = np.asarray(ref).astype(np.float64)
    rows, cols = s.shape
    member = np.zeros((rows, cols), bool)
    zero = np.zeros((rows, cols))
    if rows < 3 or cols < 3:
        return member, [zero] * 9
    bad = np.isnan(s) | (s == nodata)                   # nodata NaN: the comparison is false everywhere
    a, b, c = s[:-2, :-2], s[:-2, 1:-1], s[:-2, 2:]
    d4, e, f = s[1:-1, :-2], s[1:-1, 1:-1], s[1:-1, 2:]
    g7, h, i = s[2:, :-2], s[2:, 1:-1], s[2:, 2:]
    with np.errstate(all="ignore"):
        east = (c + 2.0 * f) + i
        west = (a + 2.0 * d4) + g7
        south = (g7 + 2.0 * h) + i
        north = (a + 2.0 * b) + c
        p = (east - west) / (8.0 * gsd_x)
        q = (south - north) / (8.0 * gsd_y)
        d = g[1:-1, 1:-1] - e
        pp, qq = p * p, q * q
        near = np.zeros((rows - 2, cols - 2), bool)
        for dy in range(3):
            for dx in range(3):
                near |= bad[dy:dy + rows - 2, dx:dx + cols - 2]
        gi = g[1:-1, 1:-1]
        ok = ~near & ~np.isnan(gi) & (gi != nodata) & np.isfinite(p) & np.isfinite(q) & np.isfinite(d)
        if need:
            ok &= (np.asarray(cls)[1:-1, 1:-1].astype(np.int64) & need) == need
        if thr > 0:
            ok &= np.abs(d) <= thr
        if slope_max > 0:
            ok &= (pp + qq) <= slope_max * slope_max
        inner = [p, q, d, pp, p * q, qq, p * d, q * d, d * d]
    member[1:-1, 1:-1] = ok
    out = []
    for v in inner:
        full = np.zeros((rows, cols))
        full[1:-1, 1:-1] = v
        out.append(full)
    return member, out


def shift_sums(src, ref, cls, need, nodata, gsd_x, gsd_y, thr=0.0, slope_max=0.0):
    """-> (the ten sums, math.fsum over the members; the sums of |term| for the bound of any summation order)"""
    member, ts = terms(src, ref, cls, need, nodata, gsd_x, gsd_y, thr, slope_max)
    sums = [float(member.sum())] + [math.fsum(t[member].tolist()) for t in ts]
    mags = [float(member.sum())] + [math.fsum(np.abs(t[member]).tolist()) for t in ts]
    return np.array(sums), np.array(mags)


def translate(src, nodata, tx, ty, tz, fill):
    """rd_translate_bilinear: the content moved by (tx, ty) pixels and lifted by tz -> fp64 [rows, cols]"""
    s = np.asarray(src).astype(np.float64)
    rows, cols = s.shape
    nanv = _canonical_nan()
    fillv = nanv if fill != fill else float(fill)
    out = np.empty((rows, cols))
    out_bits = out.view(np.uint64)
    with np.errstate(all="ignore"):
        ys = np.arange(rows, dtype=np.float64) - ty
        xs = np.arange(cols, dtype=np.float64) - tx
        y0, x0 = np.floor(ys), np.floor(xs)
        fy, fx = ys - y0, xs - x0

        def tap(v):
            return bool(np.isnan(v) or v == nodata)
        for y in range(rows):
            two_y = fy[y] != 0.0
            for x in range(cols):
                two_x = fx[x] != 0.0
                if not (0.0 <= y0[y] <= rows - (2 if two_y else 1) and 0.0 <= x0[x] <= cols - (2 if two_x else 1)):
                    out[y, x] = fillv
                    continue
                iy, ix = int(y0[y]), int(x0[x])
                v00 = s[iy, ix]
                needed = [v00]
                top = v00
                if two_x:
                    v01 = s[iy, ix + 1]
                    needed.append(v01)
                    top = v00 + fx[x] * (v01 - v00)
                val = top
                if two_y:
                    v10 = s[iy + 1, ix]
                    needed.append(v10)
                    bot = v10
                    if two_x:
                        v11 = s[iy + 1, ix + 1]
                        needed.append(v11)
                        bot = v10 + fx[x] * (v11 - v10)
                    val = top + fy[y] * (bot - top)
                val = val + tz
                if any(tap(v) for v in needed):
                    out[y, x] = fillv
                elif np.isnan(val):
                    out_bits[y, x] = NAN_BITS
                else:
                    out[y, x] = val
    return out


def solve(sums):
    """the ten sums -> dict(tx, ty, tz, sigma0, cov) or a RuntimeError where they constrain nothing"""
    n, sp, sq, sd, spp, spq, sqq, spd, sqd, sdd = [float(v) for v in sums]
    if n < 3:
        raise RuntimeError("fewer than three member pixels")
    A = np.array([[spp, spq, sp], [spq, sqq, sq], [sp, sq, n]])
    rhs = np.array([spd, sqd, sd])
    with np.errstate(all="ignore"):
        cond = np.linalg.cond(A)
    if not cond <= COND_MAX:
        raise RuntimeError("the surface does not constrain the shift")
    a, b, c = np.linalg.solve(A, rhs)
    sol = np.array([a, b, c])
    rss = max(sdd - 2.0 * sol @ rhs + sol @ A @ sol, 0.0)
    sigma0 = math.sqrt(rss / (n - 3)) if n > 3 else float("nan")
    flip = np.diag([-1.0, -1.0, 1.0])
    return dict(tx=-a, ty=-b, tz=c, sigma0=sigma0, cov=sigma0 * sigma0 * (flip @ np.linalg.inv(A) @ flip), count=int(n))


def coregister(src, ref, gsd_x, gsd_y, nodata=-9999.0, cls=None, need=0, thr=0.0, slope_max=0.0, max_iter=10, tol=1e-3):
    """the iteration: the ORIGINAL raster resampled by the shift so far, the increment estimated and added
    -> (px_x, px_y, tz, history of (dx px, dy px, dz, N), converged)"""
    px_x = px_y = tz = 0.0
    history, converged = [], False
    for _ in range(max_iter):
        cur = translate(src, nodata, px_x, px_y, tz, float("nan"))
        sums, _ = shift_sums(cur, ref, cls, need, nodata, gsd_x, gsd_y, thr, slope_max)
        r = solve(sums)
        dx, dy, dz = r["tx"] / gsd_x, r["ty"] / gsd_y, r["tz"]
        px_x, px_y, tz = px_x + dx, px_y + dy, tz + dz
        history.append((dx, dy, dz, r["count"]))
        if abs(dx) < tol and abs(dy) < tol and abs(dz) < tol:
            converged = True
            break
    return px_x, px_y, tz, history, converged


# ---- the analytic surface of the tests ------------------------------------------------------------------------------------------
def surface(x, y, box=False):
    z = 5.0 * np.sin(x / 9.0) * np.cos(y / 7.0) + 3.0 * np.sin((x + 2.0 * y) / 13.0) \
        + 8.0 * np.exp(-((x - 40.0) ** 2 + (y - 50.0) ** 2) / 200.0) + 0.05 * x
    if box:
        z = z + 12.0 * ((np.abs(x - 30.0) < 8.0) & (np.abs(y - 60.0) < 10.0))
    return z


def shifted_pair(rows, cols, sx, sy, sz, box=False):
    """G = f on the grid, S(y, x) = f(x + sx, y + sy) - sz: the shift that puts S onto G is (sx, sy) pixels and sz"""
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    return surface(x + sx, y + sy, box) - sz, surface(x, y, box)


# (rows, cols, sx, sy, sz, gsd): the cases of the issue
CASES = [(96, 96, 0.7, -0.4, 1.5, 1.0), (96, 128, -1.3, 0.6, -0.8, 0.5), (64, 64, 2.2, 1.7, 0.3, 0.25), (96, 96, 0.0, 0.0, 0.0, 1.0)]
BOX_CASE = (96, 96, 0.7, -0.4, 1.5, 1.0)
BAR_PX, BAR_M = 0.01, 0.002
