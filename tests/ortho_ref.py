"""numpy fp64 restatement of include/resdepth_hip_ortho.h, test infrastructure only: the RPC00B projection, the forward (alpha) and
inverse (beta) Krueger series to n^4 on WGS84, and the three resamplers with their "needed tap" rules, returning values, validity
and sum |w v| per pixel.  Written from the definitions, not from the kernel: the multiples of the angles are taken directly, the
latitude comes from the fixed-point iteration on the isometric latitude (the kernel takes Newton steps on the tangent)."""
import math

import numpy as np

A_WGS, F_WGS, K0, FALSE_EASTING = 6378137.0, 1.0 / 298.257223563, 0.9996, 500000.0
N_ = F_WGS / (2.0 - F_WGS)
E2 = F_WGS * (2.0 - F_WGS)
E_ = math.sqrt(E2)
A_RECT = A_WGS / (1.0 + N_) * (1.0 + N_ ** 2 / 4.0 + N_ ** 4 / 64.0)
ALPHA = (N_ / 2 - 2 * N_ ** 2 / 3 + 5 * N_ ** 3 / 16 + 41 * N_ ** 4 / 180,
         13 * N_ ** 2 / 48 - 3 * N_ ** 3 / 5 + 557 * N_ ** 4 / 1440,
         61 * N_ ** 3 / 240 - 103 * N_ ** 4 / 140,
         49561 * N_ ** 4 / 161280)
BETA = (N_ / 2 - 2 * N_ ** 2 / 3 + 37 * N_ ** 3 / 96 - N_ ** 4 / 360,
        N_ ** 2 / 48 + N_ ** 3 / 15 - 437 * N_ ** 4 / 1440,
        17 * N_ ** 3 / 480 - 37 * N_ ** 4 / 840,
        4397 * N_ ** 4 / 161280)
SCALARS = ("line_off", "samp_off", "lat_off", "lon_off", "height_off", "line_scale", "samp_scale", "lat_scale", "lon_scale",
           "height_scale")
VECTORS = ("line_num", "line_den", "samp_num", "samp_den")


# ---- transverse Mercator -----------------------------------------------------------------------------------------------------------
def utm_forward(lon, lat, lon0_deg, false_northing, terms=4):
    """degrees -> (easting, northing)"""
    lon, lat = np.asarray(lon, np.float64), np.asarray(lat, np.float64)
    dl = np.radians(lon - lon0_deg)
    tau = np.tan(np.radians(lat))
    sigma = np.sinh(E_ * np.arctanh(E_ * tau / np.sqrt(1.0 + tau * tau)))
    taup = tau * np.sqrt(1.0 + sigma * sigma) - sigma * np.sqrt(1.0 + tau * tau)
    xip = np.arctan2(taup, np.cos(dl))
    etap = np.arcsinh(np.sin(dl) / np.sqrt(taup * taup + np.cos(dl) ** 2))
    xi, eta = xip.copy(), etap.copy()
    for j in range(1, terms + 1):
        xi = xi + ALPHA[j - 1] * np.sin(2 * j * xip) * np.cosh(2 * j * etap)
        eta = eta + ALPHA[j - 1] * np.cos(2 * j * xip) * np.sinh(2 * j * etap)
    return FALSE_EASTING + K0 * A_RECT * eta, false_northing + K0 * A_RECT * xi


def utm_inverse(easting, northing, lon0_deg, false_northing, terms=4, iterations=12):
    """(easting, northing) -> degrees (lon, lat)"""
    xi = (np.asarray(northing, np.float64) - false_northing) / (K0 * A_RECT)
    eta = (np.asarray(easting, np.float64) - FALSE_EASTING) / (K0 * A_RECT)
    xip, etap = xi.copy(), eta.copy()
    for j in range(1, terms + 1):
        xip = xip - BETA[j - 1] * np.sin(2 * j * xi) * np.cosh(2 * j * eta)
        etap = etap - BETA[j - 1] * np.cos(2 * j * xi) * np.sinh(2 * j * eta)
    dl = np.arctan2(np.sinh(etap), np.cos(xip))
    taup = np.sin(xip) / np.sqrt(np.sinh(etap) ** 2 + np.cos(xip) ** 2)
    psi = np.arcsinh(taup)                               # isometric latitude
    phi = np.arctan(taup)                                # start: the conformal latitude
    for _ in range(iterations):
        phi = np.arcsin(np.tanh(psi + E_ * np.arctanh(E_ * np.sin(phi))))
    return lon0_deg + np.degrees(dl), np.degrees(phi)


# ---- RPC00B ------------------------------------------------------------------------------------------------------------------------
def monomials(P, L, H):
    return [np.ones_like(P), L, P, H, L * P, L * H, P * H, L * L, P * P, H * H, P * L * H, L ** 3, L * P * P, L * H * H, L * L * P,
            P ** 3, P * H * H, L * L * H, P * P * H, H ** 3]


def rpc_project(m, lon, lat, h):
    """m: dict of the RPC fields -> (line, samp)"""
    P, L, H = (lat - m["lat_off"]) / m["lat_scale"], (lon - m["lon_off"]) / m["lon_scale"], (h - m["height_off"]) / m["height_scale"]
    mono = monomials(P, L, H)
    poly = lambda k: sum(float(k[i]) * mono[i] for i in range(20))
    line = poly(m["line_num"]) / poly(m["line_den"]) * m["line_scale"] + m["line_off"]
    samp = poly(m["samp_num"]) / poly(m["samp_den"]) * m["samp_scale"] + m["samp_off"]
    return line, samp


def ground(rows, cols, gt, crs, lon0_deg=0.0, false_northing=0.0):
    """the pixel centres of the grid in degrees -> (lon, lat), each [rows, cols]"""
    x0, dx, y0, dy = gt
    X = np.broadcast_to(x0 + (np.arange(cols, dtype=np.float64) + 0.5) * dx, (rows, cols))
    Y = np.broadcast_to((y0 + (np.arange(rows, dtype=np.float64) + 0.5) * dy)[:, None], (rows, cols))
    if crs == "geographic":
        return X.copy(), Y.copy()
    return utm_inverse(X, Y, lon0_deg, false_northing)


def coords(dsm, nodata, gt, crs, lon0_deg, false_northing, height_offset, models, origins):
    """-> (coords [P, rows, cols, 2] with NaN where the DSM is undefined, defined [rows, cols])"""
    z = np.asarray(dsm, np.float32).astype(np.float64)
    rows, cols = z.shape
    defined = ~(np.isnan(z) | (z == nodata))
    lon, lat = ground(rows, cols, gt, crs, lon0_deg, false_northing)
    out = np.full((len(models), rows, cols, 2), np.nan)
    with np.errstate(all="ignore"):
        for v, (m, (line0, samp0)) in enumerate(zip(models, origins)):
            line, samp = rpc_project(m, lon, lat, z + height_offset)
            out[v, ..., 0] = np.where(defined, line - line0, np.nan)
            out[v, ..., 1] = np.where(defined, samp - samp0, np.nan)
    return out, defined


# ---- the resamplers ------------------------------------------------------------------------------------------------------------------
def _cubic(t):
    return [((-0.5 * t + 1.0) * t - 0.5) * t, (1.5 * t - 2.5) * t * t + 1.0, ((-1.5 * t + 2.0) * t + 0.5) * t, (0.5 * t - 0.5) * t * t]


def resample(image, image_nodata, yi, xi, kind):
    """image: 2-D array of any of the three element types; yi, xi: fp64 positions of any one shape (NaN: undefined)
    -> (value fp64, valid bool, sum |w v| fp64), value and the sum 0 where not valid"""
    img = np.asarray(image).astype(np.float64)
    rows, cols = img.shape
    nd = np.nan if image_nodata is None else float(image_nodata)
    shape = np.shape(yi)
    yi, xi = np.asarray(yi, np.float64).ravel(), np.asarray(xi, np.float64).ravel()
    with np.errstate(all="ignore"):
        if kind == "nearest":
            y0, x0 = np.floor(yi + 0.5), np.floor(xi + 0.5)
            ok = (y0 >= 0) & (x0 >= 0) & (y0 <= rows - 1) & (x0 <= cols - 1)
            v = img[np.where(ok, y0, 0).astype(np.int64), np.where(ok, x0, 0).astype(np.int64)]
            ok &= ~(v == nd)
            val, mag = v, np.abs(v)
        else:
            y0, x0 = np.floor(yi), np.floor(xi)
            fy, fx = yi - y0, xi - x0
            two_y, two_x = fy != 0, fx != 0
            if kind == "bilinear":
                ok = (y0 >= 0) & (x0 >= 0) & (y0 <= rows - 1 - two_y) & (x0 <= cols - 1 - two_x)
                iy, ix = np.where(ok, y0, 0).astype(np.int64), np.where(ok, x0, 0).astype(np.int64)
                iy1, ix1 = iy + (two_y & ok), ix + (two_x & ok)
                v00, v01, v10, v11 = img[iy, ix], img[iy, ix1], img[iy1, ix], img[iy1, ix1]
                ok &= ~((v00 == nd) | (v01 == nd) | (v10 == nd) | (v11 == nd))
                fy, fx = np.where(ok, fy, 0.0), np.where(ok, fx, 0.0)
                top, bot = v00 + fx * (v01 - v00), v10 + fx * (v11 - v10)
                val = top + fy * (bot - top)
                mag = (np.abs((1 - fx) * (1 - fy) * v00) + np.abs(fx * (1 - fy) * v01) + np.abs((1 - fx) * fy * v10)
                       + np.abs(fx * fy * v11))
            elif kind == "bicubic":
                ok = (y0 - two_y >= 0) & (x0 - two_x >= 0) & (y0 + 2 * two_y <= rows - 1) & (x0 + 2 * two_x <= cols - 1)
                iy, ix = np.where(ok, y0, 0).astype(np.int64), np.where(ok, x0, 0).astype(np.int64)
                fy, fx = np.where(ok, fy, 0.0), np.where(ok, fx, 0.0)
                sy, sx = (two_y & ok).astype(np.int64), (two_x & ok).astype(np.int64)
                wy, wx = _cubic(fy), _cubic(fx)
                val, mag, bad = np.zeros_like(fy), np.zeros_like(fy), np.zeros(fy.shape, bool)
                for j in range(4):
                    rs = np.zeros_like(fy)
                    for i in range(4):
                        v = img[iy + (j - 1) * sy, ix + (i - 1) * sx]
                        needed = (sy.astype(bool) | (j == 1)) & (sx.astype(bool) | (i == 1))
                        bad |= needed & (v == nd)
                        rs = rs + wx[i] * v
                        mag = mag + np.abs(wy[j] * wx[i] * v)
                    val = val + wy[j] * rs
                ok &= ~bad
            else:
                raise ValueError(kind)
    val, mag = np.where(ok, val, 0.0), np.where(ok, mag, 0.0)
    return val.reshape(shape), ok.reshape(shape), mag.reshape(shape)


# ---- synthetic models --------------------------------------------------------------------------------------------------------------
def synthetic_rpc(lon_range, lat_range, h_range, img_rows, img_cols, angle_deg=30.0, zoom=1.1, shift=(0.0, 0.0), seed=0,
                  small=1e-3):
    """An RPC whose affine core maps the ground rectangle onto the image turned by angle_deg about its centre, `zoom` times its
    half-size (> 1: partly off it), plus terms of second and third order of relative size `small`; denominators are 1 + small."""
    rng = np.random.default_rng(seed)
    m = dict(lon_off=0.5 * (lon_range[0] + lon_range[1]), lon_scale=0.5 * abs(lon_range[1] - lon_range[0]),
             lat_off=0.5 * (lat_range[0] + lat_range[1]), lat_scale=0.5 * abs(lat_range[1] - lat_range[0]),
             height_off=0.5 * (h_range[0] + h_range[1]), height_scale=max(0.5 * abs(h_range[1] - h_range[0]), 1.0),
             line_off=0.5 * (img_rows - 1) + shift[0], samp_off=0.5 * (img_cols - 1) + shift[1],
             line_scale=0.5 * img_rows, samp_scale=0.5 * img_cols)
    ca, sa = math.cos(math.radians(angle_deg)) * zoom, math.sin(math.radians(angle_deg)) * zoom
    for name, (kl, kp) in (("line", (sa, -ca)), ("samp", (ca, sa))):       # north is up: the line falls as the latitude rises
        num = rng.uniform(-small, small, 20)
        num[0], num[1], num[2], num[3] = 0.0, kl, kp, 0.05
        den = rng.uniform(-small, small, 20)
        den[0] = 1.0
        m[name + "_num"], m[name + "_den"] = num, den
    return m


def integer_rpc(lon0, lat0, step, off_line, off_samp):
    """pixel (r, c) of the grid whose centres are lon0 + c * step, lat0 - r * step (step a power of two) lands EXACTLY on
    (r + off_line, c + off_samp): every product and sum of the projection is exact"""
    zeros = np.zeros(20)
    one = zeros.copy()
    one[0] = 1.0
    sn, ln = zeros.copy(), zeros.copy()
    sn[1], ln[2] = 1.0, -1.0
    return dict(lon_off=lon0, lon_scale=64.0 * step, lat_off=lat0, lat_scale=64.0 * step, height_off=0.0, height_scale=1.0,
                line_off=float(off_line), samp_off=float(off_samp), line_scale=64.0, samp_scale=64.0,
                line_num=ln, line_den=one.copy(), samp_num=sn, samp_den=one.copy())
