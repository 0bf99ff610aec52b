"""include/resdepth_hip_coreg.h on the GPU (-m gpu): rd_shift_sums and rd_translate_bilinear against the numpy oracle
tests/coreg_ref.py, and the front end on top of them (resdepth_amd.coregistration estimate_shift, coregister, translate).

The sums: N is compared for equality; each of the nine sums is held to N * 2^-53 * sum |term| of the oracle's math.fsum, the worst
case of ANY order of summation -- kernel and oracle form the same terms bit for bit (every operation separately rounded on either
side) and differ in the order of the additions only, so the bound is derived, not tuned.  The resampler is compared bit for bit.
The iteration is held to the bars of tests/test_coreg_cpu.py against the truth (0.01 px, 0.002 m) and to 1e-6 px against the
oracle's iteration, four orders below that bar: the two differ in summation order only."""
import functools
import math
import struct

import numpy as np
import pytest
import torch

import coreg_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NODATA = -9999.0
GSD_X, GSD_Y = 0.5, 0.75                              # different, so that a swapped pair shows
U = 2.0 ** -53


@pytest.fixture(scope="module")
def lib():
    from resdepth_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, offset=0):
    """host array -> a contiguous device tensor of its dtype, `offset` elements into its allocation"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not offset:
        return t.to(DEV)
    buf = torch.empty(t.numel() + offset, dtype=t.dtype, device=DEV)
    view = buf[offset:].view(t.shape)
    view.copy_(t)
    return view


def _shift_sums(lib, src, ref, cls, need, nodata, thr, slope_max, offset=0, gsd_x=GSD_X, gsd_y=GSD_Y):
    rows, cols = src.shape
    s, g = _dev(src, offset), _dev(ref)
    c = None if cls is None else _dev(cls)
    nb = lib.rd_shift_sums_ws_bytes(rows, cols)
    ws = torch.full((max(nb // 8, 1),), 777.0, dtype=torch.float64, device=DEV)
    out = torch.full((10,), 12345.0, dtype=torch.float64, device=DEV)
    with torch.cuda.device(DEV):
        rc = lib.rd_shift_sums(s.data_ptr(), int(src.dtype == np.float64), g.data_ptr(), int(ref.dtype == np.float64),
                               None if c is None else c.data_ptr(), need, rows, cols, float(nodata), gsd_x, gsd_y, float(thr),
                               float(slope_max), ws.data_ptr(), nb, out.data_ptr(), _stream())
    assert rc == 0, lib.rd_last_error_string()
    return out.cpu().numpy()


def _pair(rows, cols, defects=True):
    """a source and a reference of the analytic surface half a pixel apart, noise on the source, and -- on rasters large enough to
    keep members -- nodata on and beside the tile seams (x = 63, 64, 65; y = 15, 16, 17) and in a corner, a NaN and a nodata in the
    reference, an Inf in the source; a class raster with bit 0 on about two thirds of the pixels"""
    rng = np.random.RandomState(rows * 1000 + cols)
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    src = R.surface(x + 0.4, y - 0.3) - 0.2 + 0.05 * rng.standard_normal((rows, cols))
    ref = R.surface(x, y)
    cls = (rng.randint(0, 3, (rows, cols)) > 0).astype(np.uint8) | (rng.randint(0, 2, (rows, cols)) << 2).astype(np.uint8)
    if defects and rows * cols >= 3 * 64:
        for k, xs in enumerate((63, 64, 65)):
            if xs < cols:
                src[(1 + 5 * k) % rows, xs] = NODATA
        for k, ys in enumerate((15, 16, 17)):
            if ys < rows:
                src[ys, (9 + 20 * k) % cols] = NODATA
        src[0, 0] = NODATA
        ref[rows // 2, cols // 3] = np.nan
        ref[rows // 2, cols // 3 + 2] = NODATA
        src[rows // 2, (2 * cols) // 3] = np.inf
    return src, ref, cls


# 64 x 16 tiles: nothing interior, one member, one row of tiles, one full interior tile and its neighbours by one, several tiles
SHAPES = [(1, 1), (2, 5), (3, 3), (3, 64), (18, 66), (17, 65), (19, 67), (33, 130), (50, 200)]
# (source f64, reference f64, need, thr, slope_max as a tangent)
CONFIGS = [(1, 1, 0, 0.0, 0.0), (0, 0, 1, 0.0, 0.0), (0, 1, 0, 0.3, 0.0), (1, 0, 1, 0.3, 1.0), (1, 1, 0, 0.0, 1.0), (0, 0, 5, 0.0, 0.0)]


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "s%d_r%d_need%d_thr%g_cap%g" % c)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_shift_sums_against_the_oracle(lib, shape, cfg):
    src_f64, ref_f64, need, thr, cap = cfg
    src, ref, cls = _pair(*shape)
    src = src.astype(np.float64 if src_f64 else np.float32)
    ref = ref.astype(np.float64 if ref_f64 else np.float32)
    want, mags = R.shift_sums(src, ref, cls, need, NODATA, GSD_X, GSD_Y, thr, cap)
    got = _shift_sums(lib, src, ref, cls if need else None, need, NODATA, thr, cap)
    n = want[0]
    print(f"{shape} {cfg}: N = {int(n)} (kernel {got[0]:.0f})")
    assert got[0] == n
    for k in range(1, 10):
        bound = n * U * mags[k]
        print(f"  sum {k}: |kernel - fsum| = {abs(got[k] - want[k]):.3e}, bound {bound:.3e}")
        assert abs(got[k] - want[k]) <= bound, (k, got[k], want[k], bound)
    if shape in ((1, 1), (2, 5)):
        assert n == 0
    if n == 0:
        np.testing.assert_array_equal(got.view(np.uint64), np.zeros(10, np.uint64))
    again = _shift_sums(lib, src, ref, cls if need else None, need, NODATA, thr, cap)
    moved = _shift_sums(lib, src, ref, cls if need else None, need, NODATA, thr, cap, offset=1)
    np.testing.assert_array_equal(again.view(np.uint64), got.view(np.uint64), err_msg="two calls differ")
    np.testing.assert_array_equal(moved.view(np.uint64), got.view(np.uint64), err_msg="a source one element further differs")


def test_shift_sums_members_by_hand(lib):
    """3 x 3: exactly one member, and its terms are the sums; the defects of _pair really take members away"""
    src, ref, _ = _pair(3, 3)
    got = _shift_sums(lib, src, ref, None, 0, NODATA, 0.0, 0.0)
    _, ts = R.terms(src, ref, None, 0, NODATA, GSD_X, GSD_Y)
    assert got[0] == 1
    np.testing.assert_array_equal(got[1:].view(np.uint64), np.array([t[1, 1] for t in ts]).view(np.uint64))
    clean = _pair(50, 200, defects=False)
    full = _shift_sums(lib, clean[0], clean[1], None, 0, NODATA, 0.0, 0.0)
    assert full[0] == 48 * 198
    src, ref, cls = _pair(50, 200)
    holed = _shift_sums(lib, src, ref, None, 0, NODATA, 0.0, 0.0)
    lost = R.shift_sums(clean[0], clean[1], None, 0, NODATA, GSD_X, GSD_Y)[0][0] - R.shift_sums(src, ref, None, 0, NODATA, GSD_X, GSD_Y)[0][0]
    assert full[0] - holed[0] == lost and lost >= 40
    # nodata NaN: no value is nodata, so -9999 votes (and is cut by nothing); the NaN and the Inf still do not
    nan_nd = _shift_sums(lib, src, ref, None, 0, float("nan"), 0.0, 0.0)
    assert nan_nd[0] == R.shift_sums(src, ref, None, 0, float("nan"), GSD_X, GSD_Y)[0][0] > holed[0]


def test_zero_members_give_ten_zeros(lib):
    src, ref, cls = _pair(33, 130)
    for need, c, thr in ((1, np.zeros_like(cls), 0.0), (0, None, 1e-9), (2, cls, 0.0)):
        got = _shift_sums(lib, src, ref, c, need, NODATA, thr, 0.0)
        np.testing.assert_array_equal(got.view(np.uint64), np.zeros(10, np.uint64))
    flat = np.full((20, 70), NODATA)
    np.testing.assert_array_equal(_shift_sums(lib, flat, flat, None, 0, NODATA, 0.0, 0.0).view(np.uint64), np.zeros(10, np.uint64))


def test_shift_sums_walks_several_tiles_per_block(lib):
    """2112 tiles: two per block.  Values on a grid of 2^-6 below 2^6 make every term and every partial sum exact in fp64, so the
    kernel's sums EQUAL the oracle's whatever the order"""
    rows, cols = 16 * 32 + 1, 64 * 64
    assert lib.rd_shift_sums_ws_bytes(rows, cols) == 80 * 1056
    rng = np.random.RandomState(5)
    src = rng.randint(-2 ** 12, 2 ** 12, (rows, cols)) / 64.0
    ref = rng.randint(-2 ** 12, 2 ** 12, (rows, cols)) / 64.0
    src[100, 200] = src[512, 4095] = NODATA
    got = _shift_sums(lib, src, ref, None, 0, NODATA, 0.0, 0.0, gsd_x=1.0, gsd_y=0.5)
    s, g = torch.from_numpy(src).to(DEV), torch.from_numpy(ref).to(DEV)
    a, b, c = s[:-2, :-2], s[:-2, 1:-1], s[:-2, 2:]
    d4, e, f = s[1:-1, :-2], s[1:-1, 1:-1], s[1:-1, 2:]
    g7, h, i = s[2:, :-2], s[2:, 1:-1], s[2:, 2:]
    p = ((c + 2 * f + i) - (a + 2 * d4 + g7)) / 8.0
    q = ((g7 + 2 * h + i) - (a + 2 * b + c)) / 4.0
    d = g[1:-1, 1:-1] - e
    bad = torch.nn.functional.max_pool2d((s == NODATA)[None, None].double(), 3, 1)[0, 0] > 0
    ok = ~bad
    want = [ok.sum().double()] + [(t * ok).sum() for t in (p, q, d, p * p, p * q, q * q, p * d, q * d, d * d)]
    np.testing.assert_array_equal(got, np.array([float(v) for v in want]))
    assert got[0] == (rows - 2) * (cols - 2) - 9 - 1                # an interior cell spoils nine pixels, the corner cell one


# ---- the resampler ----------------------------------------------------------------------------------------------------------------
def _translate(lib, src, nodata, tx, ty, tz, fill):
    rows, cols = src.shape
    s = _dev(src)
    out = torch.full((rows, cols), 4321.0, dtype=torch.float64, device=DEV)
    with torch.cuda.device(DEV):
        rc = lib.rd_translate_bilinear(s.data_ptr(), int(src.dtype == np.float64), rows, cols, float(nodata), tx, ty, tz, fill,
                                       out.data_ptr(), _stream())
    assert rc == 0, lib.rd_last_error_string()
    return out.cpu().numpy()


def _heights(rows, cols, dtype):
    rng = np.random.RandomState(rows * 77 + cols)
    z = (300.0 + 5.0 * rng.standard_normal((rows, cols))).astype(dtype)
    if rows * cols > 8:
        z[rows // 2, cols // 2] = NODATA
        z[rows - 1, 0] = NODATA
        z[rows // 3, (2 * cols) // 3] = np.nan
    return z


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (5, 1), (17, 65), (33, 130)], ids=lambda s: "%dx%d" % s)
def test_translate_bit_equal_to_the_oracle(lib, shape, dtype):
    rows, cols = shape
    src = _heights(rows, cols, dtype)
    odd_nan = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000123))[0]
    combos = ((0.0, float("nan")), (1.25, NODATA), (-0.1, odd_nan))
    shifts = ((0.0, 0.0), (1.0, 0.0), (0.0, -2.0), (0.5, 0.5), (-0.25, 0.75), (float(cols), 0.0), (1e300, 0.0), (0.0, -1e300),
              (0.3, 0.0), (0.0, 0.6))
    for k, (tx, ty) in enumerate(shifts):
        for tz, fill in (combos if k in (3, 4) else combos[k % 3:k % 3 + 1]):      # every combination on the sub-pixel shifts
            got = _translate(lib, src, NODATA, tx, ty, tz, fill)
            want = R.translate(src, NODATA, tx, ty, tz, fill)
            np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64), err_msg=f"shift ({tx}, {ty}), tz {tz}, fill {fill}")
            if abs(tx) >= cols or abs(ty) >= rows:
                want_bits = np.uint64(R.NAN_BITS) if fill != fill else np.array([fill]).view(np.uint64)[0]
                assert (got.view(np.uint64) == want_bits).all(), (tx, ty)
    # whole pixels: a plain slice copy, nodata and NaN become the fill, the last row and column survive
    clean = np.where(np.isnan(src) | (src == NODATA), -7.0, src.astype(np.float64))
    np.testing.assert_array_equal(_translate(lib, src, NODATA, 0.0, 0.0, 0.0, -7.0).view(np.uint64), clean.view(np.uint64))
    if cols > 1:
        got = _translate(lib, src, NODATA, 1.0, 0.0, 0.0, -7.0)
        np.testing.assert_array_equal(got[:, 1:].view(np.uint64), np.ascontiguousarray(clean[:, :-1]).view(np.uint64))
        assert (got[:, 0] == -7.0).all()
    if rows > 2:
        got = _translate(lib, src, NODATA, 0.0, -2.0, 0.0, -7.0)
        np.testing.assert_array_equal(got[:-2].view(np.uint64), np.ascontiguousarray(clean[2:]).view(np.uint64))
        assert (got[-2:] == -7.0).all()


# ---- the front end ----------------------------------------------------------------------------------------------------------------
def test_estimate_shift_returns_the_kernels_sums_and_their_solution(lib):
    from resdepth_amd import estimate_shift
    src, ref, cls = _pair(50, 200)
    mask = (cls & 1).astype(bool)
    src32 = src.astype(np.float32)
    for kw, raw in ((dict(), (None, 0, 0.0, 0.0)),
                    (dict(mask=mask, residual_threshold=0.3, max_slope=50.0), (mask.astype(np.uint8), 1, 0.3, math.tan(math.radians(50.0))))):
        est = estimate_shift(src32, torch.from_numpy(ref).to(DEV), (GSD_Y, GSD_X), nodata=NODATA, **kw)
        sums = _shift_sums(lib, src32, ref, raw[0], raw[1], NODATA, raw[2], raw[3])
        np.testing.assert_array_equal(np.asarray(est.sums).view(np.uint64), sums.view(np.uint64))
        a, b, c = np.linalg.solve(np.array([[sums[4], sums[5], sums[1]], [sums[5], sums[6], sums[2]], [sums[1], sums[2], sums[0]]]),
                                  np.array([sums[7], sums[8], sums[3]]))
        assert (est.tx, est.ty, est.tz) == (-a, -b, c) and est.px == (est.tx / GSD_X, est.ty / GSD_Y)
        assert est.count == int(sums[0]) > 1000 and est.sigma0 > 0 and est.cov.shape == (3, 3)
        assert np.all(np.diag(est.cov) > 0) and np.allclose(est.cov, est.cov.T)
    y, x = np.mgrid[0:40, 0:50].astype(np.float64)
    for flat in (0.3 * x - 0.2 * y + 4.0, np.full((40, 50), 7.0)):
        with pytest.raises(RuntimeError, match="constrain"):
            estimate_shift(flat, flat + 0.5, 1.0)
    with pytest.raises(RuntimeError, match="three"):
        estimate_shift(src, ref, 1.0, mask=np.zeros_like(mask))


@functools.lru_cache(maxsize=None)
def _oracle_run(case, box):
    rows, cols, sx, sy, sz, gsd = case
    src, ref = R.shifted_pair(rows, cols, sx, sy, sz, box=box)
    cap = math.tan(math.radians(45.0)) if box else 0.0
    return src, ref, R.coregister(src, ref, gsd, gsd, tol=1e-4, slope_max=cap)


@pytest.mark.parametrize("case,box", [(c, False) for c in R.CASES[:3]] + [(R.BOX_CASE, True)],
                         ids=lambda v: "box" if v is True else "" if v is False else "%dx%d_%g_%g_%g" % v[:5])
def test_coregister_recovers_the_shift_and_follows_the_oracle(case, box):
    from resdepth_amd import coregister, translate
    rows, cols, sx, sy, sz, gsd = case
    src, ref, (ox, oy, oz, ohist, oconv) = _oracle_run(case, box)
    res = coregister(src, ref, gsd, tol=1e-4, max_slope=45.0 if box else None)
    px, py = res.shift.px
    print(f"{case} box={box}: against the truth {px - sx:+.3e} px, {py - sy:+.3e} px, {res.shift.tz - sz:+.3e} m; against the "
          f"oracle {px - ox:+.3e} px, {py - oy:+.3e} px, {res.shift.tz - oz:+.3e} m; {len(res.history)} iterations")
    assert res.converged and oconv and len(res.history) == len(ohist)
    assert abs(px - sx) <= R.BAR_PX and abs(py - sy) <= R.BAR_PX and abs(res.shift.tz - sz) <= R.BAR_M
    assert abs(px - ox) <= 1e-6 and abs(py - oy) <= 1e-6 and abs(res.shift.tz - oz) <= 1e-6
    assert [h.count for h in res.history] == [h[3] for h in ohist]
    assert res.shift.tx == px * gsd and res.shift.ty == py * gsd and res.shift.count == res.history[-1].count
    again = translate(src, res.shift.px, res.shift.tz)
    assert res.shifted.dtype == torch.float64 and tuple(res.shifted.shape) == (rows, cols) and res.shifted.is_cuda
    assert torch.equal(res.shifted.view(torch.int64), again.view(torch.int64))
    # the shifted raster now lies on the reference: the residual away from the border (and the box's walls) is small
    r = (res.shifted - torch.from_numpy(ref).to(DEV))[4:-4, 4:-4]
    assert float(r.abs().median()) < 0.02


def test_coregister_zero_shift_and_iteration_limit():
    from resdepth_amd import coregister
    rows, cols, sx, sy, sz, gsd = R.CASES[3]
    src, ref = R.shifted_pair(rows, cols, sx, sy, sz)
    res = coregister(src, ref, gsd, tol=1e-4)
    assert res.converged and len(res.history) == 1 and res.shift.px == (0.0, 0.0) and res.shift.tz == 0.0
    assert torch.equal(res.shifted, torch.from_numpy(src).to(DEV))
    rows, cols, sx, sy, sz, gsd = R.CASES[0]
    src, ref = R.shifted_pair(rows, cols, sx, sy, sz)
    one = coregister(src, ref, gsd, tol=1e-4, max_iter=1)
    assert not one.converged and len(one.history) == 1 and one.shift.px == one.history[0].px


def test_round_trip_into_the_evaluation():
    """coregister(..., fill=nodata) goes straight into evaluate_statistics, which counts the defined pixels only"""
    from resdepth_amd import coregister, evaluate_statistics
    rows, cols, sx, sy, sz, gsd = R.CASES[0]
    src, ref = R.shifted_pair(rows, cols, sx, sy, sz)
    src[10:13, 20:24] = NODATA
    res = coregister(src.astype(np.float32), ref.astype(np.float32), gsd, tol=1e-4, fill=NODATA, nodata=NODATA)
    defined = int((res.shifted != NODATA).sum())
    assert 0 < defined < rows * cols and not bool(torch.isnan(res.shifted).any())
    stats = evaluate_statistics(res.shifted, src.astype(np.float32), ref.astype(np.float32), nodata=NODATA)
    assert stats.after["all"].count_total == defined
    assert stats.before["all"].count_total == rows * cols - 12
    assert stats.after["all"].RMSE < 0.1 * stats.before["all"].RMSE         # the offset was most of the "error"
