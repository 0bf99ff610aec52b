"""include/resdepth_hip_errmap.h on the GPU (-m gpu): rd_cell_stats against the loop over cells of tests/errmap_ref.py and against
the statistics engine itself, rd_dsm_slope and rd_bin_classes against their restatements, and the front end on top of them
(resdepth_amd.evaluation error_map, dsm_slope, evaluate_binned).

Residuals are multiples of 2^-10 below 2^10 unless a test says otherwise: r - absolute median and the mean of two middle values
are then exact in fp64, so count, max, min and the three medians are compared for equality; MAE and RMSE are held to
rtol = atol = 1e-12, the bar tests/test_eval_classes_gpu.py holds the engine to."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import errmap_ref as R
import eval_classes_ref as RC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NODATA = -9999.0


@pytest.fixture(scope="module")
def lib():
    from resdepth_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _residuals(rng, shape):
    return rng.randint(-2 ** 20 + 1, 2 ** 20, size=shape) / 1024.0


def _cells(lib, r, cls, cell_h, cell_w, need=0, thr=0.0, r_dev=None):
    """rd_cell_stats on host arrays (or on the device tensor r_dev in place of r) -> host [ncy, ncx, 8]"""
    rows, cols = cls.shape
    rd = torch.from_numpy(np.ascontiguousarray(r, np.float64)).to(DEV) if r_dev is None else r_dev
    cd = torch.from_numpy(np.ascontiguousarray(cls, np.uint8)).to(DEV)
    ncy, ncx = -(-rows // cell_h), -(-cols // cell_w)
    out = torch.full((ncy, ncx, 8), 12345.0, dtype=torch.float64, device=DEV)
    with torch.cuda.device(DEV):
        rc = lib.rd_cell_stats(rd.data_ptr(), cd.data_ptr(), rows, cols, cell_h, cell_w, need, float(thr), out.data_ptr(), _stream())
    assert rc == 0, lib.rd_last_error_string()
    return out.cpu().numpy()


def _assert_cells(got, want, what=""):
    assert got.shape == want.shape, (got.shape, want.shape)
    for k in range(8):
        print(f"{what} {R.KEYS[k]}: max |got - want| = {np.nanmax(np.abs(got[..., k] - want[..., k]), initial=0.0):.3e}")
    np.testing.assert_array_equal(got[..., R.EXACT], want[..., R.EXACT], err_msg=what)
    np.testing.assert_allclose(got[..., R.SUMS], want[..., R.SUMS], rtol=1e-12, atol=1e-12, equal_nan=True, err_msg=what)


# 37 x 53 at cell 8: ragged cells of 5 rows and of 5 columns; 300 x 260 at cell 256: cells of 44 rows and of 4 columns
SHAPES = [((37, 53), (8, 8)), ((9, 9), (4, 4)), ((300, 260), (256, 256)), ((64, 64), (16, 64)), ((1, 1), (4, 4))]


@pytest.mark.parametrize("shape,cell", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_cell_stats_match_the_loop_over_cells(lib, shape, cell):
    rng = np.random.RandomState(shape[0] * 1000 + shape[1])
    r = _residuals(rng, shape)
    cls = (rng.rand(*shape) < 0.8).astype(np.uint8) | ((rng.rand(*shape) < 0.5).astype(np.uint8) << 2)
    for need, thr in ((1, 0.0), (0, 0.0), (1 | 4, 0.0), (1, 300.0)):
        _assert_cells(_cells(lib, r, cls, cell[0], cell[1], need, thr), R.cell_stats(r, cls, cell[0], cell[1], need, thr),
                      f"{shape} cell {cell} need {need} thr {thr}")


def _crafted():
    """37 x 53 in cells of 8: the cells of the first rows are built by hand, the rest is random"""
    rng = np.random.RandomState(11)
    shape = (37, 53)
    r = _residuals(rng, shape)
    cls = (rng.rand(*shape) < 0.8).astype(np.uint8) | ((rng.rand(*shape) < 0.5).astype(np.uint8) << 2)
    win = lambda cy, cx: (slice(cy * 8, cy * 8 + 8), slice(cx * 8, cx * 8 + 8))
    cls[win(0, 0)] = 4                                          # fully masked: the class bit without the validity bit
    for cx, picks in ((1, [(6, 2)]), (2, [(0, 0), (7, 7)]), (3, [(1, 5), (4, 4), (5, 0)])):      # exactly 1, 2 and 3 members
        cls[win(0, cx)] = 0
        for y, x in picks:
            cls[y, cx * 8 + x] = 1
    r[6, 8 + 2] = -3.5
    r[win(1, 0)] = rng.randint(-1, 2, (8, 8)).astype(np.float64)    # heavy ties
    cls[win(1, 0)] |= 1
    z = np.zeros((8, 8))
    z[rng.rand(8, 8) < 0.5] = -0.0                              # -0.0 beside +0.0
    z[0, 0], z[0, 1] = -0.0, 0.0
    r[win(1, 1)] = z
    cls[win(1, 1)] |= 1
    r[win(2, 0)] = 600.0 + np.abs(r[win(2, 0)]) / 4             # a threshold of 512 empties this cell
    cls[win(2, 0)] |= 1
    half = np.abs(r[win(2, 1)]) / 4                             # and halves this one: 32 values above it, 32 below
    half.ravel()[::2] += 600.0
    r[win(2, 1)] = half
    cls[win(2, 1)] |= 1
    return r, cls


def test_cell_stats_on_crafted_cells(lib):
    r, cls = _crafted()
    full = _cells(lib, r, cls, 8, 8, 1, 0.0)
    _assert_cells(full, R.cell_stats(r, cls, 8, 8, 1, 0.0), "crafted")
    assert full[0, 0, 0] == 0 and np.isnan(full[0, 0, 1:]).all()
    np.testing.assert_array_equal(full[0, 1:4, 0], [1, 2, 3])
    np.testing.assert_array_equal(full[0, 1], [1, -3.5, -3.5, 3.5, 3.5, 3.5, -3.5, 1.4826 * 7.0])
    assert set(np.unique(full[1, 0, [1, 2, 5, 6]])) <= {-1.0, -0.5, 0.0, 0.5, 1.0}
    assert full[1, 1, 0] == 64 and (full[1, 1, 1:] == 0.0).all()
    cut = _cells(lib, r, cls, 8, 8, 1, 512.0)
    _assert_cells(cut, R.cell_stats(r, cls, 8, 8, 1, 512.0), "crafted, threshold 512")
    assert cut[2, 0, 0] == 0 and np.isnan(cut[2, 0, 1:]).all() and full[2, 0, 0] == 64
    assert cut[2, 1, 0] == 32 and full[2, 1, 0] == 64
    bit = _cells(lib, r, cls, 8, 8, 1 | 4, 0.0)                 # need with a class bit set
    _assert_cells(bit, R.cell_stats(r, cls, 8, 8, 1 | 4, 0.0), "crafted, need 1 | 4")
    assert (bit[..., 0] <= full[..., 0]).all() and bit[..., 0].sum() < full[..., 0].sum()


def _engine_row(lib, r_dev, cls_dev, need, thr):
    """rd_residual_stats_sets with one set over the whole raster -> host [8]"""
    n = cls_dev.numel()
    out = torch.empty(8, dtype=torch.float64, device=DEV)
    nb = lib.rd_residual_stats_sets_ws_bytes(n, 1)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        rc = lib.rd_residual_stats_sets(r_dev.data_ptr(), None, cls_dev.data_ptr(), n, (C.c_int * 1)(0), (C.c_int * 1)(need),
                                        (C.c_double * 1)(thr if thr > 0 else -1.0), 1, out.data_ptr(), ws.data_ptr(), nb, _stream())
    assert rc == 0, lib.rd_last_error_string()
    return out.cpu().numpy()


def test_every_cell_is_the_engine_on_that_cells_rectangle(lib):
    """96 x 80 in cells of 32 x 40; a NaN and a +Inf are members and rank as the engine ranks them"""
    rng = np.random.RandomState(5)
    shape, ch, cw = (96, 80), 32, 40
    r = _residuals(rng, shape)
    cls = (rng.rand(*shape) < 0.85).astype(np.uint8)
    for (y, x), v in (((3, 5), np.nan), ((40, 50), np.inf), ((70, 10), np.nan), ((71, 11), np.inf), ((5, 60), -np.inf)):
        r[y, x], cls[y, x] = v, 1
    r[80, 70], cls[80, 70] = -np.nan, 1                        # either sign of NaN has its place in the key order
    got = _cells(lib, r, cls, ch, cw, 1, 0.0)
    rd = torch.from_numpy(r).to(DEV)
    for cy in range(3):
        for cx in range(2):
            only = np.zeros_like(cls)
            win = (slice(cy * ch, (cy + 1) * ch), slice(cx * cw, (cx + 1) * cw))
            only[win] = cls[win]
            want = _engine_row(lib, rd, torch.from_numpy(only).to(DEV), 1, 0.0)
            row = got[cy, cx]
            print(cy, cx, row, want)
            np.testing.assert_array_equal(row[R.EXACT].view(np.int64), want[R.EXACT].view(np.int64), err_msg=f"cell {cy} {cx}")
            np.testing.assert_allclose(row[R.SUMS], want[R.SUMS], rtol=1e-12, atol=1e-12, equal_nan=True)
    assert got[1, 1, 1] == np.inf and got[0, 1, 2] == -np.inf and got[0, 0, 0] == (cls[:32, :40] != 0).sum()
    # with a threshold the NaN and the infinities are no members: every cell is finite again and matches the restatement
    cut = _cells(lib, r, cls, ch, cw, 1, 1000.0)
    assert np.isfinite(cut).all()
    finite = np.where(np.isfinite(r), r, 0.0)
    _assert_cells(cut, R.cell_stats(finite, cls & np.isfinite(r), ch, cw, 1, 1000.0), "threshold drops NaN and Inf")


def test_cell_stats_give_the_same_bits_every_time_and_at_any_alignment(lib):
    rng = np.random.RandomState(9)
    shape = (70, 133)
    r = rng.laplace(size=shape) * 3.0                           # any doubles: this is about bits, not about the oracle
    cls = (rng.rand(*shape) < 0.7).astype(np.uint8)
    first = _cells(lib, r, cls, 16, 32, 1, 0.0)
    again = _cells(lib, r, cls, 16, 32, 1, 0.0)
    np.testing.assert_array_equal(first.view(np.int64), again.view(np.int64))
    buf = torch.empty(r.size + 1, dtype=torch.float64, device=DEV)
    assert buf.data_ptr() % 16 == 0
    odd = buf[1:]                                              # 8 bytes past a 16-byte boundary
    odd.copy_(torch.from_numpy(r.ravel()))
    shifted = _cells(lib, r, cls, 16, 32, 1, 0.0, r_dev=odd)
    np.testing.assert_array_equal(first.view(np.int64), shifted.view(np.int64))
    assert np.isfinite(first).all() and first[..., 0].sum() == cls.sum()


# ---- rd_dsm_slope ----------------------------------------------------------------------------------------------------------
def _slope(lib, dsm, gsd_y, gsd_x, nodata=NODATA):
    d = torch.from_numpy(np.ascontiguousarray(dsm)).to(DEV)
    rows, cols = dsm.shape
    out = torch.full((rows, cols), 12345.0, dtype=torch.float64, device=DEV)
    with torch.cuda.device(DEV):
        rc = lib.rd_dsm_slope(d.data_ptr(), int(dsm.dtype == np.float64), rows, cols, float(nodata), float(gsd_x), float(gsd_y),
                              out.data_ptr(), _stream())
    assert rc == 0, lib.rd_last_error_string()
    return out.cpu().numpy()


SLOPE_SHAPES = [(3, 3), (4, 70), (67, 5), (130, 97), (2, 9)]


@pytest.mark.parametrize("shape", SLOPE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype,offset", [(np.float32, 0.0), (np.float64, 0.0), (np.float64, 2.0 ** 40 + 1.0)],
                         ids=["f32", "f64", "f64_beyond_f32"])
def test_slope_is_exact_where_the_sum_of_squares_is_a_perfect_square(lib, shape, dtype, offset):
    """integer heights 3 |x - x0| + 8 |y - y0| (+ an offset f32 would round) with GSD 0.25 x 0.5: p is 0 or +-12, q is 0 or +-16,
    so the slope is 0, 12, 16 or 20 -- the square root of a perfect square, which a square root within one ulp gives exactly"""
    rows, cols = shape
    y, x = np.mgrid[0:rows, 0:cols]
    z = (3.0 * np.abs(x - cols // 2) + 8.0 * np.abs(y - rows // 2) + offset).astype(dtype)
    assert (z.astype(np.float64) == 3.0 * np.abs(x - cols // 2) + 8.0 * np.abs(y - rows // 2) + offset).all()
    if rows > 4 and cols > 4:
        z[rows - 2, 1] = NODATA
    got = _slope(lib, z, 0.5, 0.25)
    want = R.slope(z, 0.5, 0.25, NODATA)
    np.testing.assert_array_equal(got, want)
    assert set(np.unique(got[~np.isnan(got)])) <= {0.0, 12.0, 16.0, 20.0}
    ring = np.ones(shape, bool)
    ring[1:-1, 1:-1] = False
    assert np.isnan(got[ring]).all() and (rows < 3 or not np.isnan(got[1:-1, 1:-1]).all())
    if shape == (2, 9):
        assert np.isnan(got).all()


@pytest.mark.parametrize("shape", SLOPE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_slope_is_within_one_ulp_on_any_surface(lib, shape, dtype):
    rng = np.random.RandomState(shape[0] + 31 * shape[1])
    z = (rng.randn(*shape) * 10.0 + 400.0).astype(dtype)
    z[rng.rand(*shape) < 0.03] = NODATA
    if shape[0] > 10:
        z[7, 3] = np.nan
    got = _slope(lib, z, 0.7, 0.3)
    want = R.slope(z, 0.7, 0.3, NODATA)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    if ok.any():
        ulps = np.abs(got[ok] - want[ok]) / np.spacing(want[ok])
        print(f"{shape} {dtype.__name__}: worst difference {ulps.max():.2f} ulp, {int((ulps > 0).sum())} of {ok.sum()} differ")
        assert (ulps <= 1.0).all()
    # every NaN is the one quiet NaN
    assert (got[np.isnan(got)].view(np.int64) == 0x7FF8000000000000).all()


def test_the_front_end_slope_in_degrees_and_as_a_tangent():
    from resdepth_amd.evaluation import dsm_slope
    y, x = np.mgrid[0:20, 0:30]
    z = (2.0 * x + 0.0 * y).astype(np.float32)
    t = dsm_slope(z, 2.0, degrees=False)
    assert t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (20, 30)
    assert (t[1:-1, 1:-1] == 1.0).all() and bool(torch.isnan(t[0]).all())
    d = dsm_slope(torch.from_numpy(z).to(DEV), (2.0, 2.0))
    assert float((d[1:-1, 1:-1] - 45.0).abs().max()) < 1e-12 and bool(torch.isnan(d[:, 0]).all())
    steep = dsm_slope(z, (1.0, 0.5), degrees=False)              # (gsd_y, gsd_x): the run along x is 0.5
    assert (steep[1:-1, 1:-1] == 4.0).all()
    z[5, 5] = -9999
    assert bool(torch.isnan(dsm_slope(z, 2.0)[4:7, 4:7]).all()) and not bool(torch.isnan(dsm_slope(z, 2.0, nodata=None)[5, 5]))
    with pytest.raises(ValueError):
        dsm_slope(z, 0.0)
    with pytest.raises(ValueError):
        dsm_slope(z[0], 1.0)


# ---- rd_bin_classes and evaluate_binned --------------------------------------------------------------------------------------
def _edges(n_bins, rng):
    """n_bins + 1 increasing multiples of 0.25 (exact as f32 too)"""
    return np.cumsum(rng.randint(1, 5, n_bins + 1)).astype(np.float64) / 4.0 - 3.0


@pytest.mark.parametrize("n_bins", [1, 6, 7, 24])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_bins_are_the_searchsorted_restatement(lib, n_bins, dtype):
    rng = np.random.RandomState(n_bins)
    n = 2777
    for ends in ("inf", "finite"):
        e = _edges(n_bins, rng)
        if ends == "inf":
            e[0], e[-1] = -np.inf, np.inf
        fin = e[np.isfinite(e)]
        lo, hi = (fin[0], fin[-1]) if len(fin) else (0.0, 0.0)
        by = (rng.randn(n) * (hi - lo + 2.0) + 0.5 * (lo + hi)).astype(dtype)
        by[:len(fin)] = fin                                       # values sitting exactly on an edge
        by[-5:] = [np.nan, np.inf, -np.inf, -0.0, 0.0]
        cls = rng.randint(0, 64, n).astype(np.uint8)
        groups = -(-n_bins // 6)
        out = torch.full((groups, n), 0xEE, dtype=torch.uint8, device=DEV)
        bd, cd = torch.from_numpy(by).to(DEV), torch.from_numpy(cls).to(DEV)
        with torch.cuda.device(DEV):
            rc = lib.rd_bin_classes(bd.data_ptr(), int(dtype == np.float64), cd.data_ptr(), n, (C.c_double * (n_bins + 1))(*e),
                                    n_bins, out.data_ptr(), _stream())
        assert rc == 0, lib.rd_last_error_string()
        want = R.bin_classes(by, cls, e)
        np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=f"{n_bins} bins, {ends} ends")
        # a value on edge k opens bin k; the last edge closes the last bin and belongs to none
        on_edge = R.bin_index(by[:len(fin)], e).tolist()
        if ends == "inf":
            assert on_edge == list(range(1, n_bins)) and (R.bin_index(by[:-5], e) >= 0).all()
            assert R.bin_index(by[-5:], e).tolist()[:3] == [-1, -1, 0]
        else:
            assert on_edge == list(range(n_bins)) + [-1] and (R.bin_index(by, e) < 0).sum() > 3


def _dsms(rng, shape):
    """gt, initial and refined DSMs whose residuals are multiples of 2^-10, with nodata in each"""
    gt = rng.randint(0, 2 ** 18, size=shape) / 1024.0 + 400.0
    init = gt + _residuals(rng, shape) / 64.0
    pred = gt + _residuals(rng, shape) / 256.0
    for a in (gt, init, pred):
        a[rng.rand(*shape) < 0.02] = NODATA
    return pred, init, gt


def _stats_rows(st):
    """a statistics dict of evaluate_binned -> its 8 (+ 6 truncated) numbers"""
    row = [st[k] for k in RC.KEYS]
    if st["truncation"]:
        row += [st["truncated"][k] for k in RC.TKEYS]
    return np.array(row, np.float64)


def test_binned_statistics_match_the_restatement():
    from resdepth_amd.evaluation import evaluate_binned
    rng = np.random.RandomState(21)
    shape = (61, 83)
    pred, init, gt = _dsms(rng, shape)
    by = rng.rand(*shape).astype(np.float32) * 10.0
    by[rng.rand(*shape) < 0.05] = np.nan
    by[0, :7] = [0.0, 1.0, 2.5, 4.0, 9.0, 10.0, -1.0]
    edges = [0.0, 1.0, 2.5, 4.0, 4.5, 6.0, 7.0, 9.0, 10.0]       # 8 bins: two planes; 4 sets per bin: two calls for a plane
    thr = 8.0
    got = evaluate_binned(pred, init, gt, by, edges, nodata=NODATA, residual_threshold=thr)
    assert len(got) == 8 and [b.lo for b in got] == edges[:-1] and [b.hi for b in got] == edges[1:]
    rb, ra, classes = RC.classify(pred, init, gt, NODATA)
    vb, va = classes["all"]
    which = R.bin_index(by, edges).reshape(shape)
    for b, entry in enumerate(got):
        for name, r, valid in (("initial", rb, vb), ("refined", ra, va)):
            m = valid & (which == b)
            assert m.sum() > 20
            want = np.array(RC.stats_row(r, m, thr))
            have = _stats_rows(entry[name])
            np.testing.assert_allclose(have, want, rtol=1e-12, atol=1e-12, err_msg=f"bin {b} {name}")
            np.testing.assert_array_equal(have[RC_MEDIANS], want[RC_MEDIANS], err_msg=f"bin {b} {name} (medians)")
            assert entry[name].truncated.threshold == thr
    plain = evaluate_binned(torch.from_numpy(pred).to(DEV), init, gt, torch.from_numpy(by).to(DEV), edges, nodata=NODATA)
    for b in range(8):
        assert "truncated" not in plain[b].refined
        np.testing.assert_array_equal(_stats_rows(plain[b].refined), _stats_rows(got[b].refined)[:8])


RC_MEDIANS = [0, 1, 2, 5, 6, 7, 8, 11, 12, 13]                   # counts, extremes and every median, truncated ones included


def test_slope_bins_are_taken_on_the_stored_tangent_raster():
    """by="slope" with edges in degrees against the same call on dsm_slope's tangent raster with the converted edges: the bin
    decisions are taken on the stored raster, so every number agrees in every bit"""
    from resdepth_amd.evaluation import dsm_slope, evaluate_binned, evaluate_statistics
    rng = np.random.RandomState(33)
    shape = (130, 97)
    pred, init, gt = _dsms(rng, shape)
    gt = np.where(gt == NODATA, NODATA, 400.0 + rng.randn(*shape).cumsum(axis=1) * 0.2).astype(np.float32)
    deg = [0.0, 2.0, 5.0, 10.0, 15.0, 20.0, 30.0, 45.0, 60.0, 90.0]
    gsd = (0.5, 0.25)
    a = evaluate_binned(pred, init, gt, "slope", deg, gsd=gsd, nodata=NODATA, residual_threshold=5.0)
    tangent = dsm_slope(gt, gsd, NODATA, degrees=False)
    b = evaluate_binned(pred, init, gt, tangent, [math.tan(math.radians(e)) for e in deg], nodata=NODATA, residual_threshold=5.0)
    assert len(a) == len(b) == 9 and [x.lo for x in a] == deg[:-1]
    for x, y in zip(a, b):
        for name in ("initial", "refined"):
            np.testing.assert_array_equal(_stats_rows(x[name]).view(np.int64), _stats_rows(y[name]).view(np.int64))
    assert sum(x.refined.count_total for x in a) > 0.5 * gt.size
    # over all of [-inf, +inf) the bins hold exactly the valid pixels with a finite covariate
    every = evaluate_binned(pred, init, gt, "slope", [-np.inf, 3.0, 12.0, 40.0, np.inf], gsd=gsd, nodata=NODATA)
    finite = torch.isfinite(tangent).cpu().numpy()
    assert not finite[0].any() and finite[1:-1, 1:-1].mean() > 0.5
    st = evaluate_statistics(pred, init, gt, mask_gt=finite.astype(np.uint8), nodata=NODATA)
    assert sum(x.refined.count_total for x in every) == st.after.all.count_total
    assert sum(x.initial.count_total for x in every) == st.before.all.count_total


# ---- error_map ---------------------------------------------------------------------------------------------------------------
def test_error_map_of_a_class_matches_the_restatement():
    from resdepth_amd.evaluation import error_map, evaluate_statistics
    rng = np.random.RandomState(44)
    shape = (64, 96)
    pred, init, gt = _dsms(rng, shape)
    building = np.zeros(shape, np.uint8)
    for _ in range(12):
        y, x = rng.randint(0, 56), rng.randint(0, 88)
        building[y:y + rng.randint(2, 9), x:x + rng.randint(2, 9)] = 1
    water = (rng.rand(*shape) < 0.1).astype(np.uint8)
    forest = (rng.rand(*shape) < 0.2).astype(np.uint8)
    gmask = (rng.rand(*shape) < 0.95).astype(np.uint8)
    kw = dict(mask_gt=gmask, mask_building=building, mask_water=water, mask_forest=forest, nodata=NODATA)
    rb, ra, classes = RC.classify(pred, init, gt, NODATA, gt_mask=(gmask, None), building=(building, None), water=(water, None),
                                  forest=(forest, None))
    st = evaluate_statistics(pred, init, gt, None, gmask, building, water, forest, nodata=NODATA)
    for klass in ("building", None, "terrain_nowater_noforest"):
        em = error_map(pred, gt, 16, initial=init, klass=klass, **kw)
        assert em["keys"] == R.KEYS and em.cell == (16, 16) and em.origin == (0, 0)
        assert em.refined.is_cuda and tuple(em.refined.shape) == tuple(em.initial.shape) == (4, 6, 8)
        vb, va = classes[klass or "all"]
        _assert_cells(em.refined.cpu().numpy(), R.cell_stats(ra, va.astype(np.uint8), 16, 16, 1), f"{klass} refined")
        _assert_cells(em.initial.cpu().numpy(), R.cell_stats(rb, vb.astype(np.uint8), 16, 16, 1), f"{klass} initial")
        assert float(em.refined[..., 0].sum()) == st.after[klass or "all"].count_total
        assert float(em.initial[..., 0].sum()) == st.before[klass or "all"].count_total
    host = error_map(pred, gt, (16, 32), klass="building", residual_threshold=2.0, **kw)
    assert "initial" not in host and tuple(host.refined.shape) == (4, 3, 8)
    dev = error_map(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), (16, 32), klass="building",
                    residual_threshold=2.0, **kw)
    assert torch.equal(host.refined.view(torch.int64), dev.refined.view(torch.int64))
    _assert_cells(host.refined.cpu().numpy(), R.cell_stats(ra, classes["building"][1].astype(np.uint8), 16, 32, 1, 2.0), "thr")
    with pytest.raises(ValueError):
        error_map(pred, gt, 16, klass="building", nodata=NODATA)    # no building mask: the class is not defined
    with pytest.raises(ValueError):
        error_map(pred, gt[:10], 16)
