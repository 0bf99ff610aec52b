"""The exact Euclidean distance transform on the GPU (include/resdepth_hip_edt.h, resdepth_amd/morphology.py), bit for bit against
the numpy oracles of tests/edt_ref.py: d2 AND idx, so the tie rule of the header is tested on every case.

Shapes: the degenerate ones; every side of the column pass's band height B = RD_EDT_BAND_ROWS (B - 1, B, B + 1, 2B + 1, and
3B + 1 with an empty band between two occupied ones); every side of the row pass's 256 threads and 64-lane waves; a 300 x 1000
raster at three densities and with one set pixel in each corner (the longest searches, the clamps at both row ends); 4 x 16384,
the LDS maximum.  A reference is computed once per mask (lru_cache) and never modified."""
import functools
import math

import numpy as np
import pytest
import torch

import edt_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32 = torch.int32


@pytest.fixture(scope="module")
def lib():
    from resdepth_amd import _lib
    assert (_lib.EDT_NONE, _lib.EDT_MAX_ROWS, _lib.EDT_MAX_COLS, _lib.EDT_BAND_ROWS) == (R.NONE, R.MAX_ROWS, R.MAX_COLS, R.BAND_ROWS)
    return _lib.load()


def edt(lib, mask, invert=0, with_idx=True, d2=None):
    """mask: uint8 device tensor [rows, cols] (any storage offset) -> (d2, idx) int32 device tensors"""
    rows, cols = mask.shape
    nb = lib.rd_edt_ws_bytes(rows, cols)
    assert nb == -(-rows // R.BAND_ROWS) * cols * 8
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    d2 = torch.full((rows, cols), -7, dtype=I32, device=DEV) if d2 is None else d2
    idx = torch.full((rows, cols), -7, dtype=I32, device=DEV) if with_idx else None
    rc = lib.rd_edt_sq(mask.data_ptr(), invert, rows, cols, d2.data_ptr(), idx.data_ptr() if with_idx else None, ws.data_ptr(), nb,
                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.rd_last_error_string()
    torch.cuda.synchronize()
    return d2, idx


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)       # a copy: the cached references are read-only


def same(lib, mask, want, invert=0):
    d2, idx = edt(lib, dev(mask), invert)
    got_d2, got_idx = d2.cpu().numpy(), idx.cpu().numpy()
    bad = np.argwhere(got_d2 != want[0])
    assert bad.size == 0, f"d2 differs at {bad[:3].tolist()} ({len(bad)} pixels)"
    bad = np.argwhere(got_idx != want[1])
    assert bad.size == 0, f"idx differs at {bad[:3].tolist()} ({len(bad)} pixels): the distances agree, the tie rule does not"


@functools.lru_cache(maxsize=None)
def big(density):
    """the 300 x 1000 mask of a density and its reference, computed once"""
    m = R.random_mask(300, 1000, density, seed=int(density * 1000))
    want = R.separable(m)
    for a in (m,) + want:
        a.setflags(write=False)
    return m, want


# ---- shapes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (3, 5)], ids=lambda s: "%dx%d" % s)
def test_degenerate_shapes(lib, shape):
    for seed, density in enumerate((0.3, 0.7, 1.0, 0.0)):
        m = R.random_mask(*shape, density, seed)
        want = R.brute(m)
        assert R.attains(m, *want)
        same(lib, m, want)
        same(lib, m, R.brute(m, invert=True), invert=1)


B = R.BAND_ROWS


@pytest.mark.parametrize("where", ["first", "last", "none", "first_and_last"])
@pytest.mark.parametrize("rows", [B - 1, B, B + 1, 2 * B + 1, 3 * B + 1])
def test_band_edges_of_the_column_pass(lib, rows, where):
    cols, bands = 70, -(-rows // B)
    m = np.zeros((rows, cols), np.uint8)
    sparse = R.random_mask(rows, cols, 0.02, rows)
    sparse[[0, min(B, rows) - 1, (bands - 1) * B, rows - 1], ::7] = 1          # the first and the last row of both bands
    if "first" in where:
        m[:B] = sparse[:B]
    if "last" in where:
        m[(bands - 1) * B:] = sparse[(bands - 1) * B:]
    same(lib, m, R.separable(m))


@pytest.mark.parametrize("cols", [63, 64, 65, 255, 256, 257, 1000])
def test_row_pass_edges(lib, cols):
    m = R.random_mask(5, cols, 0.03, cols)
    same(lib, m, R.separable(m))
    m[:, 1:-1] = 0                                     # only the two ends of the rows: every search runs its full length
    same(lib, m, R.separable(m))


@pytest.mark.parametrize("density", [0.5, 0.01, 0.999])
def test_densities(lib, density):
    m, want = big(density)
    same(lib, m, want)


@pytest.mark.parametrize("corner", [(0, 0), (0, 999), (299, 0), (299, 999)], ids=lambda c: "%d_%d" % c)
def test_a_single_pixel_in_a_corner(lib, corner):
    m = np.zeros((300, 1000), np.uint8)
    m[corner] = 1
    same(lib, m, R.one_pixel(300, 1000, *corner))


def test_no_feature_and_all_features(lib):
    rows, cols = 131, 70
    d2, idx = edt(lib, torch.zeros((rows, cols), dtype=torch.uint8, device=DEV))
    assert bool((d2 == R.NONE).all()) and bool((idx == -1).all())
    d2, idx = edt(lib, torch.ones((rows, cols), dtype=torch.uint8, device=DEV))
    assert bool((d2 == 0).all()) and torch.equal(idx.reshape(-1), torch.arange(rows * cols, dtype=I32, device=DEV))


def test_invert_is_the_complemented_mask(lib):
    m, _ = big(0.5)
    a = edt(lib, dev(m), invert=1)
    b = edt(lib, dev(1 - m), invert=0)
    c = edt(lib, dev(m), invert=5)                     # any non-zero flag inverts
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def test_any_non_zero_byte_is_set(lib):
    m, want = big(0.01)
    values = np.array([1, 2, 255, 128], np.uint8)[np.arange(m.size).reshape(m.shape) % 4]
    same(lib, m * values, want)


def test_misaligned_pointers(lib):
    m, want = big(0.01)
    rows, cols = m.shape
    raw = torch.zeros(m.size + 1, dtype=torch.uint8, device=DEV)
    raw[1:] = dev(m).reshape(-1)
    mask = raw[1:].view(rows, cols)
    store = torch.empty(m.size + 1, dtype=I32, device=DEV)
    d2 = store[1:].view(rows, cols)
    assert mask.data_ptr() % 2 == 1 and d2.data_ptr() % 8 == 4
    d2, idx = edt(lib, mask, d2=d2)
    assert np.array_equal(d2.cpu().numpy(), want[0]) and np.array_equal(idx.cpu().numpy(), want[1])


def test_a_null_idx_changes_nothing_else(lib):
    m, want = big(0.01)
    d2, none = edt(lib, dev(m), with_idx=False)
    assert none is None and np.array_equal(d2.cpu().numpy(), want[0])
    d2, _ = edt(lib, torch.zeros((5, 70), dtype=torch.uint8, device=DEV), with_idx=False)
    assert bool((d2 == R.NONE).all())


def test_the_limits(lib):
    rows, cols = 4, R.MAX_COLS
    m = np.zeros((rows, cols), np.uint8)
    m[2, 0] = 1
    same(lib, m, R.one_pixel(rows, cols, 2, 0))        # the LDS maximum and the longest search
    stream = torch.cuda.current_stream().cuda_stream
    for shape in ((4, R.MAX_COLS + 1), (R.MAX_ROWS + 1, 4)):
        n = shape[0] * shape[1]
        mask = torch.zeros(n, dtype=torch.uint8, device=DEV)
        d2, idx = torch.full((n,), -7, dtype=I32, device=DEV), torch.full((n,), -7, dtype=I32, device=DEV)
        ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
        assert lib.rd_edt_ws_bytes(*shape) == 0
        assert lib.rd_edt_sq(mask.data_ptr(), 0, shape[0], shape[1], d2.data_ptr(), idx.data_ptr(), ws.data_ptr(), 1 << 20, stream) == 1
        assert lib.rd_last_error_string()
        torch.cuda.synchronize()
        assert bool((d2 == -7).all()) and bool((idx == -7).all()) and not bool(ws.any())


def test_two_calls_give_the_same_bits(lib):
    m, _ = big(0.01)
    mask = dev(m)
    a, b = edt(lib, mask), edt(lib, mask)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- rd_fill_nearest -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_d2", [0, 1, 25, R.NONE - 1])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_fill_nearest(lib, dtype, max_d2):
    n = 70 * 33 + 1
    rng = np.random.default_rng(n)
    z = (rng.standard_normal(n) * 50.0 + 400.0).astype(dtype)
    bits = z.view(np.uint32 if dtype == np.float32 else np.uint64)
    payload = (0x7FC12345, 0xFFC00001) if dtype == np.float32 else (0x7FF8000000ABCDEF, 0xFFF8000000000001)
    bits[::11], bits[5::13] = payload[0], payload[1]   # NaNs with payloads, among the sources and among the targets
    d2 = rng.choice(np.array([0, 1, 2, 25, 26, 1000, R.NONE], np.int32), n)
    idx = rng.integers(-1, n + 5, n).astype(np.int32)
    idx[:4] = [-1, n, n + 4, n - 1]
    d2[:4] = 1
    want = R.fill_nearest(z, d2, idx, max_d2)
    out = torch.full((n,), 7.0, dtype=torch.float32 if dtype == np.float32 else torch.float64, device=DEV)
    tz, td, ti = dev(z), dev(d2), dev(idx)
    rc = lib.rd_fill_nearest(tz.data_ptr(), int(dtype == np.float64), td.data_ptr(), ti.data_ptr(), n, max_d2, out.data_ptr(),
                             torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.rd_last_error_string()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got.view(bits.dtype), want.view(bits.dtype))
    if max_d2 == 0:
        assert np.array_equal(got.view(bits.dtype), bits)
    else:
        assert (got.view(bits.dtype) != bits).any()


# ---- the front end ---------------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    return np.abs(a.view(np.int64) - b.view(np.int64))


def test_distance_transform_in_metres_and_indices():
    from resdepth_amd import distance_transform
    m, want = big(0.01)
    sq = distance_transform(m, squared=True)
    assert sq.dtype == I32 and sq.is_cuda and np.array_equal(sq.cpu().numpy(), want[0])
    for gsd in (1.0, 0.25, (0.25, 0.25)):              # powers of two: the scaling is exact, the bar is the square root's
        g = gsd if isinstance(gsd, float) else gsd[0]
        d = distance_transform(torch.from_numpy(m).to(DEV), gsd)
        assert d.dtype == torch.float64 and d.is_cuda
        got, ref = d.cpu().numpy(), np.sqrt(want[0].astype(np.float64)) * g
        # resdepth_hip_errmap.h's bar for the device's fp64 square root: within one unit in the last place, exact on squares
        print(f"gsd {g}: {int((_ulps(got, ref) > 0).sum())} of {got.size} values one ulp away")
        assert _ulps(got, ref).max() <= 1
        root = np.rint(np.sqrt(want[0].astype(np.float64))).astype(np.int64)
        square = root * root == want[0]
        assert square.sum() > 1000 and np.array_equal(got[square], root[square] * g)
    d3 = distance_transform(m, 0.3).cpu().numpy()
    assert np.array_equal(d3, distance_transform(m, 1.0).cpu().numpy() * 0.3)
    d, where = distance_transform(m, return_indices=True)
    assert where.dtype == torch.int64 and tuple(where.shape) == (300, 1000, 2)
    y, x = np.divmod(want[1].astype(np.int64), 1000)
    assert np.array_equal(where.cpu().numpy(), np.stack((y, x), axis=-1))
    d, where = distance_transform(np.zeros((5, 9)), return_indices=True)
    assert bool(torch.isinf(d).all()) and bool((d > 0).all()) and bool((where == -1).all())
    inv = distance_transform(m, invert=True, squared=True)
    assert np.array_equal(inv.cpu().numpy(), R.separable(m, invert=True)[0])


def test_edge_distance_sign_magnitude_and_infinities():
    from resdepth_amd import edge_distance
    m = np.zeros((64, 96), np.uint8)
    m[10:30, 20:50] = 1
    m[40:44, 5:9] = 1
    m[50:, 90:] = 1                                    # touches the border
    d = edge_distance(m, 0.5).cpu().numpy()
    out2, in2 = R.brute(m)[0], R.brute(m, invert=True)[0]
    want = np.where(m != 0, -np.sqrt(in2.astype(np.float64)), np.sqrt(out2.astype(np.float64))) * 0.5
    assert np.array_equal(np.sign(d), np.where(m != 0, -1.0, 1.0)) and np.abs(d).min() == 0.5
    assert _ulps(d, want).max() <= 1
    assert d[20, 35] == -5.0 and d[20, 10] == 5.0      # ten pixels inside the first box's nearest wall, ten outside
    assert bool((edge_distance(np.zeros((7, 9))) == math.inf).all()) and bool((edge_distance(np.ones((7, 9))) == -math.inf).all())


def test_buffer_mask_is_the_cross_dilation_up_to_two_and_a_disc_beyond():
    from resdepth_amd import buffer_mask
    from resdepth_amd.evaluation import dilate_mask
    m, _ = big(0.01)
    t = torch.from_numpy(m).to(DEV)
    for k in (1, 2):
        assert torch.equal(buffer_mask(t, k), dilate_mask(t, k))
        assert torch.equal(buffer_mask(t, 0.5 * k, 0.5), dilate_mask(t, k))      # the same radius in metres
    b3 = buffer_mask(t, 3)
    assert b3.dtype == torch.bool and not torch.equal(b3, dilate_mask(t, 3))
    d2 = R.separable(m)[0]
    assert np.array_equal(b3.cpu().numpy(), d2 <= 9)
    assert np.array_equal(buffer_mask(m, 2.3, 0.5).cpu().numpy(), d2 <= R.threshold(2.3, 0.5))
    assert np.array_equal(buffer_mask(m, 0).cpu().numpy(), m != 0)
    solid = np.zeros((64, 96), np.uint8)
    solid[5:40, 10:70] = 1
    solid[50:, :30] = 1
    solid[20, 30] = 0                                  # a one-pixel hole erodes its neighbourhood
    comp = R.brute(solid, invert=True)[0]
    for r in (1, 2.5, 4):
        got = buffer_mask(solid, -r).cpu().numpy()
        assert np.array_equal(got, comp > R.threshold(r, 1.0)) and 0 < got.sum() < solid.sum()
    assert bool(buffer_mask(np.ones((9, 9)), -100).all()) and not bool(buffer_mask(np.zeros((9, 9)), 100).any())


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_fill_voids(dtype):
    from resdepth_amd import fill_voids
    rng = np.random.default_rng(5)
    z = (rng.standard_normal((48, 70)) * 20.0 + 400.0).astype(dtype)
    clean = z.copy()
    z[10, 10] = -9999.0                                # isolated
    z[0:3, 60:] = -9999.0                              # touches the border
    z[20:40, 20:45] = -9999.0                          # larger than max_distance
    z[30, 5] = np.nan
    kind = torch.float32 if dtype == np.float32 else torch.float64
    bits = np.uint32 if dtype == np.float32 else np.uint64
    for cap in (None, 3.0, 1.0, 0.0):
        for gsd in (1.0, 0.5):
            want, want_mask = R.fill_voids(z, -9999.0, cap, gsd)
            got, mask = fill_voids(z, -9999, max_distance=cap, gsd=gsd, return_mask=True)
            assert got.dtype == kind and got.is_cuda and mask.dtype == torch.bool
            assert np.array_equal(got.cpu().numpy().view(bits), want.view(bits)), (cap, gsd)
            assert np.array_equal(mask.cpu().numpy(), want_mask)
    full = fill_voids(z).cpu().numpy()
    assert not (full == -9999.0).any() and not np.isnan(full).any() and full[10, 10] == z[9, 10]      # |dx| = 0 first, then the upper one
    capped = fill_voids(z, max_distance=3.0).cpu().numpy()
    assert capped[30, 32] == -9999.0 and capped[21, 21] != -9999.0
    assert np.array_equal(fill_voids(clean).cpu().numpy().view(bits), clean.view(bits))
    void = np.full((9, 12), -9999.0, dtype)
    void[3, 4] = np.nan
    assert np.array_equal(fill_voids(void).cpu().numpy().view(bits), void.view(bits))
    only_nan = fill_voids(z, nodata=None).cpu().numpy()
    assert only_nan[10, 10] == -9999.0 and only_nan[30, 5] == z[29, 5]


def test_distance_binned_evaluation_end_to_end():
    from resdepth_amd import edge_distance, evaluate_binned
    rng = np.random.default_rng(9)
    shape, gsd = (64, 96), 0.5
    gt = (400.0 + rng.standard_normal(shape)).astype(np.float32)
    init = (gt + rng.standard_normal(shape)).astype(np.float32)
    pred = (gt + 0.3 * rng.standard_normal(shape)).astype(np.float32)
    m = np.zeros(shape, np.uint8)
    m[12:36, 20:60] = 1
    m[44:52, 70:90] = 1
    edges = [-math.inf, -2.0, 0.0, 2.0, 5.0, math.inf]
    got = evaluate_binned(pred, init, gt, edge_distance(m, gsd), edges)
    out2, in2 = R.brute(m)[0], R.brute(m, invert=True)[0]
    d = np.where(m != 0, -np.sqrt(in2.astype(np.float64)), np.sqrt(out2.astype(np.float64))) * gsd
    # an edge is met exactly only by a perfect square (2 m = sqrt(16) px), where the device's square root is exact
    counts = [int(((d >= lo) & (d < hi)).sum()) for lo, hi in zip(edges[:-1], edges[1:])]
    assert [int(b.refined.count_total) for b in got] == counts == [int(b.initial.count_total) for b in got]
    assert sum(counts) == gt.size and min(counts) > 0
