"""rd_residual_dist_sets and rd_residual_dist_pooled at the C ABI against the fp64 oracle of tests/dist_ref.py: BIT equality of
every count, quantile and share, of the two forms with each other, and of two calls.

Sizes are those of tests/test_stats_forms_gpu.py (one moments block and one more; one histogram round of 512 threads x 8 values
and one more; one value past the 1024-block grid cap) and the data is that file's kind: Laplace, a tenth duplicated, with +0.0,
-0.0 and a repeated -1.25 planted.  Levels 0, 0.5, 0.68, 0.9, 0.95, 1 in both modes; tolerances 0 (the planted zeros), 1.25
(equal to planted members: the <= is tested) and 1e300."""
import ctypes as C

import numpy as np
import pytest
import torch

import dist_ref
from test_stats_forms_gpu import PAD, SIZES, _source

pytestmark = pytest.mark.gpu
LEVELS = (0.0, 0.5, 0.68, 0.9, 0.95, 1.0)
TAUS = (0.0, 1.25, 1e300)
# (need bits, threshold or none): half the pixels; a truncated set; the other source's kind; nobody (class bytes are < 16)
SETS = [(1, -1.0), (1 | 8, 1.0), (2, -1.0), (64, -1.0)]


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _arr(ctype, values):
    return (ctype * max(len(values), 1))(*values)


def _dist_sets(src0, src1, cls, sets, levels, modes, taus, set_src=None):
    """-> [len(sets), 1 + n_q + n_t] as int64 bit patterns"""
    from resdepth_amd import _lib as L
    lib = L.load()
    n, ns, nq, nt = cls.numel(), len(sets), len(levels), len(taus)
    out = torch.full((ns, 1 + nq + nt), -7.0, dtype=torch.float64, device=cls.device)
    ws = torch.empty(lib.rd_residual_dist_sets_ws_bytes(n, ns, nq, nt), dtype=torch.uint8, device=cls.device)
    with torch.cuda.device(cls.device):
        L.check(lib.rd_residual_dist_sets(L.ptr(src0), L.ptr(src1), L.ptr(cls), n, _arr(C.c_int, set_src or [0] * ns),
                                          _arr(C.c_int, [s[0] for s in sets]), _arr(C.c_double, [s[1] for s in sets]), ns,
                                          _arr(C.c_double, levels), _arr(C.c_int, modes), nq, _arr(C.c_double, taus), nt,
                                          L.ptr(out), ws.data_ptr(), ws.numel(), L.stream_ptr()), "residual_dist_sets")
    return out.cpu().numpy().view(np.int64)


def _dist_pooled(planes, stride, n_planes, p0, p1, cls, valid, sets, levels, modes, taus):
    from resdepth_amd import _lib as L
    lib = L.load()
    n, ns, nq, nt = cls.numel(), len(sets), len(levels), len(taus)
    out = torch.full((ns, 1 + nq + nt), -7.0, dtype=torch.float64, device=cls.device)
    ws = torch.empty(lib.rd_residual_dist_pooled_ws_bytes(n, ns, nq, nt), dtype=torch.uint8, device=cls.device)
    with torch.cuda.device(cls.device):
        L.check(lib.rd_residual_dist_pooled(L.ptr(planes), stride, n_planes, p0, p1, L.ptr(cls), L.ptr(valid), n,
                                            _arr(C.c_int, [s[0] for s in sets]), _arr(C.c_double, [s[1] for s in sets]), ns,
                                            _arr(C.c_double, levels), _arr(C.c_int, modes), nq, _arr(C.c_double, taus), nt,
                                            L.ptr(out), ws.data_ptr(), ws.numel(), L.stream_ptr()), "residual_dist_pooled")
    return out.cpu().numpy().view(np.int64)


def _want(r, cls, sets, levels, modes, taus):
    """the oracle's rows for sets over one stream of (value, class) pairs, as bit patterns"""
    return np.stack([dist_ref.row(dist_ref.members(r, cls, need, thr), levels, modes, taus) for need, thr in sets]).view(np.int64)


def _same_bits(got, want, what):
    # NaNs of an empty set: any quiet NaN is a NaN; everything else bit for bit
    g, w = got.view(np.float64), want.view(np.float64)
    np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=what)
    np.testing.assert_array_equal(np.where(np.isnan(g), 0, got), np.where(np.isnan(w), 0, want), err_msg=what)


@pytest.mark.parametrize("n", SIZES)
def test_both_forms_give_the_oracles_bits(n):
    dev = _dev()
    rng = np.random.RandomState(n % 9973)
    a, b = _source(rng, n), _source(rng, n)
    cls_h = rng.randint(0, 16, size=n).astype(np.uint8)
    buf = np.full(2 * n + PAD, 1e300)                  # the padding between the planes must never be read
    buf[:n], buf[n + PAD:] = a, b
    cls = torch.from_numpy(cls_h).to(dev)
    ta, tb, planes = (torch.from_numpy(x).to(dev) for x in (a, b, buf))
    ns = len(SETS)
    for mode in (0, 1):
        modes = [mode] * len(LEVELS)
        for p, (t_src, h_src) in enumerate(((ta, a), (tb, b))):
            want = _want(h_src, cls_h, SETS, LEVELS, modes, TAUS)
            got = _dist_sets(ta, tb, cls, SETS, LEVELS, modes, TAUS, set_src=[p] * ns)
            _same_bits(got, want, f"sets form, source {p}, mode {mode}")
            pooled = _dist_pooled(planes, n + PAD, 2, p, p + 1, cls, None, SETS, LEVELS, modes, TAUS)
            np.testing.assert_array_equal(pooled, got, err_msg=f"plane {p} against source {p}, mode {mode}")
    np.testing.assert_array_equal(_dist_sets(ta, tb, cls, SETS, LEVELS, modes, TAUS, set_src=[1] * ns), got,
                                  err_msg="two calls, the same bits")
    g = got.view(np.float64)
    assert g[0, 0] == float((cls_h & 1).sum()) and g[3, 0] == 0.0 and np.isnan(g[3, 1:]).all()
    if n >= 255:
        assert g[0, -1] == 1.0 and 0.0 < g[0, -2] < 1.0                      # tau = 1e300 holds everyone, 1.25 not


def test_a_rank_that_is_an_integer_and_one_that_is_not():
    """q = 0.9: with c = 11 members (c - 1) * q is 9 exactly and Q = v_(9); with c = 12 it is 9.9 and Q interpolates."""
    dev = _dev()
    rng = np.random.RandomState(5)
    r = rng.laplace(size=23)
    cls_h = np.array([1] * 11 + [2] * 12, dtype=np.uint8)
    sets = [(1, -1.0), (2, -1.0)]
    got = _dist_sets(torch.from_numpy(r).to(dev), None, torch.from_numpy(cls_h).to(dev), sets, [0.9, 0.9], [0, 1], [])
    want = _want(r, cls_h, sets, [0.9, 0.9], [0, 1], [])
    np.testing.assert_array_equal(got, want)
    g = got.view(np.float64)
    assert g[0, 0] == 11 and g[0, 1] == np.sort(r[:11])[9] and g[0, 2] == np.sort(np.abs(r[:11]))[9]
    v = np.sort(r[11:])
    assert g[1, 0] == 12 and v[9] < g[1, 1] < v[10]


def test_twenty_sets_times_eight_quantiles_and_shares_alone():
    """160 selectors in eight groups of twenty (and a group that is not full: 20 x 3 + a remainder), then tolerances only: the
    counting pass alone."""
    dev = _dev()
    n = 4097
    rng = np.random.RandomState(11)
    a, b = _source(rng, n), _source(rng, n)
    cls_h = rng.randint(0, 64, size=n).astype(np.uint8)
    cls, ta, tb = (torch.from_numpy(x).to(dev) for x in (cls_h, a, b))
    sets = [(need, thr) for need in (0, 1, 2, 4, 8, 16, 32, 3, 12, 48) for thr in (-1.0, 0.75)]
    src = [k & 1 for k in range(20)]
    levels, modes = [0.0, 0.5, 0.68, 0.9, 0.95, 1.0, 0.05, 0.9], [1, 1, 1, 1, 1, 1, 0, 0]
    taus = [0.0, 0.25, 0.5, 0.75, 1.0, 1.25, 2.0, 1e300]

    def want(lv, md, tt):
        return np.stack([dist_ref.row(dist_ref.members(b if s else a, cls_h, need, thr), lv, md, tt)
                         for s, (need, thr) in zip(src, sets)]).view(np.int64)
    _same_bits(_dist_sets(ta, tb, cls, sets, levels, modes, taus, set_src=src), want(levels, modes, taus), "20 x 8 x 8")
    _same_bits(_dist_sets(ta, tb, cls, sets[:7], levels[:3], modes[:3], taus[:1], set_src=src[:7]),
               want(levels[:3], modes[:3], taus[:1])[:7], "7 x 3 x 1: two groups, the second with one selector")
    _same_bits(_dist_sets(ta, tb, cls, sets, [], [], taus, set_src=src), want([], [], taus), "shares alone")
    _same_bits(_dist_sets(ta, tb, cls, sets, levels, modes, [], set_src=src), want(levels, modes, []), "quantiles alone")


@pytest.mark.parametrize("n", [257, 4097])
@pytest.mark.parametrize("n_planes", [2, 3])
def test_pooled_planes_under_a_validity_word(n, n_planes):
    """The pool's members come from every plane of the range whose bit of the pixel's validity word is set; the padding of
    1e300 between the planes is nobody's member: it would be the largest value and within no finite tolerance."""
    dev = _dev()
    rng = np.random.RandomState(n + n_planes)
    stride = n + PAD
    buf = np.full(n_planes * stride, 1e300)
    srcs = [_source(rng, n) for _ in range(n_planes)]
    for p, a in enumerate(srcs):
        buf[p * stride:p * stride + n] = a
    cls_h = rng.randint(0, 16, size=n).astype(np.uint8)
    valid_h = rng.randint(0, 1 << n_planes, size=n).astype(np.int16)              # drops pixels per plane
    planes, cls, valid = (torch.from_numpy(x).to(dev) for x in (buf, cls_h, valid_h))
    levels, modes = list(LEVELS) + [0.9, 0.5], [1] * 6 + [0, 0]
    for p0, p1 in [(0, n_planes), (n_planes - 1, n_planes), (0, 2)]:
        ok = [((valid_h >> p) & 1) == 1 for p in range(p0, p1)]
        r = np.concatenate([srcs[p][m] for p, m in zip(range(p0, p1), ok)])
        c = np.concatenate([cls_h[m] for m in ok])
        got = _dist_pooled(planes, stride, n_planes, p0, p1, cls, valid, SETS, levels, modes, TAUS)
        _same_bits(got, _want(r, c, SETS, levels, modes, TAUS), f"planes [{p0}, {p1})")
        assert got.view(np.float64)[0, 6] < 1e299                                 # level 1 of |r|: the largest member
        np.testing.assert_array_equal(_dist_pooled(planes, stride, n_planes, p0, p1, cls, valid, SETS, levels, modes, TAUS), got)
    # no validity word: every plane counts, as an all-ones word does
    ones = torch.full((n,), -1, dtype=torch.int16, device=dev)
    full = _dist_pooled(planes, stride, n_planes, 0, n_planes, cls, None, SETS, levels, modes, TAUS)
    np.testing.assert_array_equal(_dist_pooled(planes, stride, n_planes, 0, n_planes, cls, ones, SETS, levels, modes, TAUS), full)
    _same_bits(full, _want(np.concatenate(srcs), np.tile(cls_h, n_planes), SETS, levels, modes, TAUS), "no validity word")


def test_the_median_level_agrees_with_the_engines_median_within_the_roundings():
    """q = 0.5 and the eight numbers' median: 0.5 * (a + b) against a + 0.5 * (b - a), at most 16 * 2^-53 * max(|a|, |b|) apart."""
    from resdepth_amd import _lib as L
    lib = L.load()
    dev = _dev()
    n = 4096
    rng = np.random.RandomState(2)
    a = _source(rng, n)
    cls = torch.ones(n, dtype=torch.uint8, device=dev)
    ta = torch.from_numpy(a).to(dev)
    got = _dist_sets(ta, None, cls, [(1, -1.0)], [0.5, 0.5], [0, 1], []).view(np.float64)[0]
    out = torch.empty((1, 8), dtype=torch.float64, device=dev)
    ws = torch.empty(lib.rd_residual_stats_sets_ws_bytes(n, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.rd_residual_stats_sets(L.ptr(ta), None, L.ptr(cls), n, _arr(C.c_int, [0]), _arr(C.c_int, [1]),
                                           _arr(C.c_double, [-1.0]), 1, L.ptr(out), ws.data_ptr(), ws.numel(), L.stream_ptr()),
                "residual_stats_sets")
    eight = out.cpu().numpy()[0]
    v = np.sort(a)
    m = max(abs(v[n // 2 - 1]), abs(v[n // 2]))
    assert got[0] == n and abs(got[1] - eight[6]) <= 16 * 2.0 ** -53 * m and abs(got[2] - eight[5]) <= 16 * 2.0 ** -53 * np.abs(a).max()
