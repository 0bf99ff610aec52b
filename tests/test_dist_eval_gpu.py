"""The quantile / share options of resdepth_amd.evaluation on a 96 x 130 raster with ground-truth, building, water and forest
masks and two area rectangles: every value against the oracle of tests/dist_ref.py applied to the class partition of
tests/eval_classes_ref.py, bit for bit; and the same calls without the options against what they returned before the options
existed: the same keys, the same bits."""
import io
import logging

import numpy as np
import pytest

import dist_ref
import eval_classes_ref as R
from test_eval_classes_gpu import area_defn
from test_eval_pairs_gpu import NODATA, _planes_case, small_city

pytestmark = pytest.mark.gpu
H, W = 96, 130
THR = 1.5
WITHIN = (1.0, 2.0)
OLD_KEYS = {"truncation", "truncated", "count_total", "diff_max", "diff_min", "MAE", "RMSE", "absolute_median", "median", "NMAD"}
OLD_TRUNCATED = {"count_total", "threshold", "MAE", "RMSE", "absolute_median", "median", "NMAD"}
NEW_KEYS = {"abs_quantile", "quantile", "within"}


def _bits(x):
    return np.array([x], dtype=np.float64).view(np.int64)[0]


def _same(a, b, what):
    assert (np.isnan(a) and np.isnan(b)) or _bits(a) == _bits(b), (what, a, b)


def _check_set(st, r, abs_q, q, within, what):
    """one statistics dict against the oracle over its members r (the truncated sub-dict: over the members within THR)"""
    for d, m, tag in ((st, r, ""), (st["truncated"], r[np.abs(r) <= THR], " truncated")):
        assert d["count_total"] == len(m), what + tag
        assert set(d["abs_quantile"]) == set(abs_q) and set(d["within"]) == set(within), what + tag
        for lv in abs_q:
            _same(d["abs_quantile"][lv], dist_ref.quantile(m, lv, 1), f"{what}{tag} LE{100 * lv:g}")
        for lv in q:
            _same(d["quantile"][lv], dist_ref.quantile(m, lv, 0), f"{what}{tag} q={lv}")
        for tau in within:
            _same(d["within"][tau], dist_ref.share(m, tau), f"{what}{tag} within {tau}")
        assert ("quantile" in d) == bool(q)


def _strip(st):
    """a statistics dict without the new keys"""
    out = {k: v for k, v in st.items() if k not in NEW_KEYS}
    if "truncated" in out:
        out["truncated"] = {k: v for k, v in out["truncated"].items() if k not in NEW_KEYS}
    return out


def _equal_in_keys_and_bits(a, b, what):
    assert set(a) == set(b), (what, set(a) ^ set(b))
    for k in a:
        if isinstance(a[k], dict):
            _equal_in_keys_and_bits(a[k], b[k], f"{what}.{k}")
        elif isinstance(a[k], float):
            _same(a[k], b[k], f"{what}.{k}")
        else:
            assert a[k] == b[k], (what, k)


@pytest.fixture(scope="module")
def case():
    d = small_city(9, H, W)
    rb, ra, classes = R.classify(**d)
    assert list(classes) == R.CLASSES
    return d, rb, ra, classes


def _args(d):
    return (d["init"], d["gt"], area_defn(d["area"]), d["gt_mask"], d["building"], d["water"], d["forest"], THR)


def test_evaluate_statistics_per_class_and_side(case):
    from resdepth_amd import evaluation as E
    d, rb, ra, classes = case
    st = E.evaluate_statistics(d["pred"], *_args(d), nodata=NODATA, abs_quantiles=E.LE, within=WITHIN)
    for c in R.CLASSES:
        vb, va = classes[c]
        assert va.sum() > 20, c
        _check_set(st.before[c], rb[vb], E.LE, (), WITHIN, f"before {c}")
        _check_set(st.after[c], ra[va], E.LE, (), WITHIN, f"after {c}")
    assert 0.0 < st.after.all.within[1.0] < st.after.all.within[2.0] <= 1.0
    assert st.after.all.abs_quantile[0.68] < st.after.all.abs_quantile[0.9] < st.after.all.abs_quantile[0.95]
    assert st.after.all.truncated.within[2.0] == 1.0                      # everyone left is within THR = 1.5
    # signed quantiles too, and only the keys that were asked for
    sq = E.evaluate_statistics(d["pred"], *_args(d), nodata=NODATA, quantiles=(0.05, 0.5, 0.95))
    va = classes["building"][1]
    for lv in (0.05, 0.5, 0.95):
        _same(sq.after.building.quantile[lv], dist_ref.quantile(ra[va], lv, 0), f"q={lv}")
    assert "abs_quantile" not in sq.after.building and "within" not in sq.after.building.truncated
    # the eight numbers are those of the call without options, and that call returns what it always did
    plain = E.evaluate_statistics(d["pred"], *_args(d), nodata=NODATA)
    for when in ("before", "after"):
        for c in R.CLASSES:
            assert set(plain[when][c]) == OLD_KEYS and set(plain[when][c]["truncated"]) == OLD_TRUNCATED
            _equal_in_keys_and_bits(dict(plain[when][c]), _strip(st[when][c]), f"{when} {c}")
            _equal_in_keys_and_bits(dict(plain[when][c]), _strip(sq[when][c]), f"{when} {c}")


def test_no_options_make_exactly_the_old_library_calls(case, monkeypatch):
    from resdepth_amd import _lib, evaluation as E
    d = case[0]
    calls = []
    real = _lib.load()

    class Spy:
        def __getattr__(self, name):
            if name.startswith("rd_residual") or name.startswith("rd_eval"):
                calls.append(name)
            return getattr(real, name)
    monkeypatch.setattr(E, "load", lambda: Spy())
    E.evaluate_statistics(d["pred"], *_args(d), nodata=NODATA)
    old = ["rd_eval_classify", "rd_residual_stats_sets_ws_bytes", "rd_residual_stats_sets"]
    assert calls == old
    del calls[:]
    E.evaluate_statistics(d["pred"], *_args(d), nodata=NODATA, within=(1.0,))
    assert calls == old + ["rd_residual_dist_sets_ws_bytes", "rd_residual_dist_sets"]         # one more call, the same sets


def _pairs_call(E, d, **opts):
    p, pairs = _planes_case(31, H, W, 3)
    return E.evaluate_pairs_statistics(pairs, *_args(p), fused=pairs[0], nodata=NODATA, **opts)


def _binned_call(E, d, **opts):
    """the 61 x 83 case of test_errmap_gpu.test_binned_statistics_match_the_restatement: eight bins under a threshold"""
    from test_errmap_gpu import _dsms
    rng = np.random.RandomState(21)
    pred, init, gt = _dsms(rng, (61, 83))
    by = rng.rand(61, 83).astype(np.float32) * 10.0
    by[rng.rand(61, 83) < 0.05] = np.nan
    edges = [0.0, 1.0, 2.5, 4.0, 4.5, 6.0, 7.0, 9.0, 10.0]
    return E.evaluate_binned(pred, init, gt, by, edges, nodata=NODATA, residual_threshold=8.0)


OPTS = dict(abs_quantiles=(0.68, 0.90, 0.95), within=WITHIN)
POOLED = [(0, 1), (1, 2), (2, 3), (0, 3)]                         # planes p0 .. p1 - 1 of a call: the three pairs, then their pool
# every launching entry point a call makes, in order; a call that takes sets with their number (and the planes it draws from):
# five classes x (full, truncated) = 10 sets a pair or pool, 20 for the initial DSM and the fused surface
CALLS = {
    "pairs": (_pairs_call, {}, ["rd_dilate_mask", "rd_eval_classify_planes"]
              + [("rd_residual_stats_pooled", p0, p1, 10) for p0, p1 in POOLED] + [("rd_residual_stats_sets", 20)]),
    "pairs_options": (_pairs_call, OPTS, ["rd_dilate_mask", "rd_eval_classify_planes"]
                      + [(name, p0, p1, 10) for p0, p1 in POOLED for name in ("rd_residual_stats_pooled", "rd_residual_dist_pooled")]
                      + [("rd_residual_stats_sets", 20), ("rd_residual_dist_sets", 20)]),
    "masked": (lambda E, d, **o: E.get_statistics_masked(d["pred"] - d["gt"], THR, **o), {}, [("rd_residual_stats_sets", 2)]),
    "masked_options": (lambda E, d, **o: E.get_statistics_masked(d["pred"] - d["gt"], THR, **o), OPTS,
                       [("rd_residual_stats_sets", 2), ("rd_residual_dist_sets", 2)]),
    "get_statistics": (lambda E, d, **o: E.get_statistics(d["pred"], d["gt"], NODATA, None, THR, **o), dict(within=WITHIN),
                       ["rd_residual_stats", "rd_residual_stats", ("rd_residual_dist_sets", 2)]),
    "error_map": (lambda E, d, **o: E.error_map(d["pred"], d["gt"], 16, initial=d["init"], mask_gt=d["gt_mask"],
                                                mask_building=d["building"], nodata=NODATA), {},
                  ["rd_dilate_mask", "rd_eval_classify", "rd_cell_stats", "rd_cell_stats"]),
    # 8 bins x (initial, refined) x (full, truncated): 24 sets on the first plane of six bins -- a call of 20 and one of 4 --
    # and 8 on the second
    "binned": (_binned_call, {}, ["rd_eval_classify", "rd_bin_classes", ("rd_residual_stats_sets", 20),
                                  ("rd_residual_stats_sets", 4), ("rd_residual_stats_sets", 8)]),
}


@pytest.mark.parametrize("path", list(CALLS))
def test_every_path_makes_exactly_its_library_calls(case, monkeypatch, path):
    """the spy of the test above on every other path of the front end, recording at the call"""
    from resdepth_amd import _lib, evaluation as E
    run, opts, want = CALLS[path]
    calls = []
    real = _lib.load()

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if not name.startswith("rd_") or name.endswith("_ws_bytes"):
                return fn

            def recorded(*a):
                if name in ("rd_residual_stats_sets", "rd_residual_dist_sets"):
                    calls.append((name, a[7]))                    # (src0, src1, cls, n, set_src, set_need, set_thr, n_sets, ...
                elif name in ("rd_residual_stats_pooled", "rd_residual_dist_pooled"):
                    calls.append((name, a[3], a[4], a[10]))       # (src, stride, n_planes, p0, p1, cls, valid, n, need, thr, n_sets
                else:
                    calls.append(name)
                return fn(*a)
            return recorded
    monkeypatch.setattr(E, "load", lambda: Spy())
    run(E, case[0], **opts)
    assert calls == want


def test_evaluate_pairs_statistics_per_pair_pool_and_fused():
    from resdepth_amd import evaluation as E
    d, pairs = _planes_case(31, H, W, 3)
    fused = np.where((pairs[0] == NODATA) | (pairs[2] == NODATA), NODATA, 0.5 * (pairs[0] + pairs[2]))
    args = (d["init"], d["gt"], area_defn(d["area"]), d["gt_mask"], d["building"], d["water"], d["forest"], THR)
    opts = dict(abs_quantiles=E.LE, quantiles=(0.05,), within=WITHIN)
    st = E.evaluate_pairs_statistics(pairs, *args, fused=fused, nodata=NODATA, **opts)
    kw = {k: d[k] for k in ("init", "gt", "nodata", "area", "gt_mask", "building", "water", "forest")}
    per_pair = [R.classify(pred=pairs[p], **kw) for p in range(3)]
    for c in R.CLASSES:
        pool = []
        for p, (rb, ra, classes) in enumerate(per_pair):
            m = ra[classes[c][1]]
            pool.append(m)
            _check_set(st.pairs[p][c], m, E.LE, (0.05,), WITHIN, f"pair {p} {c}")
        assert len(pool[1]) == 0 and np.isnan(st.pairs[1][c].abs_quantile[0.9]) and np.isnan(st.pairs[1][c].within[1.0])
        _check_set(st.pooled[c], np.concatenate(pool), E.LE, (0.05,), WITHIN, f"pool {c}")
        _check_set(st.before[c], per_pair[0][0][per_pair[0][2][c][0]], E.LE, (0.05,), WITHIN, f"before {c}")
        rb, rf, classes = R.classify(pred=fused, **kw)
        _check_set(st.fused[c], rf[classes[c][1]], E.LE, (0.05,), WITHIN, f"fused {c}")
    plain = E.evaluate_pairs_statistics(pairs, *args, fused=fused, nodata=NODATA)
    for c in R.CLASSES:
        for what, a, b in [("pooled", plain.pooled[c], st.pooled[c]), ("before", plain.before[c], st.before[c]),
                           ("fused", plain.fused[c], st.fused[c])] + [(f"pair {p}", plain.pairs[p][c], st.pairs[p][c]) for p in range(3)]:
            assert set(a) == OLD_KEYS and set(a["truncated"]) == OLD_TRUNCATED
            _equal_in_keys_and_bits(dict(a), _strip(b), f"{what} {c}")


def test_get_statistics_and_get_statistics_masked(case):
    from resdepth_amd import evaluation as E
    d, rb, ra, classes = case
    va = classes["all"][1]
    masked = np.ma.MaskedArray(ra, mask=~va)
    opts = dict(abs_quantiles=E.LE, quantiles=(0.05, 0.95), within=WITHIN)
    st = E.get_statistics_masked(masked, THR, **opts)
    _check_set(st, ra[va], E.LE, (0.05, 0.95), WITHIN, "get_statistics_masked")
    plain = E.get_statistics_masked(masked, THR)
    assert set(plain) == OLD_KEYS and set(plain["truncated"]) == OLD_TRUNCATED
    _equal_in_keys_and_bits(dict(plain), _strip(st), "get_statistics_masked")
    no_thr = E.get_statistics_masked(masked, abs_quantiles=(0.9,))
    assert "truncated" not in no_thr and set(no_thr) == (OLD_KEYS - {"truncated"}) | {"abs_quantile"}
    _same(no_thr["abs_quantile"][0.9], dist_ref.quantile(ra[va], 0.9, 1), "no threshold")
    # an empty selection: count 0, NaN
    empty = E.get_statistics_masked(np.ma.MaskedArray(ra, mask=True), within=(1.0,))
    assert empty["count_total"] == 0 and np.isnan(empty["within"][1.0])

    # get_statistics: the plain residual of two rasters under a validity mask
    gm = R.mask_of(*d["gt_mask"])[0]
    g64 = d["gt"].astype(np.float64)
    ok = (d["pred"] != NODATA) & (g64 != NODATA) & gm
    r = (d["pred"] - g64)[ok]
    gs = E.get_statistics(d["pred"], d["gt"], NODATA, gm, THR, **opts)
    _check_set(gs, r, E.LE, (0.05, 0.95), WITHIN, "get_statistics")
    plain = E.get_statistics(d["pred"], d["gt"], NODATA, gm, THR)
    assert set(plain) == OLD_KEYS and set(plain["truncated"]) == OLD_TRUNCATED
    _equal_in_keys_and_bits(plain, _strip(gs), "get_statistics")


def test_the_reports_carry_the_lines(case):
    from resdepth_amd import evaluation as E
    from test_eval_classes_gpu import FakeDataset
    d = case[0]
    root = logging.getLogger("dist_eval_root")
    root.addHandler(logging.NullHandler())
    text = {}
    for name, opts in (("plain", {}), ("le", dict(abs_quantiles=E.LE, within=(1.0,)))):
        buf = io.StringIO()
        lg = logging.getLogger("dist_eval_" + name)
        lg.setLevel(logging.INFO)
        lg.propagate = False
        h = logging.StreamHandler(buf)
        lg.addHandler(h)
        E.evaluate_performance(d["pred"], FakeDataset(d["init"], NODATA), FakeDataset(d["gt"], NODATA), root, area_defn(d["area"]),
                               d["gt_mask"], d["building"], d["water"], d["forest"], lg, THR, **opts)
        lg.removeHandler(h)
        text[name] = buf.getvalue()
    assert "LE90" not in text["plain"] and "Share of pixels" not in text["plain"]
    blocks = 2 * len(R.CLASSES)
    assert text["le"].count("Linear error LE90 (|residual| quantile) [m]:") == blocks
    assert text["le"].count("Truncated linear error LE90 (|residual| quantile) [m]:") == blocks
    assert text["le"].count("hare of pixels within 1.00 m [%]:") == 2 * blocks
    kept = [ln for ln in text["le"].splitlines() if "LE" not in ln and "hare of pixels" not in ln]
    assert [ln for ln in kept if ln.strip()] == [ln for ln in text["plain"].splitlines() if ln.strip()]
