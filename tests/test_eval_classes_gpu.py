"""Class-partitioned evaluation on the GPU (-m gpu): resdepth_amd.evaluation.evaluate_performance / evaluate_statistics /
dilate_mask / get_statistics_masked against fixtures from the reference's evaluate_performance (g18) and, at city
scale, against the numpy restatement (tests/eval_classes_ref.py; its dilation is pure numpy)."""
import io
import logging

import numpy as np
import pytest
import torch

import eval_classes_ref as R
from conftest import load_npz

pytestmark = pytest.mark.gpu
MEDIAN_COLS = [5, 6, 11, 12]            # absolute median, median, truncated absolute median, truncated median


class _Band:
    def __init__(self, values, nodata):
        self.values, self.nodata = values, nodata

    def ReadAsArray(self):
        return self.values.copy()

    def GetNoDataValue(self):
        return self.nodata


class FakeDataset:
    """the dataset interface evaluate_performance reads (GDAL's names)"""

    def __init__(self, values, nodata, gsd=1.0):
        self.band, self.gsd = _Band(values, nodata), gsd

    def GetRasterBand(self, i):
        return self.band

    def ReadAsArray(self):
        return self.band.ReadAsArray()

    def GetGeoTransform(self):
        return (0.0, self.gsd, 0.0, 0.0, 0.0, -self.gsd)


def rows_of(stats, classes, thr):
    """evaluate_statistics result -> the reference's call order (per class: before, after), 14 columns"""
    out = []
    for c in classes:
        for when in ("before", "after"):
            st = stats[when][c]
            row = [st[k] for k in R.KEYS]
            row += [st["truncated"][k] for k in R.TKEYS] if thr else [np.nan] * len(R.TKEYS)
            out.append(row)
    return np.array(out)


def area_defn(area):
    return None if area is None else {"x_extent": [(int(a[0]), int(a[1])) for a in area],
                                      "y_extent": [(int(a[2]), int(a[3])) for a in area]}


def assert_rows(got, want, what):
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12, equal_nan=True, err_msg=what)
    cols = [c for c in MEDIAN_COLS if c < want.shape[1]]
    np.testing.assert_array_equal(got[:, cols], want[:, cols], err_msg=what + " (medians)")


def test_g18_parity_with_reference_evaluate_performance():
    from resdepth_amd.evaluation import evaluate_performance, evaluate_statistics
    g = load_npz("g18_eval.npz")
    nodata, gsd = float(g["nodata"]), float(g["gsd"])
    for i in range(int(g["n"])):
        p = f"c{i}/"
        args, thr = R.golden_case(g, i)
        classes = [str(c) for c in g[p + "classes"]]
        masks = {k: (FakeDataset(g[p + "mask_" + k], 255.0) if p + "mask_" + k in g else None) for k in "gbwf"}
        text = io.StringIO()
        log = logging.getLogger(f"test_g18_{i}")
        log.setLevel(logging.INFO)
        log.propagate = False
        log.handlers[:] = [logging.StreamHandler(text)]
        root = logging.getLogger("test_g18_root")
        res = evaluate_performance(g[p + "pred"], FakeDataset(g[p + "init"], nodata, gsd), FakeDataset(g[p + "gt"], nodata, gsd),
                                   root, area_defn(g.get(p + "area")), masks["g"], masks["b"], masks["w"], masks["f"],
                                   log, thr)
        assert list(res.keys()) == classes
        assert text.getvalue() == str(g[p + "report"]), f"case {i}: report differs"
        n = g[p + "pred"].size
        for c in classes:
            assert isinstance(res[c], np.ma.MaskedArray) and res[c].shape == g[p + "pred"].shape
            want = np.unpackbits(g[p + "rmask_" + c])[:n].reshape(res[c].shape).astype(bool)
            np.testing.assert_array_equal(np.ma.getmaskarray(res[c]), want, err_msg=f"case {i} class {c}")
            assert getattr(res, c) is res[c]
        got_all = res.all.compressed()
        assert got_all.dtype == np.float64
        np.testing.assert_array_equal(got_all.view(np.uint64), g[p + "rall"].view(np.uint64))
        tup = {k: (g[p + "mask_" + k], 255.0) if p + "mask_" + k in g else None for k in "gbwf"}
        st = evaluate_statistics(g[p + "pred"], g[p + "init"], g[p + "gt"], area_defn(g.get(p + "area")), tup["g"],
                                 tup["b"], tup["w"], tup["f"], thr, nodata=nodata)
        assert st.after.all.MAE == st["after"]["all"]["MAE"]
        assert_rows(rows_of(st, classes, thr), g[p + "calls"], f"case {i}")


@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (257, 129), (2048, 3001)])
def test_dilation_bit_exact(shape):
    from resdepth_amd.evaluation import dilate_mask
    rng = np.random.RandomState(shape[0] * 7 + shape[1])
    border = np.zeros(shape, bool)
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = True
    for name, m in (("sparse", rng.rand(*shape) < 0.005), ("dense", rng.rand(*shape) < 0.6), ("border", border)):
        for k in (1, 2, 3, 4):
            got = dilate_mask(m.astype(np.uint8), k)
            assert isinstance(got, np.ndarray) and got.dtype == bool
            np.testing.assert_array_equal(got, R.dilate(m, k), err_msg=f"{shape} {name} k={k}")
    t = torch.from_numpy(rng.rand(*shape) < 0.01).cuda()
    got = dilate_mask(t, 11)                             # > 8: chained launches
    assert torch.is_tensor(got) and got.is_cuda
    np.testing.assert_array_equal(got.cpu().numpy(), R.dilate(t.cpu().numpy(), 11))


def city(seed=4, h=4096, w=3000, gt_f64=False):
    rng = np.random.RandomState(seed)
    gt = rng.randn(h, w) * 5 + 400
    gt = gt if gt_f64 else gt.astype(np.float32)
    init = (gt + rng.standard_t(3, size=(h, w)) * 1.1).astype(np.float32)
    pred = gt.astype(np.float64) + rng.laplace(size=(h, w)) * 0.6
    gt[rng.rand(h, w) < 0.01] = -9999.0
    init[rng.rand(h, w) < 0.01] = -9999.0
    pred[rng.rand(h, w) < 0.01] = -9999.0

    def mask(p, nd):
        m = (rng.rand(h, w) < p).astype(np.uint8)
        m[rng.rand(h, w) < nd] = 255
        return m, 255.0

    masks = dict(gt_mask=mask(0.92, 0.01), building=mask(0.04, 0.01), water=mask(0.1, 0.0), forest=mask(0.15, 0.01))
    area = np.array([[0, w - 1, 0, 999], [100, 2100, 1500, 3100], [2000, 2999, 2900, h - 1]])
    return dict(pred=pred, init=init, gt=gt, nodata=-9999.0, area=area, **masks)


def test_city_scale_all_sets_against_restatement_and_single_set_kernel():
    from resdepth_amd.evaluation import evaluate_statistics, get_statistics
    d = city()
    thr = 2.5
    st = evaluate_statistics(d["pred"], d["init"], d["gt"], area_defn(d["area"]), d["gt_mask"], d["building"], d["water"],
                             d["forest"], thr, nodata=d["nodata"])
    rb, ra, classes = R.classify(**d)
    assert list(classes) == R.CLASSES
    got = rows_of(st, R.CLASSES, thr)
    assert got.shape == (10, 14)                         # 20 statistics sets
    assert_rows(got, R.evaluate_calls(rb, ra, classes, thr), "city")
    for c in R.CLASSES:                                  # the same sets through the single-set kernel, explicit masks
        for when, raster, v in (("before", d["init"], 0), ("after", d["pred"], 1)):
            ref = get_statistics(raster, d["gt"], d["nodata"], classes[c][v], thr)
            mine = st[when][c]
            np.testing.assert_allclose([mine[k] for k in R.KEYS], [ref[k] for k in R.KEYS], rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose([mine.truncated[k] for k in R.TKEYS], [ref["truncated"][k] for k in R.TKEYS],
                                       rtol=1e-12, atol=1e-12)


def test_f64_ground_truth_is_not_rounded():
    from resdepth_amd.evaluation import evaluate_statistics
    d = city(seed=9, h=700, w=500, gt_f64=True)
    assert d["gt"].dtype == np.float64 and np.any(d["gt"].astype(np.float32).astype(np.float64) != d["gt"])
    d["init"] = d["init"].astype(np.float64) + 1e-9           # f64 initial DSM as well
    d["init"][d["init"] == -9999.0 + 1e-9] = -9999.0
    st = evaluate_statistics(d["pred"], d["init"], d["gt"], area_defn(d["area"]), d["gt_mask"], d["building"], None,
                             d["forest"], 1.5, nodata=d["nodata"])
    rb, ra, classes = R.classify(**dict(d, water=None))
    names = [c for c in R.CLASSES if c in classes]
    assert_rows(rows_of(st, names, 1.5), R.evaluate_calls(rb, ra, classes, 1.5), "f64 gt")


def _bits(st):
    return {w: {c: {k: (v if not isinstance(v, dict) else tuple(sorted(v.items()))) for k, v in s.items()}
                for c, s in st[w].items()} for w in st}


def test_device_tensor_inputs_and_determinism():
    from resdepth_amd.evaluation import evaluate_statistics
    d = city(seed=2, h=1000, w=900)
    args = (area_defn(d["area"]),)
    host = evaluate_statistics(d["pred"], d["init"], d["gt"], *args, d["gt_mask"], d["building"], d["water"], d["forest"],
                               2.0, nodata=d["nodata"])
    again = evaluate_statistics(d["pred"], d["init"], d["gt"], *args, d["gt_mask"], d["building"], d["water"],
                                d["forest"], 2.0, nodata=d["nodata"])
    assert repr(_bits(host)) == repr(_bits(again))
    cu = lambda x: torch.from_numpy(x).cuda()                                  # noqa: E731
    dev = evaluate_statistics(cu(d["pred"]), cu(d["init"]), cu(d["gt"]), *args, (cu(d["gt_mask"][0]), 255.0),
                              (cu(d["building"][0]), 255.0), (cu(d["water"][0]), 255.0), (cu(d["forest"][0]), 255.0),
                              2.0, nodata=d["nodata"])
    assert repr(_bits(host)) == repr(_bits(dev))


def test_empty_class_and_pooled_statistics():
    from resdepth_amd.evaluation import evaluate_statistics, get_statistics_masked
    d = city(seed=3, h=300, w=200)
    no_buildings = (np.zeros_like(d["building"][0]), 255.0)
    st = evaluate_statistics(d["pred"], d["init"], d["gt"], None, d["gt_mask"], no_buildings, None, None, 1.0,
                             nodata=d["nodata"])
    for when in ("before", "after"):
        b = st[when]["building"]
        assert b.count_total == 0 and np.isnan(b.median) and np.isnan(b.MAE) and np.isnan(b.diff_max)
        assert b.truncated.count_total == 0 and np.isnan(b.truncated.NMAD)
        assert st[when]["terrain"].count_total > 0
    rng = np.random.RandomState(8)
    parts = []
    for n in (1234, 777, 4001):                         # three pairs' residuals, ragged
        r = rng.laplace(size=n) * 0.8
        parts.append(np.ma.masked_array(r, mask=rng.rand(n) < 0.1))
    pooled = np.ma.concatenate(parts)
    got = get_statistics_masked(pooled, 1.2)
    want = R.stats_row(np.ma.getdata(pooled), ~np.ma.getmaskarray(pooled), 1.2)
    mine = [got[k] for k in R.KEYS] + [got.truncated[k] for k in R.TKEYS]
    assert_rows(np.array([mine]), np.array([want]), "pooled")
    assert got.truncation and got.truncated.threshold == 1.2
    plain = get_statistics_masked(torch.from_numpy(parts[0].compressed()).cuda())
    assert not plain.truncation and "truncated" not in plain
    want = R.stats_row(parts[0].compressed(), np.ones(parts[0].count(), bool))
    assert_rows(np.array([[plain[k] for k in R.KEYS]]), np.array([want[:8]]), "tensor")
