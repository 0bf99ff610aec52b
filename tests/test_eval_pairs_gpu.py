"""Scoring every pair plane of a sweep, and the pool of all pairs, on the GPU (-m gpu): resdepth_amd.evaluation.
evaluate_pairs_statistics / evaluate_pairs_performance and the entry points of include/resdepth_hip_eval.h against the fixture
from the reference (g22) and the numpy restatement (tests/eval_pairs_ref.py).  Bars: tests/test_eval_classes_gpu.py assert_rows
(rtol = atol = 1e-12 on count, max, min, MAE, RMSE; medians exactly equal)."""
import ctypes as C
import io
import logging

import numpy as np
import pytest
import torch

import eval_classes_ref as R
import eval_pairs_ref as PR
from conftest import load_npz
from test_eval_classes_gpu import FakeDataset, assert_rows, city

pytestmark = pytest.mark.gpu
NODATA = -9999.0


def _check(st, want, thr, what, fused=False):
    names = want["classes"]
    assert list(st.before.keys()) == names and list(st.pooled.keys()) == names
    assert_rows(PR.rows_of(st.before, names, thr), want["before"], what + " before")
    assert len(st.pairs) == len(want["pairs"])
    for p, by_class in enumerate(st.pairs):
        assert_rows(PR.rows_of(by_class, names, thr), want["pairs"][p], what + f" pair {p}")
    assert_rows(PR.rows_of(st.pooled, names, thr), want["pooled"], what + " pooled")
    assert ("fused" in st) == fused
    if fused:
        assert_rows(PR.rows_of(st.fused, names, thr), want["fused"], what + " fused")


def _logger(name):
    text = io.StringIO()
    log = logging.getLogger(name)
    log.setLevel(logging.INFO)
    log.propagate = False
    log.handlers[:] = [logging.StreamHandler(text)]
    return log, text


# ---- 1. the reference's own numbers -------------------------------------------------------------------------------------------
def test_g22_parity_with_the_reference_per_pair_and_pooled():
    from resdepth_amd.evaluation import evaluate_pairs_performance, evaluate_pairs_statistics, print_statistics, AttrDict
    g = load_npz("g22_pairs_eval.npz")
    kw = PR.g22_case(g)
    thr, nodata, gsd = kw["thr"], kw["nodata"], float(g["gsd"])
    names = [str(c) for c in g["classes"]]
    area = PR.area_defn(kw["area"])
    st = evaluate_pairs_statistics(kw["pairs"], kw["init"], kw["gt"], area, kw["gt_mask"], kw["building"], kw["water"],
                                   kw["forest"], thr, nodata=nodata)
    n_planes = kw["pairs"].shape[0]
    for p in range(n_planes):
        got = np.stack([PR.rows_of(st.before, names, thr), PR.rows_of(st.pairs[p], names, thr)], axis=1).reshape(-1, 14)
        assert_rows(got, g[f"p{p}/calls"], f"g22 pair {p}")
    assert_rows(PR.rows_of(st.pooled, names, thr), g["pooled/calls"], "g22 pooled")
    assert st.pooled.all.MAE == st["pooled"]["all"]["MAE"] and st.pairs[1].terrain.truncated.threshold == thr
    # the reports: per pair the reference's text; pooled: the headings of test.py:326-357 around print_statistics
    logs = [_logger(f"test_g22_pair_{p}") for p in range(n_planes)]
    pooled_log, pooled_text = _logger("test_g22_pooled")
    masks = {k: FakeDataset(kw[m][0], 255.0) for k, m in (("g", "gt_mask"), ("b", "building"), ("w", "water"), ("f", "forest"))}
    res = evaluate_pairs_performance(kw["pairs"], FakeDataset(kw["init"], nodata, gsd), FakeDataset(kw["gt"], nodata, gsd),
                                     logging.getLogger("test_g22_root"), area, masks["g"], masks["b"], masks["w"], masks["f"],
                                     [lg for lg, _ in logs], pooled_log, thr)
    for p, (_, text) in enumerate(logs):
        assert text.getvalue() == str(g[f"p{p}/report"]), f"pair {p}: report differs"
    assert repr(res) == repr(st)
    want_log, want_text = _logger("test_g22_pooled_want")
    heads = ["OVERALL", "BUILDING PIXELS", "TERRAIN PIXELS", "TERRAIN PIXELS WITHOUT WATER", "TERRAIN PIXELS WITHOUT WATER/FOREST"]
    bodies = []
    for c, row in zip(names, g["pooled/calls"]):
        want_text.seek(0)
        want_text.truncate()
        rec = AttrDict(zip(R.KEYS, row[:8]), truncation=True, truncated=AttrDict(zip(R.TKEYS, row[8:]), threshold=thr))
        print_statistics(rec, want_log)
        bodies.append(want_text.getvalue())
    want = "\nPerformance Evaluation: Statistics over all predictions\n" + "-" * 55 + "\n\n"
    want += "Truncation threshold:\t\t\t{:.2f} m\n\n".format(thr)
    for head, body in zip(heads, bodies):
        title = f"STATISTICS, {head}: REFINED DSM"
        want += "\n" + title + "\n" + "-" * len(title) + "\n\n" + body
    assert pooled_text.getvalue() == want


# ---- 2. one plane is today's evaluation -----------------------------------------------------------------------------------------
def _classify_planes(lib, planes, stride, n_planes, init, gt, masks, rects, rows, cols, res, extra=None, r_extra=None,
                     r_before=None):
    from resdepth_amd._lib import check, ptr, stream_ptr
    n = rows * cols
    cls = torch.empty(n, dtype=torch.uint8, device="cuda")
    valid = torch.empty(n, dtype=torch.int16, device="cuda")
    rect_a = None if rects is None else (C.c_int * (4 * len(rects)))(*[v for r in rects for v in r])
    check(lib.rd_eval_classify_planes(ptr(planes), stride, n_planes, ptr(extra), ptr(init), int(init.dtype == torch.float64),
                                      ptr(gt), int(gt.dtype == torch.float64), *[ptr(m) for m in masks], rect_a,
                                      -1 if rects is None else len(rects), rows, cols, NODATA, ptr(r_before), ptr(res),
                                      ptr(r_extra), ptr(cls), ptr(valid), stream_ptr()), "eval_classify_planes")
    return cls, valid


def _pooled(lib, src, stride, n_planes, p0, p1, cls, valid, n, need, thr):
    from resdepth_amd._lib import check, ptr, stream_ptr
    ns = len(need)
    out = torch.empty((ns, 8), dtype=torch.float64, device="cuda")
    ws = torch.empty(lib.rd_residual_stats_pooled_ws_bytes(n, ns), dtype=torch.uint8, device="cuda")
    check(lib.rd_residual_stats_pooled(ptr(src), stride, n_planes, p0, p1, ptr(cls), ptr(valid), n, (C.c_int * ns)(*need),
                                       (C.c_double * ns)(*thr), ns, ptr(out), ptr(ws), ws.numel(), stream_ptr()), "pooled")
    return out.cpu().numpy()


def _device_case(d):
    """a city() dict -> device tensors the C ABI takes: (pred f64, init, gt, [gt_mask, dilated building, building nodata,
    water, forest] as 0/1 bytes, rects)"""
    from resdepth_amd.evaluation import _mask_pair, _dilate_u8, _rects
    dev = torch.device("cuda", torch.cuda.current_device())
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()                    # noqa: E731
    gm = _mask_pair(d["gt_mask"], dev)[0]
    b, bnod = _mask_pair(d["building"], dev)
    masks = [gm, _dilate_u8(b, 2), bnod, _mask_pair(d["water"], dev)[0], _mask_pair(d["forest"], dev)[0]]
    rows, cols = d["gt"].shape
    return cu(d["pred"]), cu(d["init"]), cu(d["gt"]), masks, _rects(PR.area_defn(d["area"]), rows, cols)


def small_city(seed, h, w):
    d = city(seed=seed, h=h, w=w)
    d["area"] = np.array([[0, w - 1, 0, h // 3], [w // 10, w - 1 - w // 10, h // 2, h - 1]])
    return d


def test_one_plane_equals_todays_evaluation():
    from resdepth_amd import _lib
    from resdepth_amd.evaluation import evaluate_pairs_statistics, evaluate_statistics
    d = small_city(5, 257, 129)
    args = (d["init"], d["gt"], PR.area_defn(d["area"]), d["gt_mask"], d["building"], d["water"], d["forest"], 2.0)
    one = evaluate_pairs_statistics(d["pred"][None], *args, nodata=NODATA)
    ref = evaluate_statistics(d["pred"], *args, nodata=NODATA)
    for got in (one.pairs[0], one.pooled):
        assert_rows(PR.rows_of(got, R.CLASSES, 2.0), PR.rows_of(ref.after, R.CLASSES, 2.0), "P = 1")
    assert_rows(PR.rows_of(one.before, R.CLASSES, 2.0), PR.rows_of(ref.before, R.CLASSES, 2.0), "P = 1 before")
    # the C ABI, bit for bit
    lib = _lib.load()
    pred, init, gt, masks, rects = _device_case(d)
    rows, cols = d["gt"].shape
    n = rows * cols
    rb, ra = torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda")
    cls0 = torch.empty(n, dtype=torch.uint8, device="cuda")
    rect_a = (C.c_int * (4 * len(rects)))(*[v for r in rects for v in r])
    _lib.check(lib.rd_eval_classify(_lib.ptr(pred), _lib.ptr(init), 0, _lib.ptr(gt), 0, *[_lib.ptr(m) for m in masks], rect_a,
                                    len(rects), rows, cols, NODATA, _lib.ptr(rb), _lib.ptr(ra), _lib.ptr(cls0),
                                    _lib.stream_ptr()), "eval_classify")
    res, rb1 = torch.empty_like(ra), torch.empty_like(rb)
    cls, valid = _classify_planes(lib, pred, n, 1, init, gt, masks, rects, rows, cols, res, r_before=rb1)
    assert torch.equal(res.view(torch.int64), ra.view(torch.int64)) and torch.equal(rb1.view(torch.int64), rb.view(torch.int64))
    assert int((cls & 2).max()) == 0 and int((valid.int() & ~1).abs().max()) == 0
    assert torch.equal(cls | ((valid & 1) << 1).to(torch.uint8), cls0)
    inplace = pred.clone()
    cls2, valid2 = _classify_planes(lib, inplace, n, 1, init, gt, masks, rects, rows, cols, inplace)
    assert torch.equal(inplace.reshape(-1).view(torch.int64), ra.view(torch.int64))
    assert torch.equal(cls2, cls) and torch.equal(valid2, valid)


# ---- 3. edge shapes of the histogram round (a block covers 512 x 8 pixels) -----------------------------------------------------
def _planes_case(seed, h, w, n_planes):
    """rasters with all four masks, two stripes and n_planes predictions whose nodata pixels differ; plane 1 (if any) is nodata
    everywhere"""
    rng = np.random.RandomState(seed)
    d = small_city(seed, h, w)
    g64 = np.where(d["gt"] == NODATA, 400.0, d["gt"]).astype(np.float64)
    pairs = np.empty((n_planes, h, w))
    for p in range(n_planes):
        pairs[p] = g64 + rng.laplace(size=(h, w)) * (0.4 + 0.1 * p) + 0.03 * p
        pairs[p][rng.rand(h, w) < 0.05 + 0.01 * p] = NODATA
    if n_planes > 1:
        pairs[1] = NODATA
    del d["pred"]
    return d, pairs


@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (64, 67), (257, 129)])
@pytest.mark.parametrize("n_planes", [1, 2, 3, 16])
def test_edge_shapes_against_the_restatement(shape, n_planes):
    from resdepth_amd.evaluation import evaluate_pairs_statistics
    h, w = shape
    d, pairs = _planes_case(100 * n_planes + h, h, w, n_planes)
    if n_planes > 2:
        assert (((pairs[0] == NODATA) != (pairs[2] == NODATA)).any()) or h * w == 1     # a pixel valid in some planes only
    thr = 1.5
    st = evaluate_pairs_statistics(pairs, d["init"], d["gt"], PR.area_defn(d["area"]), d["gt_mask"], d["building"], d["water"],
                                   d["forest"], thr, nodata=NODATA)
    want = PR.restate(pairs, d["init"], d["gt"], NODATA, d["area"], d["gt_mask"], d["building"], d["water"], d["forest"], thr)
    _check(st, want, thr, f"{shape} P={n_planes}")
    if n_planes > 1:                                     # the nodata plane's sets are empty, the pool is not (beyond 1 x 1)
        for c in R.CLASSES:
            e = st.pairs[1][c]
            assert e.count_total == 0 and np.isnan(e.median) and np.isnan(e.MAE) and e.truncated.count_total == 0
        if h * w > 1:
            assert st.pooled.all.count_total == sum(s.all.count_total for s in st.pairs) > 0


def test_even_pool_whose_middle_ranks_lie_in_different_planes_and_identical_planes():
    from resdepth_amd.evaluation import evaluate_pairs_statistics
    h, w = 64, 67
    rng = np.random.RandomState(3)
    gt = (rng.randn(h, w) * 5 + 400).astype(np.float32)
    init = gt + 1.0
    lo, hi = -2.0 + rng.rand(h, w), 1.0 + rng.rand(h, w)               # plane 0 below every value of plane 1
    pairs = np.stack([gt.astype(np.float64) + lo, gt.astype(np.float64) + hi])
    st = evaluate_pairs_statistics(pairs, init, gt, nodata=NODATA)
    r = pairs - gt.astype(np.float64)
    assert st.pooled.all.count_total == 2 * h * w
    assert st.pooled.all.median == 0.5 * (r[0].max() + r[1].min())     # the two middle ranks: one in each plane
    assert r[0].max() < st.pooled.all.median < r[1].min()
    want = PR.restate(pairs, init, gt, NODATA)
    _check(st, want, None, "two-plane median")
    # P identical planes: the pool has the single plane's medians exactly and P times its count
    d, planes = _planes_case(77, 257, 129, 1)
    for n_planes in (2, 5):
        rep = np.repeat(planes, n_planes, axis=0)
        args = (d["init"], d["gt"], PR.area_defn(d["area"]), d["gt_mask"], d["building"], d["water"], d["forest"], 1.0)
        one = evaluate_pairs_statistics(planes, *args, nodata=NODATA)
        many = evaluate_pairs_statistics(rep, *args, nodata=NODATA)
        for c in R.CLASSES:
            a, b = one.pooled[c], many.pooled[c]
            assert b.count_total == n_planes * a.count_total and b.truncated.count_total == n_planes * a.truncated.count_total
            for k in ("median", "absolute_median", "NMAD", "diff_max", "diff_min"):
                assert a[k] == b[k], (c, k)
            for k in ("median", "absolute_median", "NMAD"):
                assert a.truncated[k] == b.truncated[k], (c, k)
            assert repr(many.pairs[n_planes - 1][c]) == repr(one.pairs[0][c])


def test_a_threshold_that_empties_a_class():
    from resdepth_amd.evaluation import evaluate_pairs_statistics
    d, pairs = _planes_case(31, 64, 67, 3)
    pairs[2] = pairs[0] + 0.25
    pairs[2][pairs[0] == NODATA] = NODATA
    bd = R.dilate(R.mask_of(*d["building"])[0], 2)
    for p in (0, 2):
        pairs[p][bd & (pairs[p] != NODATA)] += 50.0                   # every building residual beyond the threshold
    thr = 6.0
    st = evaluate_pairs_statistics(pairs, d["init"], d["gt"], PR.area_defn(d["area"]), d["gt_mask"], d["building"], d["water"],
                                   d["forest"], thr, nodata=NODATA)
    want = PR.restate(pairs, d["init"], d["gt"], NODATA, d["area"], d["gt_mask"], d["building"], d["water"], d["forest"], thr)
    _check(st, want, thr, "emptied class")
    for by_class in (st.pairs[0], st.pairs[2], st.pooled):
        b = by_class.building
        assert b.count_total > 0 and b.truncated.count_total == 0 and np.isnan(b.truncated.median) and np.isnan(b.truncated.MAE)
        assert by_class.terrain.truncated.count_total > 0


@pytest.mark.parametrize("shape,n_planes", [((64, 67), 3), ((1, 300), 2), ((257, 129), 16)])
def test_c_abi_odd_stride_separate_destination_and_null_valid(shape, n_planes):
    from resdepth_amd import _lib
    lib = _lib.load()
    h, w = shape
    n = h * w
    d, pairs = _planes_case(7 + n_planes, h, w, n_planes)
    d["pred"] = pairs[0]
    _, init, gt, masks, rects = _device_case(d)
    stride = n + 3 if n % 2 == 0 else n + 2
    assert stride % 2 == 1 and stride > n
    span = (n_planes - 1) * stride + n
    buf = torch.full((span,), 12345.0, dtype=torch.float64, device="cuda")
    for p in range(n_planes):
        buf[p * stride:p * stride + n] = torch.from_numpy(pairs[p].reshape(-1)).cuda()
    src = buf.clone()
    res = torch.full((span,), -7.0, dtype=torch.float64, device="cuda")
    cls, valid = _classify_planes(lib, buf, stride, n_planes, init, gt, masks, rects, h, w, res)
    assert torch.equal(buf, src)                                       # a separate destination leaves the planes alone
    kw = dict(init=d["init"], gt=d["gt"], nodata=NODATA, area=d["area"], gt_mask=d["gt_mask"], building=d["building"],
              water=d["water"], forest=d["forest"])
    per = [R.classify(pred=pairs[p], **kw) for p in range(n_planes)]
    for p in range(n_planes):
        np.testing.assert_array_equal(res[p * stride:p * stride + n].cpu().numpy(), per[p][1].reshape(-1))
        np.testing.assert_array_equal(((valid.int() >> p) & 1).cpu().numpy().astype(bool), per[p][2]["all"][1].reshape(-1))
        if p + 1 < n_planes:
            assert bool((res[p * stride + n:(p + 1) * stride] == -7.0).all())         # padding untouched
    # valid == NULL: every plane of the range counts wherever the class bits hold
    need, thr = [0, 8, 16 | 8], [-1.0, 1.5, -1.0]
    p0, p1 = (0, n_planes) if n_planes < 16 else (3, 11)
    got = _pooled(lib, res, stride, n_planes, p0, p1, cls, None, n, need, thr)
    c = cls.cpu().numpy()
    vals = np.concatenate([per[p][1].reshape(-1) for p in range(p0, p1)])
    for s in range(3):
        ok = np.tile((c & need[s]) == need[s], p1 - p0)
        row = PR.stats_row(vals, ok, thr[s] if thr[s] > 0 else None)
        cols = row[:8] if thr[s] <= 0 else [row[8]] + [np.nan, np.nan] + row[9:]
        mine = got[s].copy()
        if thr[s] > 0:
            mine[1:3] = np.nan                           # the truncated record of the restatement has no max / min
        assert_rows(mine[None], np.array([cols]), f"valid NULL set {s}")
    # with the validity word: the same range against the restatement's validity
    got = _pooled(lib, res, stride, n_planes, p0, p1, cls, valid, n, [0], [-1.0])
    ok = np.concatenate([per[p][2]["all"][1].reshape(-1) for p in range(p0, p1)])
    assert_rows(got[:1], np.array([PR.stats_row(vals, ok)[:8]]), "validity word")


# ---- 4. city scale, determinism, where the inputs live ------------------------------------------------------------------------
def _bits(st):
    return repr(st)


@pytest.fixture(scope="module")
def city4():
    h, w, n_planes = 1000, 900, 4
    d = city(seed=2, h=h, w=w)
    rng = np.random.RandomState(12)
    g64 = np.where(d["gt"] == NODATA, 400.0, d["gt"]).astype(np.float64)
    pairs = np.empty((n_planes, h, w))
    pairs[0] = d.pop("pred")
    for p in range(1, n_planes):
        pairs[p] = g64 + rng.laplace(size=(h, w)) * (0.5 + 0.1 * p) - 0.02 * p
        pairs[p][rng.rand(h, w) < 0.01 * (p + 1)] = NODATA
    fused = np.median(pairs, axis=0)
    want = PR.restate(pairs, d["init"], d["gt"], NODATA, d["area"], d["gt_mask"], d["building"], d["water"], d["forest"], 2.0,
                      fused=fused)
    return d, pairs, fused, want


def test_city_scale_four_planes_against_the_restatement(city4):
    from resdepth_amd.evaluation import evaluate_pairs_statistics
    d, pairs, fused, want = city4
    assert want["classes"] == R.CLASSES
    args = (d["init"], d["gt"], PR.area_defn(d["area"]), d["gt_mask"], d["building"], d["water"], d["forest"], 2.0)
    host = evaluate_pairs_statistics(pairs, *args, fused=fused, nodata=NODATA)
    _check(host, want, 2.0, "city", fused=True)
    again = evaluate_pairs_statistics(pairs, *args, fused=fused, nodata=NODATA)
    assert _bits(host) == _bits(again)
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()                    # noqa: E731
    dp, df = cu(pairs), cu(fused)
    keep_p, keep_f = dp.clone(), df.clone()
    dev = evaluate_pairs_statistics(dp, cu(d["init"]), cu(d["gt"]), args[2], (cu(d["gt_mask"][0]), 255.0),
                                    (cu(d["building"][0]), 255.0), (cu(d["water"][0]), 255.0), (cu(d["forest"][0]), 255.0), 2.0,
                                    fused=df, nodata=NODATA)
    assert _bits(host) == _bits(dev)
    assert torch.equal(dp, keep_p) and torch.equal(df, keep_f)         # the caller's tensors are not written
    plain = evaluate_pairs_statistics(pairs, *args, nodata=NODATA)
    assert "fused" not in plain and _bits(plain.pooled) == _bits(host.pooled)


def test_a_real_sweep_scored_where_it_lies():
    from resdepth_amd import GpuGridTiles, GpuPatchSampler, UNet, predict_pairs_linear_blend
    from resdepth_amd.evaluation import evaluate_pairs_statistics
    h, w, tile = 40, 56, 32
    rng = np.random.default_rng(17)
    gt = (400.0 + 5.0 * rng.standard_normal((h, w))).astype(np.float32)
    dsm = (gt + rng.standard_normal((h, w))).astype(np.float32)
    orthos = (110.0 + 40.0 * rng.standard_normal((3, h, w))).astype(np.float32)
    gt[rng.random((h, w)) < 0.05] = NODATA
    smp = GpuPatchSampler(dsm, None, orthos, tile_size=tile, nodata=NODATA, dsm_std=3.0, ortho_mean=110.0, ortho_std=50.0)
    loader = GpuGridTiles(smp, "test", {"x_extent": [(0, w - 1)], "y_extent": [(0, h - 1)]}, "geom-stereo", [[0, 1], [1, 2], [0, 2]],
                          stride=16, batch_size=8, sweep_pairs=True)
    torch.manual_seed(5)
    model = UNet(n_input_channels=3, start_kernel=8, depth=2, bias_conv_layer=True).to("cuda:0").eval()
    plain = predict_pairs_linear_blend(loader, model)
    plain2 = predict_pairs_linear_blend(loader, model)
    assert sorted(vars(plain)) == sorted(vars(plain2)) and plain.device_pairs is None and plain.device_fused is None
    assert plain.pairs.tobytes() == plain2.pairs.tobytes() and plain.fused.tobytes() == plain2.fused.tobytes()
    kept = predict_pairs_linear_blend(loader, model, keep_device=True)
    assert kept.pairs.tobytes() == plain.pairs.tobytes() and kept.fused.tobytes() == plain.fused.tobytes()
    assert kept.device_pairs.is_cuda and kept.device_pairs.dtype == torch.float64
    assert tuple(kept.device_pairs.shape) == kept.pairs.shape == (3, h, w) and tuple(kept.device_fused.shape) == (h, w)
    assert not np.isnan(kept.pairs).any()
    before = kept.device_pairs.clone()
    on_dev = evaluate_pairs_statistics(kept, dsm, gt, residual_threshold=1.0, nodata=NODATA)
    assert torch.equal(kept.device_pairs, before)
    on_host = evaluate_pairs_statistics(kept.pairs.copy(), dsm, gt, residual_threshold=1.0, fused=kept.fused.copy(), nodata=NODATA)
    assert _bits(on_dev) == _bits(on_host) and "fused" in on_dev
    assert on_dev.pooled.all.count_total == sum(s.all.count_total for s in on_dev.pairs) > 0
    want = PR.restate(kept.pairs, dsm, gt, NODATA, thr=1.0, fused=kept.fused)
    _check(on_dev, want, 1.0, "sweep", fused=True)


# ---- 6. refusals: by return code, before anything is launched -------------------------------------------------------------------
def test_refusals():
    from resdepth_amd import _lib
    from resdepth_amd.evaluation import evaluate_pairs_statistics
    lib = _lib.load()
    t, t2, t3 = (torch.zeros(64, dtype=torch.float64, device="cuda") for _ in range(3))
    c8 = torch.zeros(64, dtype=torch.uint8, device="cuda")
    v16 = torch.zeros(64, dtype=torch.int16, device="cuda")
    out = torch.full((21 * 8,), 3.0, dtype=torch.float64, device="cuda")
    ws = torch.zeros(lib.rd_residual_stats_pooled_ws_bytes(1 << 28, 20), dtype=torch.uint8, device="cuda")
    need, thr = (C.c_int * 21)(), (C.c_double * 21)()
    p = lambda x: x.data_ptr()                                                          # noqa: E731
    s = torch.cuda.current_stream().cuda_stream

    def pooled(stride, n_planes, p0, p1, n, ns, nbytes):
        rc = lib.rd_residual_stats_pooled(p(t), stride, n_planes, p0, p1, p(c8), p(v16), n, need, thr, ns, p(out), p(ws), nbytes, s)
        return rc, lib.rd_last_error_string()
    big = 1 << 28
    assert pooled(big, 16, 0, 16, big, 1, ws.numel())[0] == 1          # 16 * 2^28 = 2^32 values
    assert b"2^32" in pooled(big, 16, 0, 16, big, 1, ws.numel())[1]
    assert pooled(4, 0, 0, 1, 4, 1, ws.numel())[0] == 1                # P = 0
    assert pooled(4, 17, 0, 17, 4, 1, ws.numel())[0] == 1              # P = 17
    assert pooled(4, 4, 2, 5, 4, 1, ws.numel())[0] == 1                # range past the planes
    assert pooled(4, 4, -1, 2, 4, 1, ws.numel())[0] == 1
    assert pooled(4, 4, 2, 2, 4, 1, ws.numel())[0] == 1                # empty range
    assert pooled(3, 4, 0, 4, 4, 1, ws.numel())[0] == 1                # planes overlap
    assert pooled(4, 4, 0, 4, 4, 21, ws.numel())[0] == 1               # more than RD_STATS_MAX_SETS
    assert pooled(4, 4, 0, 4, 4, 1, lib.rd_residual_stats_pooled_ws_bytes(4, 1) - 1)[0] == 2          # short workspace
    assert pooled(4, 4, 0, 4, 4, 1, ws.numel())[0] == 0                # and the same call with enough of it

    def classify(n_planes, stride):
        return lib.rd_eval_classify_planes(p(t), stride, n_planes, None, p(t2), 1, p(t3), 1, None, None, None, None, None, None,
                                           -1, 2, 2, NODATA, None, p(t), None, p(c8), p(v16), s)
    assert classify(0, 4) == 1 and classify(17, 4) == 1 and classify(2, 3) == 1 and classify(2, 4) == 0
    torch.cuda.synchronize()
    assert float(out[8:].min()) == 3.0                                 # nothing beyond the one accepted set was written
    z = np.zeros((4, 4))
    for bad in (np.zeros((0, 4, 4)), np.zeros((17, 4, 4)), z):
        with pytest.raises(ValueError):
            evaluate_pairs_statistics(bad, z, z)
    with pytest.raises(ValueError):
        evaluate_pairs_statistics(np.zeros((2, 4, 5)), z, z)
    with pytest.raises(ValueError):
        evaluate_pairs_statistics(np.zeros((2, 4, 4)), z, z, fused=np.zeros((4, 5)))
