"""The quantile / share oracle of tests/dist_ref.py without a GPU: against numpy's own `linear` quantile and against direct
counting; the side header include/resdepth_hip_dist.h against _lib.SIGNATURES_DIST, the library and the kernels' source; and
the report lines of print_statistics with and without the new keys."""
import os
import re

import numpy as np
import pytest

import dist_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = (0.0, 0.05, 0.5, 0.68, 0.9, 0.95, 1.0)


def _draws():
    """3000 Laplace draws with duplicates at scales 1e-3 .. 1e3, sizes 1 .. 400"""
    rng = np.random.RandomState(7)
    for k in range(3000):
        n = int(rng.randint(1, 401))
        a = rng.laplace(size=n) * 10.0 ** rng.uniform(-3, 3)
        if n >= 10:
            a[rng.randint(0, n, size=n // 10)] = a[rng.randint(0, n, size=n // 10)]
        yield a, LEVELS[k % len(LEVELS)], k & 1


def test_the_oracle_is_numpys_linear_quantile_within_the_roundings():
    """Either interpolation form rounds at most three times on quantities of magnitude <= 2 M, M = max(|v_lo|, |v_hi|): the two
    differ by at most 16 * 2^-53 * M.  Not measured: counted."""
    worst = 0.0
    for a, q, mode in _draws():
        v = np.sort(np.abs(a) if mode else a)
        got = dist_ref.quantile(a, q, mode)
        want = np.quantile(v, q, method="linear")
        h = (len(v) - 1) * q
        lo, hi = int(np.floor(h)), int(np.ceil(h))
        m = max(abs(v[lo]), abs(v[hi]))
        err = abs(got - want)
        assert err <= 16 * 2.0 ** -53 * m, (len(v), q, mode, got, want)
        assert min(v[lo], v[hi]) <= got <= max(v[lo], v[hi])
        if m > 0:
            worst = max(worst, err / (2.0 ** -53 * m))
    print(f"worst difference to np.quantile: {worst:.2f} x 2^-53 x M")


def test_the_ranks_of_the_header():
    # q = 0.9: c = 11 gives h = 9 exactly (the g == 0 branch), c = 12 gives 9.9
    v = np.arange(12, dtype=np.float64) ** 2
    assert np.float64(10) * np.float64(0.9) == 9.0 and dist_ref.quantile(v[:11], 0.9, 0) == 81.0
    h = np.float64(11) * np.float64(0.9)
    assert h != np.floor(h) and dist_ref.quantile(v, 0.9, 0) == 81.0 + (h - 9.0) * (100.0 - 81.0)
    assert dist_ref.quantile(v, 0.0, 0) == 0.0 and dist_ref.quantile(v, 1.0, 0) == 121.0
    assert np.isnan(dist_ref.quantile(v[:0], 0.5, 0)) and np.isnan(dist_ref.share(v[:0], 1.0))
    # the median of the eight numbers is 0.5 * (a + b): the same value here, in general only within the bound above
    assert dist_ref.quantile(v, 0.5, 0) == 0.5 * (v[5] + v[6])
    # mode 1 ranks |r|
    assert dist_ref.quantile(-v, 1.0, 1) == 121.0 and dist_ref.quantile(-v, 1.0, 0) == 0.0


def test_the_key_order_puts_minus_zero_below_plus_zero_and_round_trips():
    v = np.array([0.0, -0.0, -1.25, 3.0, -np.inf, np.inf, 5e-324, -5e-324])
    k = dist_ref.keys_of(v)
    np.testing.assert_array_equal(dist_ref.values_of(k).view(np.int64), v.view(np.int64))
    r = dist_ref.ranked(v, 0)
    np.testing.assert_array_equal(r, np.sort(v))
    assert np.signbit(r[3]) and not np.signbit(r[4]) and r[3] == r[4] == 0.0
    assert not np.signbit(dist_ref.ranked(v, 1)).any()


def test_the_share_is_direct_counting():
    rng = np.random.RandomState(3)
    a = np.round(rng.laplace(size=5000), 2)
    for tau in (0.0, 0.5, 1.0, 1e300):
        n_in = sum(1 for x in a if abs(x) <= tau)
        assert dist_ref.share(a, tau) == n_in / 5000
    assert dist_ref.share(a, 1e300) == 1.0 and 0.0 < dist_ref.share(a, 0.0) < 0.05
    cls = rng.randint(0, 16, size=a.size)
    m = dist_ref.members(a, cls, 1 | 8, 1.0)
    assert len(m) == sum(1 for x, c in zip(a, cls) if (c & 9) == 9 and abs(x) <= 1.0)
    row = dist_ref.row(m, (0.9, 0.5), (1, 0), (0.5,))
    assert row.shape == (4,) and row[0] == len(m) and row[1] == dist_ref.quantile(m, 0.9, 1) and row[3] == dist_ref.share(m, 0.5)


def _side_header():
    text = open(os.path.join(ROOT, "include", "resdepth_hip_dist.h")).read()
    return text, re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def test_side_header_signatures_constants_and_version():
    from resdepth_amd import _lib
    main = open(os.path.join(ROOT, "include", "resdepth_hip.h")).read()
    assert '#include "resdepth_hip_dist.h"' in main
    assert "rd_residual_dist" not in re.sub(r'#include "resdepth_hip_dist.h".*', "", main)
    text, code = _side_header()
    exported = set(re.findall(r"\b(rd_\w+)\s*\(", code))
    assert exported == set(_lib.SIGNATURES_DIST) == {"rd_residual_dist_sets_ws_bytes", "rd_residual_dist_sets",
                                                     "rd_residual_dist_pooled_ws_bytes", "rd_residual_dist_pooled"}
    # one ctypes argument per parameter of the declaration
    for name, (_, args) in _lib.SIGNATURES_DIST.items():
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1)
        assert len(decl.split(",")) == len(args), name
    defines = {k: int(v) for k, v in re.findall(r"#define\s+(RD_\w+)\s+(\d+)", code)}
    assert (defines["RD_DIST_MAX_Q"], defines["RD_DIST_MAX_T"]) == (_lib.DIST_MAX_Q, _lib.DIST_MAX_T) == (8, 8)
    # the header owns up to what the issue asks of it
    for phrase in ("NOT in bits", "-0.0 ranks below", "NaN", "never contracted"):
        assert phrase in text, phrase
    lib = _lib.load()
    assert lib.rd_version() == 116
    # the scratch query is host arithmetic, and at most what the largest call needs: 20 histogram pairs, the counters, 160
    # selection states and weights
    nb = lib.rd_residual_dist_sets_ws_bytes(1, 1, 1, 1)
    assert 0 < nb <= 20 * 512 * 4 + 20 * 9 * 8 + 160 * (48 + 8) + 256
    assert lib.rd_residual_dist_sets_ws_bytes(1 << 26, 20, 8, 8) == nb == lib.rd_residual_dist_pooled_ws_bytes(1 << 26, 20, 8, 8)


def test_the_kernels_share_the_engine_and_round_three_times():
    from resdepth_amd import evaluation as E
    csrc = os.path.join(ROOT, "resdepth_amd", "csrc")
    assert "resdepth_hip_dist.h" in open(os.path.join(csrc, "build.sh")).read()
    src = open(os.path.join(csrc, "rd_stats.hip")).read()
    for name in ("__dsub_rn", "__dmul_rn", "__dadd_rn", "dist_prepare_kernel", "dist_finish_kernel", "run_group("):
        assert name in src, name
    # the selector table: no kernel addresses a state as set * 3 + mode any more, the medians' plan fills the table instead
    assert not re.search(r"st\[g\.set\(", src) and src.count("st[g.sel(") >= 4 and "g.put(j, set, mode, set * 3 + mode)" in src
    # both forms reuse the medians' histogram and pick kernels
    body = src[src.index("int rd_residual_dist_sets("):]
    for name in ("sets_hist_kernel", "pooled_hist_kernel", "sets_dist_count_kernel", "pooled_dist_count_kernel"):
        assert name in body, name
    assert src.count("RD_LAUNCH(sets_pick_kernel") == 1
    assert E.LE == (0.68, 0.90, 0.95) and (E.MAX_Q, E.MAX_T) == (8, 8)


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, s):
        self.lines.append(s)


def _stats(E, extra=False, truncated=False):
    st = E.AttrDict(truncation=truncated, count_total=10.0, diff_max=3.0, diff_min=-2.0, MAE=1.0, RMSE=1.5, absolute_median=0.5,
                    median=0.25, NMAD=0.75)
    if truncated:
        st.truncated = E.AttrDict(count_total=8.0, threshold=2.0, MAE=0.5, RMSE=0.6, absolute_median=0.4, median=0.1, NMAD=0.3)
    if extra:
        for d, k in ((st, 1.0),) + (((st.truncated, 0.5),) if truncated else ()):
            d["abs_quantile"] = {0.68: 1.25 * k, 0.9: 2.5 * k, 0.95: 3.0 * k}
            d["quantile"] = {0.05: -1.5 * k}
            d["within"] = {1.0: 0.87, 2.0: 1.0}
    return st


@pytest.mark.parametrize("truncated", [False, True])
def test_print_statistics_keeps_the_block_and_adds_one_line_per_value(truncated):
    from resdepth_amd import evaluation as E
    old, new = _Log(), _Log()
    E.print_statistics(_stats(E, False, truncated), old)
    E.print_statistics(_stats(E, True, truncated), new)
    assert len(old.lines) == (12 if truncated else 7)
    assert old.lines[0] == "Maximum residual error [m]:\t\t\t\t\t\t{:10.3f} m".format(3.0)
    assert old.lines[6] == "Normalized median absolute deviation (NMAD) [m]:\t\t\t{:10.3f} m\n".format(0.75)
    assert not any("LE90" in s or "quantile" in s or "within" in s for s in old.lines)
    # the reference's lines are all there, in order; the new ones follow their block
    assert [s for s in new.lines if s in old.lines] == old.lines
    added = new.lines[7:13]
    assert added == ["Linear error LE68 (|residual| quantile) [m]:\t\t\t\t{:10.3f} m".format(1.25),
                     "Linear error LE90 (|residual| quantile) [m]:\t\t\t\t{:10.3f} m".format(2.5),
                     "Linear error LE95 (|residual| quantile) [m]:\t\t\t\t{:10.3f} m".format(3.0),
                     "Residual quantile q=0.05 [m]:\t\t\t\t\t\t{:10.3f} m".format(-1.5),
                     "Share of pixels within 1.00 m [%]:\t\t\t\t\t{:10.3f} %".format(87.0),
                     "Share of pixels within 2.00 m [%]:\t\t\t\t\t{:10.3f} %\n".format(100.0)]
    if truncated:
        assert len(new.lines) == 24 and new.lines[13] == old.lines[7]
        assert new.lines[18] == "Truncated linear error LE68 (|residual| quantile) [m]:\t\t\t{:10.3f} m".format(0.625)
        assert new.lines[21].startswith("Truncated residual quantile q=0.05 [m]:\t")
        assert new.lines[23].startswith("Truncated share of pixels within 2.00 m [%]:\t") and new.lines[23].endswith("%\n")
    else:
        assert len(new.lines) == 13
    # only the keys present print
    some = _stats(E, True, False)
    del some["quantile"], some["within"]
    log = _Log()
    E.print_statistics(some, log, print_min_max=False)
    assert len(log.lines) == 5 + 3 and log.lines[-1].endswith(" m\n")


def test_the_options_are_checked_on_the_host():
    from resdepth_amd import evaluation as E
    assert E._dist_options(None, None, None) is None and E._dist_options((), [], None) is None
    d = E._dist_options(E.LE, (0.05,), (1, 2))
    assert (d.n_q, d.n_t, d.width) == (4, 2, 7) and list(d.mode_a) == [1, 1, 1, 0] and list(d.tau_a) == [1.0, 2.0]
    st = {}
    d.fill(st, np.arange(7.0))
    assert st == {"abs_quantile": {0.68: 1.0, 0.9: 2.0, 0.95: 3.0}, "quantile": {0.05: 4.0}, "within": {1.0: 5.0, 2.0: 6.0}}
    only = {}
    E._dist_options(None, None, (0.5,)).fill(only, np.array([9.0, 0.25]))
    assert only == {"within": {0.5: 0.25}}
    for bad in (dict(abs_quantiles=(1.5,)), dict(quantiles=(-0.1,)), dict(within=(-1.0,)), dict(within=(float("inf"),)),
                dict(quantiles=(float("nan"),)), dict(abs_quantiles=[0.5] * 5, quantiles=[0.5] * 4), dict(within=[1.0] * 9)):
        with pytest.raises(ValueError):
            E._dist_options(bad.get("abs_quantiles"), bad.get("quantiles"), bad.get("within"))


def test_host_rows_land_under_the_right_class_and_key():
    """_class_stats on a synthetic read-back: three classes under a threshold, so six rows in (full, truncated) steps, each
    row its eight numbers and behind them (count, one |residual| level, one signed level, two shares).  Every number is
    distinct -- 100 * row + column -- so a value under a wrong class, in the wrong one of stats / stats.truncated or under a
    wrong key shows."""
    from resdepth_amd import evaluation as E
    keys = ["count_total", "diff_max", "diff_min", "MAE", "RMSE", "absolute_median", "median", "NMAD"]
    classes, thr = ["all", "building", "terrain"], 2.0
    dist = E._dist_options((0.9,), (0.05,), (1.0, 2.0))
    assert dist.width == 5
    host = 100.0 * np.arange(6.0)[:, None] + np.arange(13.0)[None, :]
    st = E._class_stats(host, classes, thr, dist)
    assert list(st) == classes
    for q, c in enumerate(classes):
        full, trunc = 100.0 * (2 * q), 100.0 * (2 * q + 1)
        extra = lambda base: {"abs_quantile": {0.9: base + 9}, "quantile": {0.05: base + 10},         # noqa: E731
                              "within": {1.0: base + 11, 2.0: base + 12}}
        want = {"truncation": True,
                "truncated": {"count_total": trunc, "threshold": thr, "MAE": trunc + 3, "RMSE": trunc + 4,
                              "absolute_median": trunc + 5, "median": trunc + 6, "NMAD": trunc + 7, **extra(trunc)},
                **{k: full + j for j, k in enumerate(keys)}, **extra(full)}
        assert st[c] == want, c
        assert list(st[c]) == list(want) and list(st[c].truncated) == list(want["truncated"]), c     # the order of the keys too
        assert all(type(v) is float for v in st[c].values() if not isinstance(v, (dict, bool))), c
    # the same rows without options and without a threshold: one row per class, exactly the old keys
    plain = E._class_stats(host, classes, None)
    for q, c in enumerate(classes):
        assert list(plain[c]) == ["truncation"] + keys, c
        assert plain[c] == {"truncation": False, **{k: 100.0 * q + j for j, k in enumerate(keys)}}, c
