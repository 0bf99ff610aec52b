"""The restatements of tests/errmap_ref.py without a GPU: hand-computed cells, Horn's slope on integer planes, the bins against
direct interval tests; the side header include/resdepth_hip_errmap.h against _lib.SIGNATURES_ERRMAP, the library's exports and
build.sh; the argument checks of the front end, which all come before any launch."""
import os
import re

import numpy as np
import pytest

import errmap_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rd_cell_stats", "rd_dsm_slope", "rd_bin_classes"}


def test_cell_stats_on_hand_computed_cells():
    """2 x 2 cells of (4, 4) over 8 x 8, one per case: odd count, even count, one member, empty"""
    r = np.zeros((8, 8))
    cls = np.zeros((8, 8), np.uint8)
    # cell (0, 0): five members -3, -1, 0.5, 2, 4
    for (y, x), v in zip([(0, 0), (1, 2), (2, 1), (3, 3), (0, 3)], [-3.0, -1.0, 0.5, 2.0, 4.0]):
        r[y, x], cls[y, x] = v, 1
    # cell (0, 1): four members -2, 1, 3, 6
    for (y, x), v in zip([(0, 4), (1, 5), (2, 6), (3, 7)], [-2.0, 1.0, 3.0, 6.0]):
        r[y, x], cls[y, x] = v, 1
    # cell (1, 0): one member -1.5; cell (1, 1): values, but none of the class
    r[5, 1], cls[5, 1] = -1.5, 1
    r[4:, 4:] = 7.0
    got = R.cell_stats(r, cls, 4, 4, need=1)
    assert got.shape == (2, 2, 8)
    # |r| sorted 0.5 1 2 3 4: absolute median 2; r sorted -3 -1 0.5 2 4: median 0.5; |r - 2| = 5 3 1.5 0 2 -> median 2
    np.testing.assert_array_equal(got[0, 0], [5, 4.0, -3.0, 10.5 / 5, np.sqrt(30.25 / 5), 2.0, 0.5, 1.4826 * 2.0])
    # |r| sorted 1 2 3 6: absolute median 2.5; median (1 + 3) / 2 = 2; |r - 2.5| = 4.5 1.5 0.5 3.5 -> (1.5 + 3.5) / 2
    np.testing.assert_array_equal(got[0, 1], [4, 6.0, -2.0, 3.0, np.sqrt(50.0 / 4), 2.5, 2.0, 1.4826 * 2.5])
    np.testing.assert_array_equal(got[1, 0], [1, -1.5, -1.5, 1.5, 1.5, 1.5, -1.5, 1.4826 * 3.0])
    assert got[1, 1, 0] == 0 and np.isnan(got[1, 1, 1:]).all()
    # a threshold halves the first cell (|r| <= 2: -1, 0.5, 2) and empties the one-member cell below 1.5
    t = R.cell_stats(r, cls, 4, 4, need=1, thr=2.0)
    np.testing.assert_array_equal(t[0, 0, [0, 1, 2, 6]], [3, 2.0, -1.0, 0.5])
    assert R.cell_stats(r, cls, 4, 4, need=1, thr=1.0)[1, 0, 0] == 0
    # ragged cells: 8 x 8 at (5, 3) is 2 x 3 cells, the last row of cells 3 pixels high, the last column 2 wide
    ragged = R.cell_stats(r, np.ones_like(cls), 5, 3)
    assert ragged.shape == (2, 3, 8)
    np.testing.assert_array_equal(ragged[..., 0], [[15, 15, 10], [9, 9, 6]])
    assert ragged[..., 0].sum() == 64


@pytest.mark.parametrize("alpha,beta,gsd_x,gsd_y", [(3, -2, 0.25, 0.5), (0, 5, 1.0, 2.0), (-7, 0, 0.5, 0.5), (1, 1, 4.0, 0.125)])
def test_slope_of_an_integer_plane_is_exact(alpha, beta, gsd_x, gsd_y):
    y, x = np.mgrid[0:9, 0:11]
    z = (alpha * x + beta * y).astype(np.float64)
    for dsm in (z, z.astype(np.float32)):
        s = R.slope(dsm, gsd_y, gsd_x, nodata=-9999.0)
        want = np.sqrt((alpha / gsd_x) ** 2 + (beta / gsd_y) ** 2)
        np.testing.assert_array_equal(s[1:-1, 1:-1], np.full((7, 9), want))
        ring = np.ones(z.shape, bool)
        ring[1:-1, 1:-1] = False
        assert np.isnan(s[ring]).all()


def test_slope_spreads_nodata_and_nan_over_the_3x3_neighbourhood():
    y, x = np.mgrid[0:9, 0:11]
    z = (2.0 * x - y).astype(np.float64)
    z[4, 5] = -9999.0
    z[6, 2] = np.nan
    s = R.slope(z, 1.0, 1.0, nodata=-9999.0)
    want = np.zeros(z.shape, bool)
    want[3:6, 4:7] = want[5:8, 1:4] = True
    want[0, :] = want[-1, :] = want[:, 0] = want[:, -1] = True
    np.testing.assert_array_equal(np.isnan(s), want)
    assert (s[~want] == np.sqrt(5.0)).all()
    # without a nodata value -9999 is a height like any other
    assert not np.isnan(R.slope(z, 1.0, 1.0)[4, 5]) and np.isnan(R.slope(z, 1.0, 1.0)[6, 2])
    assert np.isnan(R.slope(z[:2], 1.0, 1.0)).all() and R.slope(z[:2], 1.0, 1.0).shape == (2, 11)


def test_bins_are_half_open_and_go_to_planes_of_six():
    edges = [-np.inf, 0.0, 1.0, 2.5, 4.0, 8.0, 16.0, 32.0, np.inf]
    by = np.array([-np.inf, -1.0, 0.0, 0.999, 1.0, 2.5, 7.9, 8.0, 31.0, 32.0, 1e300, np.inf, np.nan, -0.0])
    want = [0, 0, 1, 1, 2, 3, 4, 5, 6, 7, 7, -1, -1, 1]
    np.testing.assert_array_equal(R.bin_index(by, edges), want)
    direct = [next((b for b in range(8) if edges[b] <= v < edges[b + 1]), -1) for v in by]
    assert direct == want
    cls = np.arange(len(by), dtype=np.uint8) * 5 + 3                 # other class bits present: only the low two survive
    planes = R.bin_classes(by, cls, edges)
    assert planes.shape == (2, len(by)) and planes.dtype == np.uint8
    for i, b in enumerate(want):
        lo = int(cls[i]) & 3
        assert planes[0, i] == lo | ((4 << b) if 0 <= b < 6 else 0), i
        assert planes[1, i] == lo | ((4 << (b - 6)) if b >= 6 else 0), i
    assert R.bin_classes(by, cls, [0.0, 1.0]).shape == (1, len(by)) and R.bin_classes(by, cls, list(range(25))).shape[0] == 4


def _side_header():
    text = open(os.path.join(ROOT, "include", "resdepth_hip_errmap.h")).read()
    return text, re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def test_side_header_signatures_constants_and_exports():
    from resdepth_amd import _lib
    main = open(os.path.join(ROOT, "include", "resdepth_hip.h")).read()
    assert '#include "resdepth_hip_errmap.h"' in main
    text, code = _side_header()
    exported = set(re.findall(r"\b(rd_\w+)\s*\(", code))
    assert exported == set(_lib.SIGNATURES_ERRMAP) == NAMES
    for name, (_, args) in _lib.SIGNATURES_ERRMAP.items():
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1)
        assert len(decl.split(",")) == len(args), name
    defines = {k: int(v) for k, v in re.findall(r"#define\s+(RD_\w+)\s+(\d+)", code)}
    assert (defines["RD_CELL_MIN"], defines["RD_CELL_MAX"], defines["RD_BIN_MAX"]) == \
        (_lib.CELL_MIN, _lib.CELL_MAX, _lib.BIN_MAX) == (4, 256, 24)
    # the header owns up to what is asked of it
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    for phrase in ("never contracted", "-0.0 ranks below", "NaN", "fixed tree", "no floating-point atomics", "half-open",
                   "cell_stats_kernel", "dsm_slope_kernel", "bin_classes_kernel", "takes scratch", "overlap"):
        assert phrase in flat, phrase
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name), name
    # the three names live in this header and this table alone
    inc = os.path.join(ROOT, "include")
    for other in sorted(os.listdir(inc)):
        if other != "resdepth_hip_errmap.h":
            body = open(os.path.join(inc, other)).read()
            for name in NAMES:
                assert not re.search(r"\b%s\s*\(" % name, body), (other, name)
    for table in ("SIGNATURES", "SIGNATURES_TTA", "SIGNATURES_PAIRS", "SIGNATURES_EVAL", "SIGNATURES_LOSS", "SIGNATURES_OPTIM",
                  "SIGNATURES_DIST"):
        assert not NAMES & set(getattr(_lib, table)), table


def test_the_kernels_use_the_engines_helpers_and_never_contract():
    from resdepth_amd import evaluation as E
    csrc = os.path.join(ROOT, "resdepth_amd", "csrc")
    assert "resdepth_hip_errmap.h" in open(os.path.join(csrc, "build.sh")).read()
    src = open(os.path.join(csrc, "rd_stats.hip")).read()
    cell = src[src.index("void cell_stats_kernel("):src.index("void dsm_slope_kernel(")]
    for name in ("SetMoments m", "m.reduce(", "in_set(", "key_of(pick_value(", "unkey(", "1.4826"):
        assert name in cell, name
    assert cell.count("atomicAdd(") == cell.count("atomicAdd(&lh") == 2        # integer LDS counters, nothing else
    slope = src[src.index("void dsm_slope_kernel("):src.index("void bin_classes_kernel(")]
    for name in ("__dadd_rn", "__dsub_rn", "__dmul_rn", "__ddiv_rn", "__dsqrt_rn", "__shared__"):
        assert name in slope, name
    assert "p * p" not in slope and "q * q" not in slope        # the squares go through __dmul_rn
    body = src[src.index("int rd_cell_stats("):]
    for name in ("RD_LAUNCH(cell_stats_kernel", "RD_LAUNCH(dsm_slope_kernel", "RD_LAUNCH(bin_classes_kernel", "ProfScope ps(",
                 "RD_REQUIRE(", "RD_LAUNCH_CHECK("):
        assert name in body, name
    assert body.count("RD_LAUNCH(") == 3                           # one launch each
    assert (E.CELL_MIN, E.CELL_MAX, E.BIN_MAX, E.BINS_PER_PLANE) == (4, 256, 24, 6)


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, s):
        self.lines.append(s)


def test_print_binned_writes_one_line_per_bin():
    from resdepth_amd import evaluation as E
    row = lambda k: E._stats_dict([10.0 * k, 3.0, -2.0, 1.0 * k, 1.5 * k, 0.5, 0.25 * k, 0.75], None, None)
    stats = [E.AttrDict(lo=0.0, hi=5.0, initial=row(2), refined=row(1)),
             E.AttrDict(lo=5.0, hi=float("inf"), initial=row(4), refined=row(3))]
    log = _Log()
    E.print_binned(stats, log, unit="deg")
    assert len(log.lines) == 3 and "Bin [deg]" in log.lines[0] and "NMAD [m]" in log.lines[0]
    assert log.lines[1].startswith("[    0.000,    5.000)\t        10\t     2.000 ->     1.000\t     3.000 ->     1.500")
    assert log.lines[2].startswith("[    5.000,      inf)\t        30\t") and log.lines[2].endswith("\n")
    assert not log.lines[1].endswith("\n")


def test_argument_errors_are_raised_before_any_launch():
    """on a machine without a GPU nothing below can reach a launch: a ValueError means the check came first"""
    from resdepth_amd import evaluation as E
    z = np.zeros((8, 8), np.float32)
    for cell in (3, 257, (4, 300), (0, 8), (4, 4, 4)):
        with pytest.raises(ValueError):
            E.error_map(z, z, cell)
    with pytest.raises(ValueError):
        E.error_map(z, z, 4, residual_threshold=float("inf"))
    for edges in ([0.0], [0.0, 0.0], [1.0, 0.5], [0.0, float("nan"), 2.0], list(range(26))):
        with pytest.raises(ValueError):
            E.evaluate_binned(z, z, z, z, edges)
    with pytest.raises(ValueError, match="gsd"):
        E.evaluate_binned(z, z, z, "slope", [0.0, 10.0])
    with pytest.raises(ValueError):
        E.evaluate_binned(z, z, z, "aspect", [0.0, 10.0], gsd=1.0)
    with pytest.raises(ValueError):
        E.evaluate_binned(z, z, z, "slope", [0.0, 100.0, 120.0], gsd=1.0)      # tan() does not increase across 90 degrees
    with pytest.raises(ValueError):
        E.evaluate_binned(z, z, z, z[:4], [0.0, 10.0])
    assert E._degrees_to_tangent(45.0) == np.tan(np.radians(45.0)) and E._degrees_to_tangent(float("-inf")) == float("-inf")
