"""The distance transform without a GPU: the side header include/resdepth_hip_edt.h against _lib.SIGNATURES_EDT, the library's
exports and build.sh; the scratch query as a function of the shape; the argument checks of resdepth_amd.morphology, which all
come before any launch; and the numpy oracles of tests/edt_ref.py against each other, against scipy where it is installed, and
against the cross dilation that evaluation.dilate_mask computes."""
import math
import os
import re

import numpy as np
import pytest

import edt_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rd_edt_ws_bytes", "rd_edt_sq", "rd_fill_nearest"}
HEADER = "resdepth_hip_edt.h"


def test_side_header_signatures_constants_and_exports():
    from resdepth_amd import _lib
    main = open(os.path.join(ROOT, "include", "resdepth_hip.h")).read()
    assert main.count('#include "%s"' % HEADER) == 1
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    exported = set(re.findall(r"\b(rd_\w+)\s*\(", code))
    assert exported == set(_lib.SIGNATURES_EDT) == NAMES
    for name, (_, args) in _lib.SIGNATURES_EDT.items():
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1)
        assert len(decl.split(",")) == len(args), name
    defines = {k: int(v) for k, v in re.findall(r"#define\s+(RD_\w+)\s+(\d+)", code)}
    assert (defines["RD_EDT_MAX_ROWS"], defines["RD_EDT_MAX_COLS"], defines["RD_EDT_NONE"], defines["RD_EDT_BAND_ROWS"]) == \
        (_lib.EDT_MAX_ROWS, _lib.EDT_MAX_COLS, _lib.EDT_NONE, _lib.EDT_BAND_ROWS) == (R.MAX_ROWS, R.MAX_COLS, R.NONE, R.BAND_ROWS)
    assert R.NONE == 2 ** 31 - 1 and R.MAX_ROWS ** 2 + R.MAX_COLS ** 2 < 2 ** 31 and R.MAX_ROWS * R.MAX_COLS < 2 ** 31
    # the header owns up to what is asked of it
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    for phrase in ("THE TIE RULE", "smallest |x - c| wins, then the smaller column x, then the smaller row y", "no atomics",
                   "no floating point", "whatever the alignment", "same bits on every call", "idx may be null", "never dereferenced",
                   "Memory: reads", "and nothing else", "launches nothing and writes nothing", "Refused:", "edt_band_kernel",
                   "edt_column_kernel", "edt_row_kernel", "fill_nearest_kernel", "overlap", "alignment: none beyond the element's own"):
        assert phrase in flat, phrase
    assert flat.count("Memory: reads") == 2 and flat.count("Refused:") == 2
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.rd_version() == 116                    # the feature is detected by symbol
    # the three names live in this header and this table alone
    inc = os.path.join(ROOT, "include")
    for other in sorted(os.listdir(inc)):
        if other != HEADER:
            body = open(os.path.join(inc, other)).read()
            for name in NAMES:
                assert not re.search(r"\b%s\s*\(" % name, body), (other, name)
    tables = [t for t in dir(_lib) if t.startswith("SIGNATURES") and t != "SIGNATURES_EDT"]
    assert "SIGNATURES" in tables and len(tables) >= 11
    for table in tables:
        assert not NAMES & set(getattr(_lib, table)), table


def test_no_new_unit_and_every_launch_through_rd_launch():
    csrc = os.path.join(ROOT, "resdepth_amd", "csrc")
    build = open(os.path.join(csrc, "build.sh")).read()
    units = re.search(r'^UNITS="([^"]*)"$', build, re.M).group(1).split()
    assert len(units) == 12 and "all twelve translation" in build and HEADER in build
    src = open(os.path.join(csrc, "rd_stats.hip")).read()
    # a section of its own between the plane fusion and the error maps, whose launches tests/test_errmap_cpu.py counts to the end
    assert src.index("int rd_fuse_planes(") < src.index("void edt_band_kernel(") < src.index("int rd_fill_nearest(") < \
        src.index("void cell_stats_kernel(")
    end = src.index('}  // extern "C"', src.index("int rd_fill_nearest("))
    code = re.sub(r"//[^\n]*", "", src[src.index("void edt_band_kernel("):end])
    assert "hipLaunchKernelGGL" not in code and "<<<" not in code and "atomic" not in code
    assert code.count("RD_LAUNCH(") == 5 and code.count("RD_LAUNCH_CHECK(") == 4       # band, column, row; the fill in two widths
    for word in ("float", "double ", "sqrt"):
        assert word not in code[:code.index("static bool edt_overlap(")], word         # integer kernels
    for name in ("__shared__", "__syncthreads_or("):
        assert name in code, name


def test_the_scratch_query_is_a_function_of_the_shape():
    from resdepth_amd import _lib
    q = _lib.load().rd_edt_ws_bytes
    assert q(0, 5) == q(5, 0) == q(-1, -1) == q(R.MAX_ROWS + 1, 4) == q(4, R.MAX_COLS + 1) == q(2 ** 31 - 1, 2 ** 31 - 1) == 0
    b = R.BAND_ROWS
    assert q(1, 1) == 8 and q(b, 70) == 560 and q(b + 1, 70) == 1120 and q(8192, 8192) == 8192 // b * 8192 * 8
    assert q(R.MAX_ROWS, R.MAX_COLS) == R.MAX_ROWS // b * R.MAX_COLS * 8
    sizes = [q(rows, 37) for rows in range(1, 4 * b + 2)]
    assert all(x <= y for x, y in zip(sizes, sizes[1:])) and sizes == [q(rows, 37) for rows in range(1, 4 * b + 2)]


def test_argument_errors_are_raised_before_any_launch():
    """on a machine without a GPU nothing below can reach a launch: a ValueError means the check came first"""
    import resdepth_amd as pkg
    from resdepth_amd import morphology as M
    for name in ("distance_transform", "edge_distance", "buffer_mask", "fill_voids"):
        assert getattr(pkg, name) is getattr(M, name) and name in pkg.__all__
    z = np.zeros((8, 8), np.float32)
    calls = {
        "distance_transform": lambda x, **kw: M.distance_transform(x, **kw),
        "edge_distance": lambda x, **kw: M.edge_distance(x, **kw),
        "buffer_mask": lambda x, **kw: M.buffer_mask(x, kw.pop("radius", 2.0), **kw),
        "fill_voids": lambda x, **kw: M.fill_voids(x, **kw),
    }

    class Huge:
        """a raster beyond the limits that takes no memory: the shape is all the checks may look at"""
        def __init__(self, *shape):
            self.shape = shape

    for name, fn in calls.items():
        for x in (z[0], np.zeros((2, 8, 8)), np.zeros((0, 8)), np.zeros((8, 0)), np.float32(1.0), Huge(R.MAX_ROWS + 1, 4),
                  Huge(4, R.MAX_COLS + 1)):
            with pytest.raises(ValueError):
                fn(x)
        for gsd in (0.0, -1.0, float("nan"), float("inf"), (1.0, 2.0), (0.5, 0.25), (1.0, 0.0), (1.0, 1.0, 1.0), None):
            with pytest.raises(ValueError):
                fn(z, gsd=gsd)
    for bad in (-1.0, float("nan"), -1e-9):
        with pytest.raises(ValueError):
            M.fill_voids(z, max_distance=bad)
    with pytest.raises(ValueError):
        M.buffer_mask(z, float("nan"))
    # the threshold both the front end and the tests use
    assert M.squared_threshold(2.0, 1.0) == R.threshold(2.0, 1.0) == 4 and M.squared_threshold(5.0, 0.5) == 100
    assert M.squared_threshold(0.3, 0.1) == R.threshold(0.3, 0.1) == 9          # 0.3 / 0.1 rounds below 3: the 1e-9 is for this
    assert M.squared_threshold(0.0, 1.0) == 0 and M.squared_threshold(2.9999, 1.0) == 8
    assert M.squared_threshold(1e9, 0.5) == M.squared_threshold(math.inf, 1.0) == M.NO_CAP == R.NONE - 1


# ---- the oracles -------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 0.5), (1, 9, 0.3), (9, 1, 0.3), (3, 5, 0.4), (17, 23, 0.05), (23, 17, 0.5), (31, 40, 0.01), (12, 12, 0.97)]


@pytest.mark.parametrize("case", SHAPES, ids=lambda c: "%dx%d_%g" % c)
def test_the_two_oracles_agree_and_the_index_attains_the_distance(case):
    rows, cols, density = case
    for seed in range(3):
        m = R.random_mask(rows, cols, density, seed)
        for invert in (False, True):
            a, b = R.brute(m, invert), R.separable(m, invert)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            assert R.attains(m, *a, invert=invert)
            assert a[0].dtype == a[1].dtype == np.int32


def test_the_tie_rule_by_hand():
    m = np.zeros((5, 5), np.uint8)
    m[0, 2] = m[4, 2] = m[2, 0] = m[2, 4] = 1             # four pixels at distance 2 of the centre
    for oracle in (R.brute, R.separable):
        d2, idx = oracle(m)
        assert d2[2, 2] == 4 and idx[2, 2] == 0 * 5 + 2   # |dx| = 0 first, then the smaller row
        assert d2[2, 1] == 1 and idx[2, 1] == 2 * 5 + 0
    m = np.zeros((3, 5), np.uint8)
    m[1, 0] = m[1, 4] = 1
    assert R.brute(m)[1][1, 2] == 1 * 5 + 0               # equal |dx|: the smaller column
    m = np.zeros((3, 4), np.uint8)
    m[0, 0] = m[2, 1] = 1                                  # from (1, 1): d2 = 2 with |dx| = 1 against d2 = 1 with |dx| = 0
    assert R.brute(m)[1][1, 1] == 2 * 4 + 1
    m[2, 1], m[1, 3], m[0, 0], m[0, 2], m[2, 2] = 0, 0, 0, 1, 1           # from (1, 1): (0, 2) and (2, 2), both d2 = 2 and dx = 1
    assert R.brute(m)[1][1, 1] == 0 * 4 + 2 == R.separable(m)[1][1, 1]    # the smaller row
    d2, idx = R.brute(np.zeros((2, 3)))
    assert (d2 == R.NONE).all() and (idx == -1).all()


def test_the_oracles_agree_with_scipy_on_the_squared_distances():
    ndimage = pytest.importorskip("scipy.ndimage")
    for rows, cols, density in SHAPES + [(60, 90, 0.002), (90, 60, 0.2)]:
        m = R.random_mask(rows, cols, density, 7)
        if not m.any():
            continue
        dist = ndimage.distance_transform_edt(m == 0)      # scipy measures to the nearest ZERO
        assert np.array_equal(np.rint(dist * dist).astype(np.int64), R.separable(m)[0].astype(np.int64))
        assert np.abs(dist * dist - R.separable(m)[0]).max() < 1e-6


def test_small_discs_are_the_cross_dilation_and_larger_ones_are_not():
    m = R.random_mask(40, 60, 0.01, 11)
    d2 = R.separable(m)[0]
    assert np.array_equal(d2 <= 1, R.cross_dilation(m, 1)) and np.array_equal(d2 <= 4, R.cross_dilation(m, 2))
    assert not np.array_equal(d2 <= 9, R.cross_dilation(m, 3))
    ndimage = pytest.importorskip("scipy.ndimage")
    for k in (1, 2, 3):
        assert np.array_equal(R.cross_dilation(m, k), ndimage.binary_dilation(m != 0, iterations=k))


def test_the_fill_oracle_by_hand():
    z = np.array([[1.0, -9999.0, 3.0], [np.nan, -9999.0, -9999.0], [7.0, 8.0, -9999.0]], np.float32)
    got, filled = R.fill_voids(z, -9999.0)
    assert np.array_equal(got, np.array([[1, 1, 3], [1, 8, 3], [7, 8, 8]], np.float32))       # (0, 1): the smaller column
    assert np.array_equal(filled, np.isnan(z) | (z == -9999.0))
    got, filled = R.fill_voids(z, -9999.0, max_distance=0.5, gsd=1.0)
    assert np.array_equal(got.view(np.uint32), z.view(np.uint32)) and not filled.any()
    out = R.fill_nearest(z, np.ones((3, 3), np.int32), np.array([[-1, 9, 100], [0, 0, 0], [8, 8, 8]], np.int32), 1)
    assert np.array_equal(out[0].view(np.uint32), z[0].view(np.uint32)) and (out[1] == 1.0).all() and (out[2] == -9999.0).all()
