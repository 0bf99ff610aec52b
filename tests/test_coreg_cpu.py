"""Co-registration without a GPU: the side header include/resdepth_hip_coreg.h against _lib.SIGNATURES_COREG, the library's exports
and build.sh; the argument checks of the front end, which all come before any launch; and the method itself in the numpy oracle
tests/coreg_ref.py -- a known shift recovered on the analytic surface inside 0.01 px and 0.002 m, the slope cap seen to act on a
box, a plane and a constant raster refused.

The bars: a numpy prototype of the method ended within 0.0014 px and 0.0003 m of the truth on these cases; 0.01 px and 0.002 m are
about seven times that, to absorb the smoothing bias of the bilinear resampling on other surfaces."""
import math
import os
import re

import numpy as np
import pytest

import coreg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rd_shift_sums_ws_bytes", "rd_shift_sums", "rd_translate_bilinear"}
HEADER = "resdepth_hip_coreg.h"


def _side_header():
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    return text, re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def test_side_header_signatures_constants_and_exports():
    from resdepth_amd import _lib
    main = open(os.path.join(ROOT, "include", "resdepth_hip.h")).read()
    assert main.count('#include "%s"' % HEADER) == 1
    text, code = _side_header()
    exported = set(re.findall(r"\b(rd_\w+)\s*\(", code))
    assert exported == set(_lib.SIGNATURES_COREG) == NAMES
    for name, (_, args) in _lib.SIGNATURES_COREG.items():
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1)
        assert len(decl.split(",")) == len(args), name
    defines = {k: int(v) for k, v in re.findall(r"#define\s+(RD_\w+)\s+(\d+)", code)}
    assert (defines["RD_SHIFT_NSUMS"], defines["RD_SHIFT_MAX_BLOCKS"], defines["RD_SHIFT_MAX_TILES"]) == \
        (_lib.SHIFT_NSUMS, _lib.SHIFT_MAX_BLOCKS, _lib.SHIFT_MAX_TILES) == (10, 2048, 1 << 30)
    # the header owns up to what is asked of it
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    for phrase in ("never contracted", "fixed tree", "No floating-point atomics", "whatever the alignment", "ten zeros",
                   "Memory: reads", "and nothing else", "launches nothing and writes nothing", "Refused:", "NOT NEEDED",
                   "0x7ff8000000000000", "as doubles", "shift_sums_kernel", "shift_sums_finish_kernel",
                   "translate_bilinear_kernel", "overlap"):
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
    tables = [t for t in dir(_lib) if t.startswith("SIGNATURES") and t != "SIGNATURES_COREG"]
    assert len(tables) >= 10
    for table in tables:
        assert not NAMES & set(getattr(_lib, table)), table


def test_the_new_unit_is_built_and_launches_through_rd_launch():
    csrc = os.path.join(ROOT, "resdepth_amd", "csrc")
    build = open(os.path.join(csrc, "build.sh")).read()
    units = re.search(r'^UNITS="([^"]*)"$', build, re.M).group(1).split()
    assert "rd_coreg" in units and len(units) == 12 and "all twelve translation" in build and HEADER in build
    code = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "rd_coreg.hip")).read())
    assert "hipLaunchKernelGGL" not in code and "<<<" not in code and "atomic" not in code
    assert code.count("RD_LAUNCH(") == 3 and code.count("RD_LAUNCH_CHECK(") == 3   # the sums and their finish, the resampler
    kernels = code[code.index("void shift_sums_kernel("):code.index("using namespace rd;")]
    for name in ("__dadd_rn", "__dsub_rn", "__dmul_rn", "__ddiv_rn", "__shared__"):
        assert name in kernels, name
    # no bare fp64 product or sum of two values in the kernels: everything goes through the intrinsics
    for bare in ("p * p", "q * q", "p * q", "p * d", "q * d", "d * d", "fx * ", "fy * ", "sqrt"):
        assert bare not in kernels, bare


def test_the_scratch_query_is_a_function_of_the_shape():
    from resdepth_amd import _lib
    lib = _lib.load()
    q = lib.rd_shift_sums_ws_bytes
    assert q(0, 5) == q(5, 0) == q(-1, -1) == 0
    assert q(1, 1) == q(16, 64) == 80 and q(17, 64) == q(16, 65) == 160
    assert q(16 * 32, 64 * 64) == 80 * 2048                                          # 2048 tiles: one each
    assert q(16 * 32 + 1, 64 * 64) == 80 * -(-(33 * 64) // 2)                        # 2112 tiles: two each, 1056 blocks
    assert q(8192, 8192) == 80 * 2048
    assert q(2 ** 31 - 1, 2 ** 31 - 1) == 0                                          # beyond RD_SHIFT_MAX_TILES: refused


def test_argument_errors_are_raised_before_any_launch():
    """on a machine without a GPU nothing below can reach a launch: a ValueError means the check came first"""
    import resdepth_amd as pkg
    from resdepth_amd import coregistration as CR
    assert pkg.estimate_shift is CR.estimate_shift and pkg.coregister is CR.coregister and pkg.translate is CR.translate
    z = np.zeros((8, 8), np.float32)
    for fn in (CR.estimate_shift, CR.coregister):
        for bad in (dict(reference=z[:4]), dict(source=z[0]), dict(source=np.zeros((2, 8, 8)), reference=np.zeros((2, 8, 8))),
                    dict(source=np.zeros((0, 8)), reference=np.zeros((0, 8))), dict(gsd=0.0), dict(gsd=-1.0),
                    dict(gsd=float("nan")), dict(gsd=float("inf")), dict(gsd=(1.0, 0.0)), dict(gsd=(1.0, 2.0, 3.0)),
                    dict(gsd=None), dict(residual_threshold=-1.0), dict(residual_threshold=float("inf")),
                    dict(residual_threshold=0.0), dict(max_slope=0.0), dict(max_slope=90.0), dict(max_slope=-5.0),
                    dict(max_slope=120.0), dict(max_slope=float("nan")), dict(mask=np.ones((8, 7), bool))):
            kw = dict(dict(source=z, reference=z, gsd=1.0), **bad)
            with pytest.raises(ValueError):
                fn(kw.pop("source"), kw.pop("reference"), kw.pop("gsd"), **kw)
    for bad in (dict(max_iter=0), dict(max_iter=2.5), dict(tol=0.0), dict(tol=-1e-3), dict(tol=float("nan"))):
        with pytest.raises(ValueError):
            CR.coregister(z, z, 1.0, **bad)
    for shift, dz in (((float("nan"), 0.0), 0.0), ((0.0, float("inf")), 0.0), ((0.0, 0.0), float("nan")), ((1.0, 2.0, 3.0), 0.0)):
        with pytest.raises(ValueError):
            CR.translate(z, shift, dz)
    with pytest.raises(ValueError):
        CR.translate(z[0], (0.0, 0.0))


# ---- the oracle on hand-computed numbers -----------------------------------------------------------------------------------------
def test_oracle_gradient_and_membership_by_hand():
    """z = 2x + 3y on a 4 x 5 grid at gsd (x 0.5, y 2): p = 2 / 0.5 = 4, q = 3 / 2 = 1.5 on the six interior pixels"""
    y, x = np.mgrid[0:4, 0:5].astype(np.float64)
    s = 2.0 * x + 3.0 * y
    g = s + 0.25
    sums, mags = R.shift_sums(s, g, None, 0, -9999.0, 0.5, 2.0)
    np.testing.assert_array_equal(sums, [6, 24, 9, 1.5, 96, 36, 13.5, 6, 2.25, 0.375])
    np.testing.assert_array_equal(mags, sums)
    s2 = s.copy()
    s2[0, 0] = -9999.0                                   # the corner: only pixel (1, 1) has it in its neighbourhood
    assert R.shift_sums(s2, g, None, 0, -9999.0, 0.5, 2.0)[0][0] == 5
    assert R.shift_sums(s2, g, None, 0, float("nan"), 0.5, 2.0)[0][0] == 6      # nodata NaN: no value is nodata
    g2 = g.copy()
    g2[1, 1], g2[2, 3] = np.nan, -9999.0
    assert R.shift_sums(s, g2, None, 0, -9999.0, 0.5, 2.0)[0][0] == 4
    cls = np.zeros((4, 5), np.uint8)
    cls[1, 1:4] = 3
    assert R.shift_sums(s, g, cls, 1, -9999.0, 0.5, 2.0)[0][0] == 3 and R.shift_sums(s, g, cls, 4, -9999.0, 0.5, 2.0)[0][0] == 0
    assert R.shift_sums(s, g, None, 0, -9999.0, 0.5, 2.0, thr=0.2)[0][0] == 0
    assert R.shift_sums(s, g, None, 0, -9999.0, 0.5, 2.0, thr=0.25)[0][0] == 6
    # p^2 + q^2 = 18.25: the cap compares squares
    assert R.shift_sums(s, g, None, 0, -9999.0, 0.5, 2.0, slope_max=math.sqrt(18.25) * (1 + 1e-12))[0][0] == 6
    assert R.shift_sums(s, g, None, 0, -9999.0, 0.5, 2.0, slope_max=4.2)[0][0] == 0
    s3 = s.copy()
    s3[2, 2] = np.inf                                    # every interior pixel of a 4 x 5 raster touches (2, 2) or is it
    assert R.shift_sums(s3, g, None, 0, -9999.0, 0.5, 2.0)[0][0] == 0
    for shape in ((1, 1), (2, 5), (5, 2)):
        np.testing.assert_array_equal(R.shift_sums(np.ones(shape), np.ones(shape), None, 0, -9999.0, 1.0, 1.0)[0], np.zeros(10))


def test_oracle_translate_by_hand():
    s = np.arange(12, dtype=np.float64).reshape(3, 4)
    nan_bits = np.uint64(R.NAN_BITS)
    np.testing.assert_array_equal(R.translate(s, -9999.0, 0.0, 0.0, 0.0, np.nan).view(np.uint64), s.view(np.uint64))
    t = R.translate(s, -9999.0, 1.0, 0.0, 0.5, np.nan)               # the content moves one column to the right
    np.testing.assert_array_equal(t[:, 1:], s[:, :-1] + 0.5)
    assert (t[:, 0].view(np.uint64) == nan_bits).all()
    t = R.translate(s, -9999.0, 0.0, -2.0, 0.0, -1.0)                # two rows up: the last row of the source arrives on top
    np.testing.assert_array_equal(t[0], s[2])
    assert (t[1:] == -1.0).all()
    t = R.translate(s, -9999.0, 0.5, 0.5, 0.0, np.nan)
    assert t[1, 1] == (0 + 1 + 4 + 5) / 4.0 and t[2, 3] == (6 + 7 + 10 + 11) / 4.0 and np.isnan(t[0]).all() and np.isnan(t[:, 0]).all()
    t = R.translate(s, -9999.0, -0.25, 0.75, 0.0, np.nan)            # out(y, x) = src(y - 0.75, x + 0.25)
    assert t[1, 0] == 0.25 + 0.25 * (4.25 - 0.25) and np.isnan(t[:, 3]).all() and np.isnan(t[0]).all()      # fx = fy = 0.25
    s2 = s.copy()
    s2[1, 1] = -9999.0
    t = R.translate(s2, -9999.0, 0.5, 0.0, 0.0, 7.0)                 # taps (y, x - 1) and (y, x)
    assert t[1, 1] == 7.0 and t[1, 2] == 7.0 and t[1, 3] == 6.5 and t[0, 1] == 0.5
    assert (R.translate(s, -9999.0, 4.0, 0.0, 0.0, np.nan).view(np.uint64) == nan_bits).all()
    assert (R.translate(s, -9999.0, 1e300, 0.0, 0.0, -3.0) == -3.0).all()


# ---- the method: a known shift on the analytic surface ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "%dx%d_%g_%g_%g" % c[:5])
def test_oracle_recovers_a_known_shift(case):
    rows, cols, sx, sy, sz, gsd = case
    src, ref = R.shifted_pair(rows, cols, sx, sy, sz)
    px, py, tz, history, converged = R.coregister(src, ref, gsd, gsd, tol=1e-4)
    print(f"{case}: error {px - sx:+.6f} px, {py - sy:+.6f} px, {tz - sz:+.6f} m after {len(history)} iterations")
    assert converged and len(history) <= 6
    assert abs(px - sx) <= R.BAR_PX and abs(py - sy) <= R.BAR_PX and abs(tz - sz) <= R.BAR_M
    if (sx, sy, sz) == (0.0, 0.0, 0.0):
        assert (px, py, tz) == (0.0, 0.0, 0.0) and len(history) == 1     # d is zero everywhere: exact zeros, one iteration


def test_the_slope_cap_is_seen_to_act_on_a_box():
    rows, cols, sx, sy, sz, gsd = R.BOX_CASE
    src, ref = R.shifted_pair(rows, cols, sx, sy, sz, box=True)
    px, py, tz, history, converged = R.coregister(src, ref, gsd, gsd, tol=1e-4, slope_max=math.tan(math.radians(45.0)))
    print(f"capped at 45 degrees: error {px - sx:+.6f} px, {py - sy:+.6f} px, {tz - sz:+.6f} m after {len(history)} iterations")
    assert converged
    assert abs(px - sx) <= R.BAR_PX and abs(py - sy) <= R.BAR_PX and abs(tz - sz) <= R.BAR_M
    ux, uy, uz, uh, _ = R.coregister(src, ref, gsd, gsd, tol=1e-4)
    print(f"without a cap: error {ux - sx:+.6f} px, {uy - sy:+.6f} px, {uz - sz:+.6f} m after {len(uh)} iterations")
    assert math.hypot(ux - sx, uy - sy) > 0.05 and abs(ux - sx) > 0.05


def test_a_plane_and_a_constant_constrain_nothing():
    from resdepth_amd.coregistration import solve_shift
    y, x = np.mgrid[0:32, 0:40].astype(np.float64)
    for s in (0.3 * x - 0.2 * y + 4.0, np.full((32, 40), 7.0)):
        sums, _ = R.shift_sums(s, s + 0.5, None, 0, -9999.0, 1.0, 1.0)
        assert sums[0] == 30 * 38
        with pytest.raises(RuntimeError, match="constrain"):
            R.solve(sums)
        with pytest.raises(RuntimeError, match="constrain"):
            solve_shift(sums, 1.0, 1.0)
    with pytest.raises(RuntimeError, match="three"):
        solve_shift([2, 0, 0, 0, 0, 0, 0, 0, 0, 0], 1.0, 1.0)
    with pytest.raises(RuntimeError):
        R.solve([2, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def test_the_front_ends_solve_is_the_oracles():
    from resdepth_amd.coregistration import solve_shift
    rows, cols, sx, sy, sz, gsd = R.CASES[1]
    src, ref = R.shifted_pair(rows, cols, sx, sy, sz)
    sums, _ = R.shift_sums(src, ref, None, 0, -9999.0, gsd, gsd)
    got, want = solve_shift(sums, gsd, gsd), R.solve(sums)
    a, b, c = np.linalg.solve(np.array([[sums[4], sums[5], sums[1]], [sums[5], sums[6], sums[2]], [sums[1], sums[2], sums[0]]]),
                              np.array([sums[7], sums[8], sums[3]]))
    assert (got.tx, got.ty, got.tz) == (-a, -b, c) == (want["tx"], want["ty"], want["tz"])
    assert got.px == (got.tx / gsd, got.ty / gsd) and got.count == want["count"] == int(sums[0])
    np.testing.assert_array_equal(got.sums, sums)
    np.testing.assert_allclose(got.cov, want["cov"], rtol=1e-9)
    assert got.sigma0 == pytest.approx(want["sigma0"], rel=1e-9) and got.cov.shape == (3, 3)
    # sigma0 against the residuals themselves
    member, ts = R.terms(src, ref, None, 0, -9999.0, gsd, gsd)
    res = ts[2][member] - (a * ts[0][member] + b * ts[1][member] + c)
    assert got.sigma0 == pytest.approx(math.sqrt(float(res @ res) / (member.sum() - 3)), rel=1e-6)
