"""Ortho-rectification without a GPU: the side header include/resdepth_hip_ortho.h against _lib.SIGNATURES_ORTHO, the library's
exports and build.sh; the descriptor's size against the dtype that packs it; the RPC parsers; the argument checks of the front end,
which all come before any launch; and the map projection of the numpy oracle tests/ortho_ref.py (the series the kernel restates)
against anchors that do not depend on the series.

The anchor bar is 1e-6 m: with correct n^4 terms the truncation of the Krueger series is O(n^5 a) ~ 1e-7 m, a wrong n^4
coefficient shows at about 1e-5 m."""
import math
import os
import re

import numpy as np
import pytest

import ortho_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rd_ortho_rpc"}
HEADER = "resdepth_hip_ortho.h"
BAR_M = 1e-6
M_PER_DEG = math.pi / 180.0 * R.A_WGS                  # a metre on the ground is at least 1 / M_PER_DEG degrees of either angle


def _side_header():
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    return text, re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def test_side_header_signatures_constants_and_exports():
    from resdepth_amd import _lib
    main = open(os.path.join(ROOT, "include", "resdepth_hip.h")).read()
    assert main.count('#include "%s"' % HEADER) == 1
    assert main.index('#include "%s"' % HEADER) < main.index("#endif /* RESDEPTH_HIP_H */")
    text, code = _side_header()
    exported = set(re.findall(r"\b(rd_\w+)\s*\(", code))
    assert exported == set(_lib.SIGNATURES_ORTHO) == NAMES
    for name, (_, args) in _lib.SIGNATURES_ORTHO.items():
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1)
        assert len(decl.split(",")) == len(args) == 20, name
    defines = {k: int(v) for k, v in re.findall(r"#define\s+(RD_\w+)\s+(\d+)", code)}
    assert defines["RD_ORTHO_MAX_VIEWS"] == _lib.ORTHO_MAX_VIEWS == 16
    assert {k: defines["RD_ORTHO_" + k.upper().replace("UINT", "U").replace("FLOAT", "F")] for k in _lib.ORTHO_DTYPES} == _lib.ORTHO_DTYPES
    assert {k: defines["RD_ORTHO_" + k.upper()] for k in _lib.ORTHO_CRS} == _lib.ORTHO_CRS == {"geographic": 0, "utm": 1}
    assert {k: defines["RD_ORTHO_" + k.upper()] for k in _lib.ORTHO_RESAMPLING} == _lib.ORTHO_RESAMPLING
    # the header owns up to what is asked of it
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    for phrase in ("Refused:", "Memory: reads", "and nothing else", "launches nothing and writes nothing", "NOT NEEDED",
                   "as doubles", "64-bit", "ortho_rpc_kernel", "overlap", "No atomics", "no scratch buffer",
                   "no data-dependent loop", "same bits on every call", "rounded ONCE to float", "Catmull-Rom",
                   "alignment: none beyond the element's own", "non-temporal", "wave-uniform"):
        assert phrase in flat, phrase
    assert flat.count("Memory: reads") == 1 and flat.count("Refused:") == 1
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.rd_version() == 116                    # the feature is detected by symbol
    # the name lives in this header and this table alone
    inc = os.path.join(ROOT, "include")
    for other in sorted(os.listdir(inc)):
        if other != HEADER:
            body = open(os.path.join(inc, other)).read()
            for name in NAMES:
                assert not re.search(r"\b%s\s*\(" % name, body), (other, name)
    tables = [t for t in dir(_lib) if t.startswith("SIGNATURES") and t != "SIGNATURES_ORTHO"]
    assert len(tables) >= 11
    for table in tables:
        assert not NAMES & set(getattr(_lib, table)), table


def test_the_kernel_lives_in_an_existing_unit_and_launches_through_rd_launch():
    csrc = os.path.join(ROOT, "resdepth_amd", "csrc")
    build = open(os.path.join(csrc, "build.sh")).read()
    units = re.search(r'^UNITS="([^"]*)"$', build, re.M).group(1).split()
    assert len(units) == 12 and "all twelve translation" in build and HEADER in build
    owners = [u for u in units if "rd_ortho_rpc" in open(os.path.join(csrc, u + ".hip")).read()]
    assert owners == ["rd_tiles"]
    code = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "rd_tiles.hip")).read())
    section = code[code.rindex("namespace rd {"):]                    # the last section of the unit
    assert "hipLaunchKernelGGL" not in section and "<<<" not in section and "atomic" not in section.lower()
    assert "__shared__" not in section and "while" not in section
    assert section.count("RD_LAUNCH(ortho_rpc_kernel<") == 3 and section.count("RD_LAUNCH_CHECK(") == 1   # one per resampling
    assert "void ortho_rpc_kernel(" in section and "st_nt1(" in section and "getenv" not in section
    # one footprint is built: no switch between the measured three survives
    assert len(re.findall(r"constexpr int ORTHO_FW = (\d+)", section)) == 1 and "#if" not in section.replace("#ifdef RD_NO_NT", "")


def test_the_descriptor_is_packed_as_the_header_lays_it_out():
    from resdepth_amd import _lib, ortho
    text, code = _side_header()
    assert "} rd_ortho_view; /* 776 bytes */" in text
    assert np.dtype(ortho._VIEW_DESC).itemsize == _lib.ORTHO_VIEW_BYTES == 776
    body = re.search(r"typedef struct rd_ortho_view \{(.*?)\} rd_ortho_view;", code, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [re.sub(r"\[\d+\]|[\s\*]", "", f.split()[-1]) for f in decl.split(",")]
    assert fields == list(ortho._VIEW_DESC.names)                     # the same members in the same order
    off = ortho._VIEW_DESC.fields
    assert (off["image"][1], off["pitch"][1], off["rows"][1], off["dtype"][1], off["line0"][1], off["line_off"][1],
            off["line_num"][1], off["samp_den"][1]) == (0, 8, 16, 24, 32, 56, 136, 616)
    src = open(os.path.join(ROOT, "resdepth_amd", "csrc", "rd_tiles.hip")).read()
    assert "static_assert(sizeof(rd_ortho_view) == 776" in src


# ---- the RPC class -----------------------------------------------------------------------------------------------------------------
def _model(seed=3):
    return R.synthetic_rpc((7.9, 8.1), (47.3, 47.5), (300.0, 700.0), 4000, 5000, seed=seed)


def test_rpc_parsers_round_trip_through_both_text_forms():
    from resdepth_amd import RPC, ortho
    assert ortho.RPC is RPC
    m = _model()
    rpc = RPC(**m)
    for back in (RPC.from_dict(rpc.to_dict()), RPC.from_rpc_txt(rpc.to_rpc_txt()),
                 RPC.from_dict({k: (v.split() if " " in v else float(v)) for k, v in rpc.to_dict().items()})):
        for name in R.SCALARS:
            assert getattr(back, name) == m[name], name
        for name in R.VECTORS:
            np.testing.assert_array_equal(getattr(back, name), m[name])
    txt = rpc.to_rpc_txt()
    assert "LINE_OFF: " in txt and " pixels" in txt and "LAT_OFF" in txt and " degrees" in txt and "SAMP_DEN_COEFF_20: " in txt
    vendor = "LINE_OFF: +004032.00 pixels\nSAMP_OFF: +5000.5 pixels\nLAT_OFF: +47.4000 degrees\nLONG_OFF: +008.0000 degrees\n" \
             "HEIGHT_OFF: +0500.000 meters\nLINE_SCALE: +004033.00 pixels\nSAMP_SCALE: +5001 pixels\nLAT_SCALE: +00.1000 degrees\n" \
             "LONG_SCALE: +000.2 degrees\nHEIGHT_SCALE: +0501.000 meters\n"
    for key in ("LINE_NUM_COEFF", "LINE_DEN_COEFF", "SAMP_NUM_COEFF", "SAMP_DEN_COEFF"):
        vendor += "".join("%s_%d: %+.6E\n" % (key, i, (1.0 if i == 1 else -1.5e-3 * i)) for i in range(1, 21))
    v = RPC.from_rpc_txt(vendor)
    assert (v.line_off, v.samp_off, v.lat_off, v.lon_off, v.height_off) == (4032.0, 5000.5, 47.4, 8.0, 500.0)
    assert (v.line_scale, v.samp_scale, v.lat_scale, v.lon_scale, v.height_scale) == (4033.0, 5001.0, 0.1, 0.2, 501.0)
    assert v.samp_den[0] == 1.0 and v.samp_den[19] == -0.03 and v.line_num[1] == -0.003
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), "ortho_cpu_%d_RPC.TXT" % os.getpid())
    with open(path, "w") as f:
        f.write(vendor)
    try:
        assert RPC.from_rpc_txt(path).line_off == 4032.0
    finally:
        os.remove(path)
    for broken in (vendor.replace("LAT_OFF", "LAT_OF"), vendor.replace("SAMP_NUM_COEFF_7:", "SAMP_NUM_COEFF_77:"),
                   vendor.replace("+0501.000 meters", "+0000.000 meters"), vendor.replace("+5000.5 pixels", "pixels")):
        with pytest.raises(ValueError):
            RPC.from_rpc_txt(broken)
    with pytest.raises(ValueError):
        RPC.from_dict({k: v for k, v in rpc.to_dict().items() if k != "LONG_SCALE"})
    with pytest.raises(ValueError):
        RPC(**dict(m, line_num=np.zeros(19)))
    with pytest.raises(ValueError):
        RPC(**dict(m, lat_off=float("nan")))


def test_rpc_project_is_the_oracles_projection():
    from resdepth_amd import RPC
    m = _model(5)
    rng = np.random.default_rng(0)
    lon, lat, h = rng.uniform(7.9, 8.1, 50), rng.uniform(47.3, 47.5, 50), rng.uniform(300, 700, 50)
    line, samp = RPC(**m).project(lon, lat, h)
    want_line, want_samp = R.rpc_project(m, lon, lat, h)
    np.testing.assert_allclose(line, want_line, rtol=0, atol=1e-8)
    np.testing.assert_allclose(samp, want_samp, rtol=0, atol=1e-8)
    # by hand: at the offsets every normalised coordinate is 0 and the ratio is num[0] / den[0] = 0
    l0, s0 = RPC(**m).project(m["lon_off"], m["lat_off"], m["height_off"])
    assert (float(l0), float(s0)) == (m["line_off"], m["samp_off"])
    # the rows fall as the latitude rises, the image is turned by 30 degrees
    l1, s1 = RPC(**m).project(m["lon_off"], m["lat_off"] + 0.01, m["height_off"])
    assert l1 < l0 and s1 > s0


def test_argument_errors_are_raised_before_any_launch():
    """on a machine without a GPU nothing below can reach a launch: a ValueError means the check came first"""
    import resdepth_amd as pkg
    from resdepth_amd import ortho as O
    assert pkg.orthorectify is O.orthorectify and pkg.project_grid is O.project_grid and pkg.RPC is O.RPC
    rpc = O.RPC(**_model())
    img = np.zeros((8, 9), np.uint16)
    dsm = np.zeros((6, 7), np.float32)
    gt = (8.0, 1e-5, 0.0, 47.4, 0.0, -1e-5)
    good = dict(images=[img], rpcs=[rpc], dsm=dsm, geotransform=gt, crs="geographic")
    nan, inf = float("nan"), float("inf")
    bad_all = [dict(images=[]), dict(images=img), dict(images=[img] * 17, rpcs=[rpc] * 17), dict(images=[img.astype(np.int32)]),
               dict(images=[img.astype(np.float64)]), dict(images=[img[0]]), dict(images=[np.zeros((0, 4), np.uint8)]),
               dict(images=[[[1, 2], [3, 4]]]), dict(rpcs=[rpc, rpc]), dict(rpcs=[_model()]), dict(rpcs=rpc),
               dict(dsm=dsm[0]), dict(dsm=np.zeros((0, 3), np.float32)), dict(dsm=np.zeros((2, 3, 4), np.float32)),
               dict(geotransform=(8.0, 1e-5, 1e-9, 47.4, 0.0, -1e-5)), dict(geotransform=(8.0, 1e-5, 0.0, 47.4, 1e-9, -1e-5)),
               dict(geotransform=(8.0, 0.0, 0.0, 47.4, 0.0, -1e-5)), dict(geotransform=(8.0, 1e-5, 0.0, 47.4, 0.0, 0.0)),
               dict(geotransform=(8.0, nan, 0.0, 47.4, 0.0, -1e-5)), dict(geotransform=(8.0, 1e-5, 0.0, inf, 0.0, -1e-5)),
               dict(geotransform=gt[:5]), dict(geotransform=None), dict(crs="utm"), dict(crs=("utm", 0, "N")),
               dict(crs=("utm", 61, "N")), dict(crs=("utm", 32, "X")), dict(crs=("utm", 32.5, "N")), dict(crs=("utm", 32)),
               dict(crs="EPSG:4326"), dict(height_offset=nan), dict(height_offset=inf), dict(height_offset="x"),
               dict(image_origin=nan), dict(image_origin=[0.0, 0.5]), dict(image_window=(1, 2, 3)), dict(image_window=(nan, 0)),
               dict(image_window=[(0, 0), (1, 1)])]
    bad_ortho = [dict(resampling="cubic"), dict(resampling=1), dict(fill="x"), dict(image_nodata=[0, 0])]
    for fn, cases in ((O.orthorectify, bad_all + bad_ortho), (O.project_grid, bad_all)):
        for bad in cases:
            kw = dict(good, **bad)
            with pytest.raises(ValueError):
                fn(kw.pop("images"), kw.pop("rpcs"), kw.pop("dsm"), kw.pop("geotransform"), kw.pop("crs"), **kw)
    with pytest.raises(ValueError, match="rotated"):
        O.orthorectify([img], [rpc], dsm, (8.0, 1e-5, 1e-9, 47.4, 0.0, -1e-5), "geographic")
    with pytest.raises(ValueError, match="crs"):
        O.orthorectify([img], [rpc], dsm, gt, ("utm", 99, "N"))
    with pytest.raises(ValueError, match="resampling"):
        O.orthorectify([img], [rpc], dsm, gt, "geographic", resampling="lanczos")
    # what the checks let through, as far as it can be seen without a device
    args = O._arguments([img, img[:, ::2]], [rpc, rpc], dsm, gt, ("utm", 32, "S"), None, 47.5, "bicubic", [None, 0], 0.5, (10, 20), -1.0,
                        "t")
    grid, kinds, nd, hoff, rs, fill, inod, origin, window = args
    assert grid == (6, 7, 8.0, 1e-5, 47.4, -1e-5, 1, 9.0, 1.0e7) and math.isnan(nd) and (hoff, rs, fill) == (47.5, 2, -1.0)
    assert kinds == [("uint16", 8, 9, 9), ("uint16", 8, 5, None)] and math.isnan(inod[0]) and inod[1] == 0.0
    assert origin == [0.5, 0.5] and window == [(10.0, 20.0)] * 2
    assert O._grid(dsm, gt, ("utm", 1, "N"), "t")[-2:] == (-177.0, 0.0)


# ---- the projection's anchors, independent of the series -------------------------------------------------------------------------
@pytest.mark.parametrize("lat", [10.0, 47.4, 70.0, -33.0])
def test_the_northing_on_the_central_meridian_is_the_meridian_arc(lat):
    from scipy.integrate import quad
    arc, err = quad(lambda p: R.A_WGS * (1 - R.E2) * (1 - R.E2 * math.sin(p) ** 2) ** -1.5, 0.0, math.radians(lat),
                    epsabs=0.0, epsrel=1e-13)
    assert err < 5e-7                                    # the reference's own error, inside the bar
    east, north = R.utm_forward(9.0, lat, 9.0, 0.0)
    print(f"lat {lat}: northing {float(north):.9f} m, k0 x arc {R.K0 * arc:.9f} m, difference {float(north) - R.K0 * arc:+.3e} m")
    assert abs(float(north) - R.K0 * arc) <= BAR_M and abs(float(east) - 500000.0) <= BAR_M
    lon, back = R.utm_inverse(500000.0, R.K0 * arc, 9.0, 0.0)
    assert abs(float(back) - lat) * M_PER_DEG <= BAR_M and abs(float(lon) - 9.0) * M_PER_DEG <= BAR_M


def test_forward_then_inverse_returns_the_angles():
    lat, dlon = np.meshgrid(np.linspace(-80.0, 80.0, 81), np.linspace(-3.0, 3.0, 25), indexing="ij")
    for lon0, fn in ((9.0, 0.0), (-177.0, 1.0e7)):
        east, north = R.utm_forward(lon0 + dlon, lat, lon0, fn)
        lon, back = R.utm_inverse(east, north, lon0, fn)
        worst_lat = float(np.abs(back - lat).max()) * M_PER_DEG
        worst_lon = float((np.abs(lon - lon0 - dlon) * np.cos(np.radians(lat))).max()) * M_PER_DEG
        print(f"lon0 {lon0}: worst round trip {worst_lat:.3e} m in latitude, {worst_lon:.3e} m in longitude")
        assert worst_lat <= BAR_M and worst_lon <= BAR_M
    # the n^4 terms are seen by this bar: without them the round trip misses it
    east, north = R.utm_forward(9.0 + dlon, lat, 9.0, 0.0)
    lon3, lat3 = R.utm_inverse(east, north, 9.0, 0.0, terms=3)
    assert float(np.abs(lat3 - lat).max()) * M_PER_DEG > BAR_M
    # a known point: 8.55 E, 47.37 N in zone 32 N lies west of the central meridian at about 5.25e6 m north
    e1, n1 = R.utm_forward(8.55, 47.37, 9.0, 0.0)
    assert 465000 < float(e1) < 467000 and 5246000 < float(n1) < 5247500


# ---- the resamplers of the oracle by hand -------------------------------------------------------------------------------------------
def test_oracle_resamplers_by_hand():
    img = np.arange(20, dtype=np.float32).reshape(4, 5)
    y = np.array([0.0, 3.0, 3.0, 1.5, -0.25, 1.0, 3.25, np.nan, np.inf, 1.0])
    x = np.array([0.0, 4.0, 4.25, 2.5, 0.0, 4.0, 0.0, 1.0, 1.0, 1e300])
    val, ok, mag = R.resample(img, None, y, x, "bilinear")
    np.testing.assert_array_equal(ok, [1, 1, 0, 1, 0, 1, 0, 0, 0, 0])
    np.testing.assert_array_equal(val[:6], [0.0, 19.0, 0.0, 10.0, 0.0, 9.0])            # (1.5, 2.5): (7 + 8 + 12 + 13) / 4
    assert mag[3] == 10.0 and mag[1] == 19.0
    val, ok, _ = R.resample(img, None, y, x, "nearest")
    np.testing.assert_array_equal(ok, [1, 1, 1, 1, 1, 1, 1, 0, 0, 0])
    np.testing.assert_array_equal(val[:7], [0.0, 19.0, 19.0, 13.0, 0.0, 9.0, 15.0])     # 0.5 rounds up, -0.25 to row 0
    val, ok, mag = R.resample(img, None, y, x, "bicubic")
    np.testing.assert_array_equal(ok, [1, 1, 0, 1, 0, 1, 0, 0, 0, 0])                   # (1.5, 2.5) has rows 0..3, columns 1..4
    assert val[0] == 0.0 and val[1] == 19.0 and val[5] == 9.0 and val[3] == pytest.approx(10.0, abs=1e-12)   # a plane is kept
    assert mag[3] > 10.0                                                                # negative lobes
    w = R._cubic(np.float64(0.5))
    assert w == [-0.0625, 0.5625, 0.5625, -0.0625] and R._cubic(np.float64(0.0)) == [0.0, 1.0, 0.0, 0.0]
    # nodata: only NEEDED taps count
    val, ok, _ = R.resample(img, 8.0, np.array([1.0, 1.0, 1.5, 2.0]), np.array([2.0, 3.0, 3.0, 2.5]), "bilinear")
    np.testing.assert_array_equal(ok, [1, 0, 0, 1])
    val, ok, _ = R.resample(img, 8.0, np.array([2.0, 1.0, 1.5]), np.array([2.0, 2.5, 1.5]), "bicubic")
    np.testing.assert_array_equal(ok, [1, 0, 0])
    u16 = (np.arange(20).reshape(4, 5) * 3000).astype(np.uint16)
    val, ok, _ = R.resample(u16, 0, np.array([0.0, 1.0]), np.array([0.0, 1.0]), "nearest")
    assert not ok[0] and ok[1] and val[1] == 18000.0


def test_integer_rpc_lands_on_integers_exactly():
    step = 2.0 ** -10
    m = R.integer_rpc(8.0, 47.0, step, 30, -10)
    gt = (8.0 - 0.5 * step, step, 47.0 + 0.5 * step, -step)
    c, defined = R.coords(np.zeros((70, 130), np.float32), -9999.0, gt, "geographic", 0.0, 0.0, 0.0, [m], [(0.0, 0.0)])
    r_, c_ = np.mgrid[0:70, 0:130]
    np.testing.assert_array_equal(c[0, ..., 0], r_ + 30.0)
    np.testing.assert_array_equal(c[0, ..., 1], c_ - 10.0)
    assert defined.all()
