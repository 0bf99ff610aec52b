"""Ortho-rectification on the GPU (rd_ortho_rpc through resdepth_amd.ortho) against the numpy fp64 oracle tests/ortho_ref.py.

The bars.  Coordinates: 1e-6 px -- operands normalised to [-1, 1], about 100 fp64 operations, scales <= 1e5: a first-order rounding
estimate of <= 5e-8 px, of which the UTM inverse contributes about 1e-8 at 0.25 m pixels; the bar is 20 x that and the measured
maximum is printed (a value above 1e-7 is to be explained, not absorbed; measured on one MI355X: 2.8e-14 px on the geographic
grid, 2.2e-8 px on the UTM grids).  Resampling: the oracle's resamplers are evaluated AT
THE KERNEL'S OWN coords, so floor, rounding, bounds and the needed-tap rule are functions of identical fp64 inputs: valid must be
equal everywhere, and |out - oracle| <= 2^-23 sum |w v| -- one float rounding of a sum whose fp64 evaluation may differ by
contraction."""
import numpy as np
import pytest
import torch

import ortho_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NODATA, FILL = -9999.0, -7.0
ROWS, COLS = 70, 130
KINDS = ("nearest", "bilinear", "bicubic")
GRIDS = {
    "geographic": dict(gt=(8.0, 1.0e-5, 0.0, 47.4, 0.0, -1.0e-5), crs="geographic", lon0=0.0, fn=0.0),
    "utm": dict(gt=(465000.0, 0.25, 0.0, 5247000.0, 0.0, -0.25), crs=("utm", 32, "N"), lon0=9.0, fn=0.0),
    "utm_south": dict(gt=(612345.5, 0.5, 0.0, 6250000.25, 0.0, -0.5), crs=("utm", 56, "S"), lon0=153.0, fn=1.0e7),
}


def _gt4(gt):
    return (gt[0], gt[1], gt[3], gt[5])


def _dsm(rows, cols, seed=1):
    """heights that are multiples of 1/64 below 1024 (a constant can be added exactly), 5 % nodata, one NaN"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:rows, 0:cols]
    z = np.round((400.0 + 30.0 * np.sin(y / 9.0) * np.cos(x / 13.0) + rng.uniform(-2, 2, (rows, cols))) * 64.0) / 64.0
    z = z.astype(np.float32)
    z[rng.uniform(size=(rows, cols)) < 0.05] = NODATA
    if rows * cols > 1:
        z[rows // 2, cols // 3] = np.nan
    return z


def _images():
    rng = np.random.default_rng(7)
    a = rng.integers(1, 60000, (96, 80)).astype(np.uint16)
    a[rng.uniform(size=a.shape) < 0.03] = 0                       # this image's nodata
    b = rng.integers(0, 256, (50, 61)).astype(np.uint8)
    wide = rng.normal(100.0, 40.0, (64, 100)).astype(np.float32)
    return a, b, wide


def _models(grid, rows, cols, shapes, n=None):
    lon, lat = R.ground(rows, cols, _gt4(grid["gt"]), "geographic" if grid["crs"] == "geographic" else "utm", grid["lon0"], grid["fn"])
    lon_r, lat_r = (float(lon.min()), float(lon.max())), (float(lat.min()), float(lat.max()))
    # a single row or column: the model keeps a scale of at least 1e-4 degrees (about 11 m).  A lat_scale of 2e-6 degrees, the
    # meridian convergence across a 1 x 257 grid at 0.25 m, turns the few ulps of a latitude near 47 degrees into 6e-7 px (measured)
    widen = lambda r: r if r[1] - r[0] >= 1e-4 else (0.5 * (r[0] + r[1]) - 5e-5, 0.5 * (r[0] + r[1]) + 5e-5)      # noqa: E731
    lon_r, lat_r = widen(lon_r), widen(lat_r)
    return [R.synthetic_rpc(lon_r, lat_r, (350.0, 450.0), r, c, angle_deg=30.0 + 5.0 * i, zoom=1.15 - 0.1 * (i % 3),
                            shift=(3.0 * (i % 4), -2.0 * (i % 5)), seed=10 + i) for i, (r, c) in enumerate(shapes)]


@pytest.fixture(scope="module")
def scene():
    from resdepth_amd import RPC
    a, b, wide = _images()
    wide_t = torch.from_numpy(wide).to(DEV)
    images = [torch.from_numpy(a.view(np.int16)).to(DEV).view(torch.uint16), b, wide_t[:, 10:74]]      # device, host, strided
    assert images[2].stride(0) == 100 and not images[2].is_contiguous()
    host = [a, b, wide[:, 10:74]]
    inod = [0, None, None]
    s = dict(images=images, host=host, inod=inod, dsm=_dsm(ROWS, COLS), RPC=RPC)
    for name, g in GRIDS.items():
        s[name] = _models(g, ROWS, COLS, [h.shape for h in host])
    return s


def _call(s, grid_name, kind="bilinear", dsm=None, models=None, images=None, inod=None, **kw):
    from resdepth_amd import orthorectify
    g = GRIDS[grid_name]
    models = s[grid_name] if models is None else models
    return orthorectify(s["images"] if images is None else images, [s["RPC"](**m) for m in models], s["dsm"] if dsm is None else dsm,
                        g["gt"], g["crs"], nodata=NODATA, resampling=kind, image_nodata=s["inod"] if inod is None else inod,
                        fill=FILL, **kw)


def _want_coords(s, grid_name, dsm=None, models=None, height_offset=0.0, origins=None):
    g = GRIDS[grid_name]
    models = s[grid_name] if models is None else models
    return R.coords(s["dsm"] if dsm is None else dsm, NODATA, _gt4(g["gt"]), "geographic" if g["crs"] == "geographic" else "utm",
                    g["lon0"], g["fn"], height_offset, models, origins or [(0.0, 0.0)] * len(models))


# ---- coordinates --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid_name", list(GRIDS))
@pytest.mark.parametrize("shape", [(ROWS, COLS), (1, 1), (1, 257)], ids=lambda s: "%dx%d" % s)
def test_coordinates_against_the_oracle(scene, grid_name, shape):
    from resdepth_amd import project_grid
    g = GRIDS[grid_name]
    dsm = scene["dsm"] if shape == (ROWS, COLS) else _dsm(*shape, seed=5)
    if shape == (1, 1):
        dsm = np.full((1, 1), 412.5, np.float32)
    models = scene[grid_name] if shape == (ROWS, COLS) else _models(g, shape[0], shape[1], [h.shape for h in scene["host"]])
    got = project_grid(scene["images"], [scene["RPC"](**m) for m in models], dsm, g["gt"], g["crs"], nodata=NODATA).cpu().numpy()
    want, defined = _want_coords(scene, grid_name, dsm=dsm, models=models)
    assert got.shape == want.shape == (3,) + shape + (2,)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    assert (np.isnan(got[..., 0]) == ~defined[None]).all()
    worst = float(np.nanmax(np.abs(got - want)))
    print(f"coords {grid_name} {shape}: worst |kernel - oracle| = {worst:.3e} px")
    assert worst <= 1e-6


def test_coordinates_with_an_origin_and_a_window(scene):
    from resdepth_amd import project_grid
    g = GRIDS["utm"]
    rpcs = [scene["RPC"](**m) for m in scene["utm"]]
    got = project_grid(scene["images"], rpcs, scene["dsm"], g["gt"], g["crs"], nodata=NODATA, image_origin=0.5,
                       image_window=[(0, 0), (3, 5), (10.5, 0.25)], height_offset=-2.5).cpu().numpy()
    want, _ = _want_coords(scene, "utm", height_offset=-2.5, origins=[(0.5, 0.5), (3.5, 5.5), (11.0, 0.75)])
    assert float(np.nanmax(np.abs(got - want))) <= 1e-6


# ---- resampling: decisions exact ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid_name", ["geographic", "utm"])
@pytest.mark.parametrize("kind", KINDS)
def test_resampling_at_the_kernels_own_coordinates(scene, kind, grid_name):
    out, valid, coords = _call(scene, grid_name, kind, return_valid=True, return_coords=True)
    assert out.dtype == torch.float32 and valid.dtype == torch.bool and coords.dtype == torch.float64
    assert out.shape == valid.shape == (3, ROWS, COLS) and coords.shape == (3, ROWS, COLS, 2) and out.device.type == "cuda"
    out, valid, coords = out.cpu().numpy(), valid.cpu().numpy(), coords.cpu().numpy()
    for v, (img, nd) in enumerate(zip(scene["host"], scene["inod"])):
        val, ok, mag = R.resample(img, nd, coords[v, ..., 0], coords[v, ..., 1], kind)
        np.testing.assert_array_equal(valid[v], ok)                  # everywhere, no exclusions
        assert 0.15 < ok.mean() < 0.9, (v, ok.mean())                # partly off the image
        assert (out[v][~ok] == np.float32(FILL)).all()
        err = np.abs(out[v].astype(np.float64) - val)[ok]
        bound = (2.0 ** -23 * mag)[ok]
        print(f"{kind} {grid_name} view {v} ({img.dtype}): worst error / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert (err <= bound).all()
    # the u16 view has nodata taps inside the image: they show
    c0 = coords[0]
    inside = (c0[..., 0] > 2) & (c0[..., 0] < 93) & (c0[..., 1] > 2) & (c0[..., 1] < 77)
    assert (inside & ~valid[0]).any()


# ---- exact positions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_integer_positions_return_the_image_bit_for_bit(scene, kind):
    from resdepth_amd import orthorectify
    step = 2.0 ** -10
    gt = (8.0 - 0.5 * step, step, 0.0, 47.0 + 0.5 * step, 0.0, -step)
    dsm = np.zeros((ROWS, COLS), np.float32)
    offs = [(30, -10), (-25, 20), (0, 0)]
    rpcs = [scene["RPC"](**R.integer_rpc(8.0, 47.0, step, ol, os_)) for ol, os_ in offs]
    out, valid = orthorectify(scene["images"], rpcs, dsm, gt, "geographic", resampling=kind, fill=FILL, return_valid=True)
    out, valid = out.cpu().numpy(), valid.cpu().numpy()
    r, c = np.mgrid[0:ROWS, 0:COLS]
    for v, ((ol, os_), img) in enumerate(zip(offs, scene["host"])):
        yi, xi = r + ol, c + os_
        ok = (yi >= 0) & (yi <= img.shape[0] - 1) & (xi >= 0) & (xi <= img.shape[1] - 1)   # the last row and column included
        assert ok.any() and not ok.all()
        np.testing.assert_array_equal(valid[v], ok)
        want = np.where(ok, img[np.clip(yi, 0, img.shape[0] - 1), np.clip(xi, 0, img.shape[1] - 1)].astype(np.float32), np.float32(FILL))
        np.testing.assert_array_equal(out[v].view(np.uint32), want.view(np.uint32))
    assert valid[0][65, 89] and not valid[0][66, 89] and not valid[0][65, 90]               # image[95, 79], then one further


# ---- end to end without the oracle's sampler ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid_name", ["geographic", "utm_south"])
def test_a_linear_ramp_is_reproduced_at_the_oracles_coordinates(scene, grid_name):
    a, b, c = 10.0, 0.25, 0.5
    yy, xx = np.mgrid[0:200, 0:300]
    ramp = (a + b * yy + c * xx).astype(np.float32)
    assert (ramp.astype(np.float64) == a + b * yy + c * xx).all()
    models = _models(GRIDS[grid_name], ROWS, COLS, [ramp.shape])
    out, valid = _call(scene, grid_name, "bilinear", models=models, images=[ramp], inod=[None], return_valid=True)
    out, valid = out.cpu().numpy()[0], valid.cpu().numpy()[0]
    want, defined = _want_coords(scene, grid_name, models=models)
    yi, xi = want[0, ..., 0], want[0, ..., 1]
    with np.errstate(invalid="ignore"):
        surely_in = defined & (yi > 1e-6) & (yi < 199 - 1e-6) & (xi > 1e-6) & (xi < 299 - 1e-6)
        surely_out = ~defined | (yi < -1e-6) | (yi > 199 + 1e-6) | (xi < -1e-6) | (xi > 299 + 1e-6)
    assert valid[surely_in].all() and not valid[surely_out].any() and 0.15 < valid.mean() < 0.9
    value = a + b * yi[valid] + c * xi[valid]
    err = np.abs(out[valid].astype(np.float64) - value)
    bound = np.spacing(np.abs(value).astype(np.float32)).astype(np.float64) + 1e-6 * (abs(b) + abs(c))
    print(f"ramp {grid_name}: worst error {float(err.max()):.3e}, worst error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()


# ---- other checks -------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.cpu().numpy().view(np.uint32 if t.dtype == torch.float32 else np.uint8)


@pytest.mark.parametrize("kind", KINDS)
def test_the_optional_outputs_change_no_bit_and_two_calls_agree(scene, kind):
    plain = _call(scene, "utm", kind)
    again = _call(scene, "utm", kind)
    out_v, valid = _call(scene, "utm", kind, return_valid=True)
    out_c, coords = _call(scene, "utm", kind, return_coords=True)
    out_vc, valid2, coords2 = _call(scene, "utm", kind, return_valid=True, return_coords=True)
    for other in (again, out_v, out_c, out_vc):
        np.testing.assert_array_equal(_bits(plain), _bits(other))
    assert torch.equal(valid, valid2) and torch.equal(coords.view(torch.int64), coords2.view(torch.int64))


def test_sixteen_views(scene):
    three, valid3 = _call(scene, "geographic", "bicubic", return_valid=True)
    order = [i % 3 for i in range(16)]
    out, valid = _call(scene, "geographic", "bicubic", models=[scene["geographic"][i] for i in order],
                       images=[scene["images"][i] for i in order], inod=[scene["inod"][i] for i in order], return_valid=True)
    assert out.shape == (16, ROWS, COLS)
    for v, i in enumerate(order):
        np.testing.assert_array_equal(_bits(out[v]), _bits(three[i]))
        assert torch.equal(valid[v], valid3[i])


def test_a_view_off_the_grid_is_all_fill(scene):
    models = [dict(scene["utm"][0], line_off=scene["utm"][0]["line_off"] + 1.0e4), scene["utm"][1]]
    out, valid = _call(scene, "utm", "bilinear", models=models, images=scene["images"][:2], inod=scene["inod"][:2], return_valid=True)
    assert not bool(valid[0].any()) and bool((out[0] == FILL).all()) and bool(valid[1].any())


def test_height_offset_is_a_constant_added_to_the_dsm(scene):
    dsm = scene["dsm"]
    lifted = np.where((dsm == NODATA) | np.isnan(dsm), dsm, dsm + np.float32(12.5)).astype(np.float32)
    assert (lifted.astype(np.float64)[dsm > 0] == dsm.astype(np.float64)[dsm > 0] + 12.5).all()      # exact in float32
    a, va, ca = _call(scene, "utm", "bilinear", height_offset=12.5, return_valid=True, return_coords=True)
    b, vb, cb = _call(scene, "utm", "bilinear", dsm=lifted, return_valid=True, return_coords=True)
    np.testing.assert_array_equal(_bits(a), _bits(b))
    assert torch.equal(va, vb) and torch.equal(ca.view(torch.int64), cb.view(torch.int64))
    plain = _call(scene, "utm", "bilinear")
    assert not torch.equal(plain, a)                                 # the height is seen: the H terms of the models


def test_a_crop_with_its_window_equals_the_scene_on_the_overlap(scene):
    r0, c0 = 17, 9
    crops = [scene["images"][0][r0:, c0:], scene["host"][1][r0:, c0:], scene["images"][2][r0:, c0:]]
    for kind in KINDS:
        full, vf, cf = _call(scene, "geographic", kind, return_valid=True, return_coords=True)
        crop, vc, cc = _call(scene, "geographic", kind, images=crops, image_window=(r0, c0), return_valid=True, return_coords=True)
        shift = torch.tensor([float(r0), float(c0)], dtype=torch.float64, device=cf.device)
        same = (cc == cf - shift) | (torch.isnan(cc) & torch.isnan(cf))
        assert bool(same.all())
        assert bool((vf | ~vc).all()) and int(vc.sum()) > 500 and int((vf & ~vc).sum()) > 50
        assert torch.equal(crop[vc], full[vc])


def test_offsets_beyond_2_to_the_31_elements(scene):
    from resdepth_amd import orthorectify
    side = 46400                                                     # 2.15e9 elements
    assert side * side > 2 ** 31
    big = torch.zeros((side, side), dtype=torch.uint8, device=DEV)
    pattern = torch.from_numpy(np.random.default_rng(3).integers(1, 256, (40, 40)).astype(np.uint8)).to(DEV)
    big[side - 40:, side - 40:] = pattern
    step = 2.0 ** -10
    gt = (8.0 - 0.5 * step, step, 0.0, 47.0 + 0.5 * step, 0.0, -step)
    rpc = scene["RPC"](**R.integer_rpc(8.0, 47.0, step, side - 32, side - 32))
    try:
        for kind in KINDS:
            out, valid = orthorectify([big], [rpc], np.zeros((32, 32), np.float32), gt, "geographic", resampling=kind,
                                      image_nodata=0, fill=FILL, return_valid=True)
            assert bool(valid.all()), kind
            assert torch.equal(out[0], pattern[8:, 8:].float()), kind
    finally:
        del big
        torch.cuda.empty_cache()


# ---- the front end ------------------------------------------------------------------------------------------------------------------
def test_the_result_feeds_the_patch_sampler_and_the_grid_tiles(scene):
    from resdepth_amd import GpuGridTiles, GpuPatchSampler
    out = _call(scene, "utm", "bilinear", models=scene["utm"][:2], images=scene["images"][:2], inod=scene["inod"][:2])
    assert out.shape == (2, ROWS, COLS) and out.is_contiguous()
    dsm = np.where(np.isnan(scene["dsm"]), NODATA, scene["dsm"]).astype(np.float32)
    smp = GpuPatchSampler(torch.from_numpy(dsm).to(DEV), None, out, tile_size=32, nodata=NODATA)
    tiles = GpuGridTiles(smp, "test", {"x_extent": [(0, COLS - 1)], "y_extent": [(0, ROWS - 1)]}, "geom-stereo", [[0, 1]],
                         transform_orthos=False, batch_size=4)
    n = min(4, len(tiles.dataset))
    batch = tiles.assemble(0, n)
    assert batch["input"].shape == (n, 3, 32, 32)
    for k in range(n):
        y, x = (int(v) for v in tiles.dataset.pos[k])
        assert torch.equal(batch["input"][k, 1:], out[:, y:y + 32, x:x + 32])


def test_bad_arguments_raise_with_a_device_present(scene):
    from resdepth_amd import orthorectify
    g = GRIDS["geographic"]
    rpcs = [scene["RPC"](**m) for m in scene["geographic"]]
    with pytest.raises(ValueError, match="rotated"):
        orthorectify(scene["images"], rpcs, scene["dsm"], (8.0, 1e-5, 1e-7, 47.4, 0.0, -1e-5), g["crs"])
    with pytest.raises(ValueError, match="images"):
        orthorectify([torch.zeros((4, 4), dtype=torch.int32, device=DEV)], rpcs[:1], scene["dsm"], g["gt"], g["crs"])
