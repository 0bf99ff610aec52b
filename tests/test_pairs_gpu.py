"""All image pairs of a raster in one sweep: GpuGridTiles(sweep_pairs=True), the blend into planes
(rd_blend_accumulate_planes), the per-pixel fusion (rd_fuse_planes) and predict_pairs_linear_blend.  The yardsticks are
today's single-pair sweep (predict_linear_blend over a loader of ONE pair), rd_blend_accumulate_tta on a plane's samples alone
and float64 host loops / np.median; everything but the standard deviation is compared bit for bit.

Scene (tests/test_tta_gpu.py's): 88 x 120 raster (no side a multiple of the stride), tile 32, strides 16 (35 tiles) and 24
(clamped last tiles), FOUR ortho planes, scattered nodata in the input DSM and one 32 x 32 block of nodata on a grid position
of both strides (a tile with a NaN mean, in every plane)."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, T = 88, 120, 32
AREA = {"x_extent": [(0, W - 1)], "y_extent": [(0, H - 1)]}
NODATA, DSM_STD, OSTD = -9999.0, 3.0, 50.0
PAIRS = {1: [[0, 1]], 3: [[0, 1], [1, 2], [0, 3]], 4: [[0, 1], [1, 2], [0, 3], [2, 3]]}     # P = 3: pairs sharing a plane


@pytest.fixture(scope="module")
def rasters():
    rng = np.random.default_rng(17)
    dsm = (400.0 + 5.0 * rng.standard_normal((H, W))).astype(np.float32)
    dsm[rng.random((H, W)) < 0.03] = NODATA
    dsm[48:80, 48:80] = NODATA                      # tile (48, 48) of both strides: all nodata
    orthos = (110.0 + 40.0 * rng.standard_normal((4, H, W))).astype(np.float32)
    return dsm, orthos


def _sampler(rasters, gt=False):
    from resdepth_amd import GpuPatchSampler
    dsm, orthos = rasters
    return GpuPatchSampler(dsm, dsm.copy() if gt else None, orthos, tile_size=T, nodata=NODATA, dsm_std=DSM_STD, ortho_mean=110.0,
                           ortho_std=OSTD)


def _loader(rasters, pairs, stride=16, **kw):
    from resdepth_amd import GpuGridTiles
    return GpuGridTiles(_sampler(rasters), "test", AREA, "geom-stereo", pairs, stride=stride, **kw)


def _collect(loader):
    out = {}
    for b in loader:
        for k, v in b.items():
            out.setdefault(k, []).append(v.cpu())
    return {k: torch.cat(v).numpy() for k, v in out.items()}


@pytest.fixture(scope="module")
def model():
    from resdepth_amd import UNet
    torch.manual_seed(5)
    m = UNet(n_input_channels=3, start_kernel=8, depth=2, bias_conv_layer=True)
    g = torch.Generator().manual_seed(6)
    sd = m.state_dict()
    for k in sd:                                    # eval-mode BN with statistics that matter
        if k.endswith("running_mean"):
            sd[k] = torch.randn(sd[k].shape, generator=g) * 0.1
        elif k.endswith("running_var"):
            sd[k] = torch.rand(sd[k].shape, generator=g) + 0.5
    m.load_state_dict(sd)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def single(rasters, model):
    """today's route, computed once per (pair, stride, tta): predict_linear_blend over a loader of that pair alone"""
    from resdepth_amd import predict_linear_blend
    cache = {}

    def get(pair, stride, tta=None):
        key = (tuple(pair), stride, tta)
        if key not in cache:
            cache[key] = np.array(predict_linear_blend(_loader(rasters, [list(pair)], stride, batch_size=16, tta=tta), model))
        return cache[key]
    return get


@pytest.fixture(scope="module")
def swept(rasters, model):
    """one-pass sweeps, computed once per argument set"""
    from resdepth_amd import predict_pairs_linear_blend
    cache = {}

    def get(p, stride, batch, tta=None, fuse="median", spread=None, return_pairs=True):
        key = (p, stride, batch, tta, fuse, spread, return_pairs)
        if key not in cache:
            ld = _loader(rasters, PAIRS[p], stride, batch_size=batch, tta=tta, sweep_pairs=True)
            cache[key] = predict_pairs_linear_blend(ld, model, fuse=fuse, spread=spread, return_pairs=return_pairs)
        return cache[key]
    return get


# ---- host references of rd_fuse_planes ---------------------------------------------------------------------------------------
def _ref_fuse(v, fuse, spread):
    """v: float64 [P, n] -> (fused, spread or None): the order rules of include/resdepth_hip_pairs.h as float64 host loops"""
    p = v.shape[0]
    nan = np.isnan(v).any(axis=0)
    with np.errstate(invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        acc = v[0].copy()
        for k in range(1, p):
            acc = acc + v[k]
        mean = acc / p
        fused = mean if fuse == "mean" else np.median(v, axis=0)
        out = None
        if spread == "range":
            out = v.max(axis=0) - v.min(axis=0)
        elif spread == "std":
            ss = np.zeros_like(mean)
            for k in range(p):
                d = v[k] - mean
                ss = ss + d * d
            out = np.sqrt(ss / p)
    fused = np.where(nan, np.nan, fused)
    if out is not None:
        out = np.where(nan, np.nan, out)
    return fused, out


def _same(got, want, what):
    assert np.array_equal(got, want, equal_nan=True), what
    ok = ~np.isnan(want)
    nz = ok & (want != 0)
    assert np.array_equal(got[nz].view(np.int64), want[nz].view(np.int64)), what     # bit for bit (the sign of a zero aside)


def _check_fuse(got_f, got_s, v, fuse, spread, what):
    want_f, want_s = _ref_fuse(v, fuse, spread)
    assert np.array_equal(np.isnan(got_f), np.isnan(v).any(axis=0)), what          # NaN exactly where any plane is NaN
    _same(got_f, want_f, (what, fuse))
    if spread is None:
        assert got_s is None
    elif spread == "range":
        _same(got_s, want_s, (what, spread))
    else:
        assert np.array_equal(np.isnan(got_s), np.isnan(want_s)), what
        ok = ~np.isnan(want_s)
        assert np.allclose(got_s[ok], want_s[ok], rtol=1e-12, atol=0.0), (what, float(np.abs(got_s[ok] - want_s[ok]).max()))


# ---- 0. the loader ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,stride,tta,swap", [(3, 16, None, False), (4, 24, None, False), (3, 24, "flips", False), (3, 16, [0, 9], True)])
def test_loader_repeats_every_tile_once_per_pair(rasters, p, stride, tta, swap):
    from resdepth_amd import tiling
    pairs = PAIRS[p]
    ld = _loader(rasters, pairs, stride, batch_size=7, sweep_pairs=True, tta=tta, tta_swap_views=swap)
    got = _collect(ld)
    ds = ld.dataset
    g = len(ds.tta) if ds.tta else 1
    alone = [_collect(_loader(rasters, [pr], stride, batch_size=16, tta=tta, tta_swap_views=swap)) for pr in pairs]
    tiles = alone[0]["input"].shape[0] // g
    assert ds.n_pairs == p and ds.image_pairs == pairs and len(ds) == tiles * p * g == got["input"].shape[0]
    assert got["pair"].dtype == np.int32 and got["pair"].tolist() == list(ds.pair_idx) == [k for _ in range(tiles) for k in range(p)
                                                                                            for _ in range(g)]
    assert "target" not in got and "loss_mask" not in got
    if tta is not None:
        assert got["tta"].tolist() == list(tiling.tta_codes(tta)) * (2 if swap else 1) * (tiles * p)
    # column 6 of the sample table: the pair row, plus n_pairs for a swapped sample
    col6 = ld._table[:len(ds), 6].cpu().tolist()
    assert col6 == [k + p * s for k, s in zip(ds.pair_idx, ds.tta_swap or [0] * len(ds))]
    for i in range(tiles):
        for k in range(p):
            a, b = (i * p + k) * g, i * g
            for key in ("input", "dsm_mean", "patch_offset_y", "patch_offset_x", "patch_valid_pixels_uly", "patch_valid_pixels_lrx"):
                assert np.array_equal(got[key][a:a + g], alone[k][key][b:b + g], equal_nan=True), (key, i, k)


def test_without_sweep_pairs_the_loader_is_todays(rasters):
    ld = _loader(rasters, PAIRS[3], batch_size=16)
    assert ld.dataset.n_pairs is None and ld.dataset.image_pairs is None and not ld.sweep_pairs
    assert len(ld.dataset) == 35 and list(ld.dataset.pair_idx) == [0] * 35
    b = next(iter(ld))
    assert "pair" not in b and b["input"].shape == (16, 3, T, T)
    one = next(iter(_loader(rasters, PAIRS[1], batch_size=16)))
    assert torch.equal(b["input"].view(torch.int32), one["input"].view(torch.int32))         # pair 0 at every position


def test_ground_truth_is_not_read_and_says_so(rasters):
    from resdepth_amd import GpuGridTiles
    with pytest.warns(UserWarning, match="no target / loss_mask"):
        ld = GpuGridTiles(_sampler(rasters, gt=True), "test", AREA, "geom-stereo", PAIRS[3], sweep_pairs=True, batch_size=8)
    b = next(iter(ld))
    assert "target" not in b and "loss_mask" not in b and "pair" in b


# ---- 1. plane identity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [5, 32])
@pytest.mark.parametrize("stride", [16, 24])
@pytest.mark.parametrize("p", [1, 3, 4])
def test_every_plane_is_todays_single_pair_sweep(swept, single, p, stride, batch):
    res = swept(p, stride, batch)
    assert res.pairs.shape == (p, H, W) and res.pairs.dtype == np.float64 and res.image_pairs == PAIRS[p]
    for k, pair in enumerate(PAIRS[p]):
        want = single(pair, stride)
        assert np.isnan(want).any() and not np.isnan(want).all()
        assert np.array_equal(res.pairs[k], want, equal_nan=True), (k, pair)
    if p > 1:
        assert not np.array_equal(res.pairs[0], res.pairs[1], equal_nan=True)


@pytest.mark.parametrize("batch", [5, 32])
@pytest.mark.parametrize("stride", [16, 24])
def test_every_plane_is_todays_single_pair_sweep_under_tta(swept, single, stride, batch):
    res = swept(3, stride, batch, tta="flips")
    for k, pair in enumerate(PAIRS[3]):
        assert np.array_equal(res.pairs[k], single(pair, stride, "flips"), equal_nan=True), (k, pair)
    assert not np.array_equal(res.pairs[0], single(PAIRS[3][0], stride), equal_nan=True)


# ---- 2. the blend into planes ------------------------------------------------------------------------------------------------
NB, NP = 130, 3


@pytest.fixture(scope="module")
def blend_case():
    """130 samples (two launch splits at 64 and 128): the 35 stride-16 tiles four times over -- overlapping tiles and repeated
    positions, so the per-pixel order matters --, random predictions / means / orientation codes, planes round-robin"""
    from resdepth_amd import tiling
    _, pos, reg, _ = tiling.grid_samples(AREA["x_extent"], AREA["y_extent"], T, "test", 16)
    pos, reg = (pos * 4)[:NB], (reg * 4)[:NB]
    g = torch.Generator().manual_seed(9)
    pred = torch.randn(NB, 1, T, T, generator=g)
    mean = 400.0 + torch.randn(NB, generator=g)
    std = torch.full((NB,), DSM_STD)
    aug = torch.randint(0, 16, (NB,), generator=g, dtype=torch.int32)
    plane = (torch.arange(NB) % NP).to(torch.int32)
    base = torch.randn(NP, H, W, generator=g, dtype=torch.float64)
    d = lambda t: t.to(DEV).contiguous()
    return dict(pred=d(pred), mean=d(mean), std=d(std), aug=d(aug), plane=d(plane), base=d(base),
                pos=d(torch.tensor(pos, dtype=torch.int32)), reg=d(torch.tensor(reg, dtype=torch.int32)))


def _blend(c, idx, raster, log2_variants=2, **kw):
    """ops.blend_accumulate of the samples idx (a slice or an index tensor), oriented"""
    from resdepth_amd import ops
    f = lambda t: t[idx].contiguous()
    kw = {k: (f(v) if torch.is_tensor(v) else v) for k, v in kw.items()}
    return ops.blend_accumulate(f(c["pred"]), f(c["mean"]), f(c["std"]), f(c["pos"]), f(c["reg"]), T, 16, raster, aug=f(c["aug"]),
                                log2_variants=log2_variants, **kw)


@pytest.mark.parametrize("n", [24, 64, 72, 130])
def test_every_plane_is_the_tta_blend_of_its_own_samples(blend_case, n):
    c = blend_case
    got = _blend(c, slice(0, n), c["base"].clone(), plane=c["plane"], n_planes=NP)
    for p in range(NP):
        sel = torch.nonzero(c["plane"][:n] == p).flatten()
        want = _blend(c, sel, c["base"][p].clone())                    # rd_blend_accumulate_tta
        assert torch.equal(got[p], want), p
        assert not torch.equal(got[p], c["base"][p])


@pytest.mark.parametrize("n", [24, 130])
def test_no_plane_column_and_one_plane_is_the_tta_blend(blend_case, n):
    from resdepth_amd import _lib
    c = blend_case
    want = _blend(c, slice(0, n), c["base"][0].clone())
    got = c["base"][0].clone()
    rc = _lib.load().rd_blend_accumulate_planes(c["pred"].data_ptr(), c["mean"].data_ptr(), c["std"].data_ptr(), c["pos"].data_ptr(),
                                                c["reg"].data_ptr(), c["aug"].data_ptr(), None, n, T, 16, 2, got.data_ptr(), 1, H * W,
                                                H, W, _lib.stream_ptr())
    assert rc == 0
    assert torch.equal(got, want)
    zero = torch.zeros(NB, dtype=torch.int32, device=DEV)
    assert torch.equal(_blend(c, slice(0, n), c["base"][0].clone(), plane=zero), want)


def test_plane_bits_do_not_depend_on_the_call_split_or_the_run(blend_case):
    c = blend_case
    one = _blend(c, slice(0, NB), c["base"].clone(), plane=c["plane"], n_planes=NP)
    again = _blend(c, slice(0, NB), c["base"].clone(), plane=c["plane"], n_planes=NP)
    assert torch.equal(one, again)
    r = c["base"].clone()
    for k in range(0, NB, 50):                      # cuts at 50 and 100: inside the 64-sample launches of the whole call
        _blend(c, slice(k, min(k + 50, NB)), r, plane=c["plane"], n_planes=NP)
    assert torch.equal(r, one)


def test_a_plane_index_outside_the_planes_is_skipped(blend_case):
    c = blend_case
    plane = c["plane"].clone()
    bad = torch.arange(NB, device=DEV) % 7 == 3
    plane[bad] = torch.where(torch.arange(NB, device=DEV)[bad] % 2 == 0, -1, NP).to(torch.int32)
    buf = torch.full(((NP + 2) * H * W,), 7.25, dtype=torch.float64, device=DEV)             # a plane's room on either side
    raster = buf[H * W:(NP + 1) * H * W].view(NP, H, W)
    raster.copy_(c["base"])
    _blend(c, slice(0, NB), raster, plane=plane, n_planes=NP)
    keep = torch.nonzero(~bad).flatten()
    want = _blend(c, keep, c["base"].clone(), plane=c["plane"], n_planes=NP)
    assert torch.equal(raster, want)
    assert bool((buf[:H * W] == 7.25).all()) and bool((buf[(NP + 1) * H * W:] == 7.25).all())


# ---- 3. the fusion -----------------------------------------------------------------------------------------------------------
FN = 37 * 53


def _fuse_planes_np(p):
    """float64 normals [p, FN] with planted ties, a duplicated plane, +-0 and NaNs in single planes"""
    rng = np.random.default_rng(100 + p)
    v = rng.standard_normal((p, FN)) * 3.0 + 400.0
    if p > 1:
        v[1, 100:400] = v[0, 100:400]                       # ties between two planes
        v[:, 500:520] = v[0, 500:520]                       # all planes equal
        v[p - 1] = np.where(rng.random(FN) < 0.2, v[0], v[p - 1])
    if p > 2:
        v[2] = v[0]                                         # a duplicated plane
    v[:, 600:640] = 0.0
    v[::2, 600:640] = -0.0                                  # +-0 in alternating planes
    v[:, 640:650] = np.where(rng.random((p, 10)) < 0.5, 0.0, -0.0)
    for k in range(p):                                      # NaNs in single planes, at pixels of their own
        v[k, 700 + 13 * k:700 + 13 * k + 5] = np.nan
    v[0, FN - 1] = np.nan                                   # the last pixel of an odd n: the scalar tail
    v[p - 1, 0] = np.nan
    return v


def _fuse_c(v, stride, fuse, spread, offset=0):
    """rd_fuse_planes called directly: planes `stride` doubles apart, outputs `offset` doubles into their buffers"""
    from resdepth_amd import _lib, ops
    p, n = v.shape
    buf = torch.full((p * stride + 2,), 5.5, dtype=torch.float64, device=DEV)
    for k in range(p):
        buf[k * stride:k * stride + n] = torch.from_numpy(v[k]).to(DEV)
    outs = [torch.full((n + offset + 2,), 5.5, dtype=torch.float64, device=DEV) for _ in range(2)]
    want_s = spread is not None
    rc = _lib.load().rd_fuse_planes(buf.data_ptr(), stride, p, n, ops.FUSE_MODES[fuse], outs[0].data_ptr() + 8 * offset,
                                    ops.SPREAD_MODES[spread], outs[1].data_ptr() + 8 * offset if want_s else None, _lib.stream_ptr())
    assert rc == 0, _lib.load().rd_last_error_string()
    torch.cuda.synchronize()
    for o in outs[:1 + want_s]:
        assert bool((o[:offset] == 5.5).all()) and bool((o[offset + n:] == 5.5).all()), "written outside the output"
    return outs[0][offset:offset + n].cpu().numpy(), (outs[1][offset:offset + n].cpu().numpy() if want_s else None)


@pytest.mark.parametrize("extra", [0, 1, 7])
@pytest.mark.parametrize("p", [1, 2, 3, 4, 5, 8, 15, 16])
def test_fuse_is_the_host_loop(p, extra):
    v = _fuse_planes_np(p)
    for fuse in ("mean", "median"):
        for spread in (None, "range", "std"):
            got_f, got_s = _fuse_c(v, FN + extra, fuse, spread)
            _check_fuse(got_f, got_s, v, fuse, spread, (p, extra, fuse, spread))


@pytest.mark.parametrize("p", [1, 2, 3, 4, 5, 8, 15, 16])
def test_fuse_into_outputs_that_are_8_byte_aligned_only(p):
    v = _fuse_planes_np(p)
    for fuse, spread in (("median", "std"), ("mean", "range"), ("median", None)):
        got_f, got_s = _fuse_c(v, FN + 1, fuse, spread, offset=1)
        _check_fuse(got_f, got_s, v, fuse, spread, (p, fuse, spread))
        got_f, got_s = _fuse_c(v, FN + 7 - (FN + 7) % 2, fuse, spread, offset=1)       # even stride: only the outputs are off
        _check_fuse(got_f, got_s, v, fuse, spread, (p, fuse, spread))


def test_fuse_planes_wrapper():
    from resdepth_amd import ops
    v = _fuse_planes_np(5)
    planes = torch.from_numpy(v).to(DEV).view(5, 37, 53)
    f, s = ops.fuse_planes(planes, "median", "std")
    assert f.shape == s.shape == (37, 53)
    _check_fuse(f.cpu().numpy().ravel(), s.cpu().numpy().ravel(), v, "median", "std", "wrapper")
    f2, none = ops.fuse_planes(planes[1:4], "mean")                     # a view along the plane axis
    assert none is None
    _check_fuse(f2.cpu().numpy().ravel(), None, v[1:4], "mean", None, "view")
    wide = torch.zeros(5, 37, 60, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="contiguous"):
        ops.fuse_planes(wide[:, :, :53])
    with pytest.raises(ValueError, match="fuse"):
        ops.fuse_planes(planes, "mode")
    with pytest.raises(ValueError, match="spread"):
        ops.fuse_planes(planes, "mean", "iqr")
    with pytest.raises(TypeError):
        ops.fuse_planes(planes.float())


# ---- 4. end to end -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [3, 4])
@pytest.mark.parametrize("fuse,spread", [("median", "std"), ("mean", "range"), ("median", None), ("mean", "std")])
def test_fused_and_spread_are_the_fusion_of_the_planes(swept, p, fuse, spread):
    res = swept(p, 24, 32, fuse=fuse, spread=spread)
    assert res.fused.shape == (H, W) and (res.spread is None) == (spread is None)
    v = res.pairs.reshape(p, H * W)
    _check_fuse(res.fused.ravel(), None if res.spread is None else res.spread.ravel(), v, fuse, spread, (p, fuse, spread))
    assert np.isnan(res.fused).any() and not np.isnan(res.fused).all()
    if spread is not None:
        assert float(np.nanmax(res.spread)) > 0.0


@pytest.mark.parametrize("p", [3, 4])
def test_without_the_planes_the_fused_raster_is_the_same(swept, p):
    full = swept(p, 24, 32, fuse="median", spread="std")
    lean = swept(p, 24, 32, fuse="median", spread="std", return_pairs=False)
    assert lean.pairs is None and lean.image_pairs == PAIRS[p]
    assert np.array_equal(lean.fused, full.fused, equal_nan=True) and np.array_equal(lean.spread, full.spread, equal_nan=True)


def test_host_reuse_delivers_into_the_same_memory(rasters, model):
    from resdepth_amd import predict_pairs_linear_blend
    ld = _loader(rasters, PAIRS[3], 24, batch_size=32, sweep_pairs=True)
    a = predict_pairs_linear_blend(ld, model, host="reuse")
    keep = a.fused.copy()
    b = predict_pairs_linear_blend(ld, model, host="reuse")
    assert b.fused.ctypes.data == a.fused.ctypes.data and np.array_equal(b.fused, keep, equal_nan=True)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def test_loader_refusals(rasters):
    from resdepth_amd import GpuGridTiles
    with pytest.raises(ValueError, match="strategy='test'"):
        GpuGridTiles(_sampler(rasters, gt=True), "val", AREA, "geom-stereo", PAIRS[3], sweep_pairs=True)
    with pytest.raises(ValueError, match="image views"):
        GpuGridTiles(_sampler(rasters), "test", AREA, "geom", PAIRS[3], sweep_pairs=True)
    with pytest.raises(ValueError, match="up to 16"):
        GpuGridTiles(_sampler(rasters), "test", AREA, "geom-stereo", [[i % 4, (i + 1) % 4] for i in range(17)], sweep_pairs=True)
    with pytest.raises(ValueError, match="world > 1"):
        GpuGridTiles(_sampler(rasters), "test", AREA, "geom-stereo", PAIRS[3], sweep_pairs=True, shard=(0, 2))
    assert len(GpuGridTiles(_sampler(rasters), "test", AREA, "geom-stereo", [[i % 4, (i + 1) % 4] for i in range(16)],
                            sweep_pairs=True).dataset) == 35 * 16


def test_sweep_refusals(rasters, model, monkeypatch):
    from resdepth_amd import predict_linear_blend, predict_pairs_linear_blend
    with pytest.raises(ValueError, match="sweep_pairs=True"):
        predict_pairs_linear_blend(_loader(rasters, PAIRS[3], batch_size=16), model)
    with pytest.raises(ValueError, match="predict_pairs_linear_blend"):
        predict_linear_blend(_loader(rasters, PAIRS[3], batch_size=16, sweep_pairs=True), model)
    ld = _loader(rasters, PAIRS[3], batch_size=16, sweep_pairs=True)
    for kw in (dict(fuse="mode"), dict(spread="iqr")):
        with pytest.raises(ValueError):
            predict_pairs_linear_blend(ld, model, **kw)
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(RuntimeError, match="world > 1"):
        predict_pairs_linear_blend(ld, model)


def test_c_refusals_write_nothing(blend_case):
    from resdepth_amd import _lib, ops
    lib = _lib.load()
    n, p = 64, 4
    planes = torch.randn(p * (n + 2), dtype=torch.float64, device=DEV)
    fused, spread = torch.full((n,), 5.5, dtype=torch.float64, device=DEV), torch.full((n,), 5.5, dtype=torch.float64, device=DEV)
    s = _lib.stream_ptr()
    bad = [(planes.data_ptr(), n + 2, 0, n, 1, fused.data_ptr(), 2, spread.data_ptr()),          # P = 0
           (planes.data_ptr(), 4, 17, 4, 1, fused.data_ptr(), 2, spread.data_ptr()),             # P = 17
           (planes.data_ptr(), n - 1, p, n, 1, fused.data_ptr(), 2, spread.data_ptr()),          # plane_stride < n
           (planes.data_ptr(), n + 2, p, n, 1, fused.data_ptr(), 2, None),                       # a spread mode without its output
           (planes.data_ptr(), n + 2, p, n, 1, fused.data_ptr(), 1, None),
           (planes.data_ptr(), n + 2, p, n, 2, fused.data_ptr(), 0, None),                       # unknown modes
           (planes.data_ptr(), n + 2, p, n, 0, fused.data_ptr(), 3, spread.data_ptr()),
           (planes.data_ptr(), n + 2, p, 0, 0, fused.data_ptr(), 0, None),                       # no pixels
           (None, n + 2, p, n, 0, fused.data_ptr(), 0, None), (planes.data_ptr(), n + 2, p, n, 0, None, 0, None)]
    for args in bad:
        assert lib.rd_fuse_planes(*args, s) == 1 and lib.rd_last_error_string().startswith(b"rd_fuse_planes"), args   # RD_ERR_ARG
    torch.cuda.synchronize()
    assert bool((fused == 5.5).all()) and bool((spread == 5.5).all())
    assert lib.rd_fuse_planes(planes.data_ptr(), n + 2, p, n, 1, fused.data_ptr(), 0, None, s) == 0      # NULL spread with `none`
    c = blend_case
    raster = c["base"].clone()
    for kw, what in ((dict(log2_variants=5), "log2_variants"), (dict(log2_variants=-1), "log2_variants")):
        with pytest.raises(RuntimeError, match=what):
            _blend(c, slice(0, 24), raster, plane=c["plane"], n_planes=NP, **kw)
    ptrs = [c[k].data_ptr() for k in ("pred", "mean", "std", "pos", "reg", "aug", "plane")]
    for n_planes, stride in ((0, H * W), (-1, H * W), (NP, H * W - 1), (1, 0)):
        rc = lib.rd_blend_accumulate_planes(*ptrs, 24, T, 16, 0, raster.data_ptr(), n_planes, stride, H, W, s)
        assert rc == 1 and b"plane_stride" in lib.rd_last_error_string()
    torch.cuda.synchronize()
    assert torch.equal(raster, c["base"])
    with pytest.raises(TypeError):
        _blend(c, slice(0, 24), raster, plane=c["plane"].long(), n_planes=NP)
    with pytest.raises(ValueError):
        ops.blend_accumulate(c["pred"][:24], c["mean"][:24], c["std"][:24], c["pos"][:24], c["reg"][:24], T, 16, raster[0],
                             plane=c["plane"][:24].contiguous(), n_planes=NP)
    assert torch.equal(raster, c["base"])
