"""Test-time augmentation of the tiled sweep: oriented grid tiles (rd_assemble_grid_tiles_aug), the blend that undoes the
orientation (rd_blend_accumulate_tta) and predict_linear_blend over GpuGridTiles(tta=...).  Everything is compared bit for bit:
the yardsticks are the plain loader, rd_assemble_patches (pinned to the reference's transforms by the g9 / g20 fixtures) and
the existing ops.blend_accumulate.

Scene: 88 x 120 raster (no side a multiple of the stride), tile 32, strides 16 (35 tiles) and 24 (clamped last tiles whose
non-overlap box starts deeper than the overlap: the zero-weight branch of the ramp), 3 ortho planes, scattered nodata in the
input DSM and one 32 x 32 block of nodata on a grid position of both strides (a tile with a NaN mean)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, T = 88, 120, 32
AREA = {"x_extent": [(0, W - 1)], "y_extent": [(0, H - 1)]}
NODATA, DSM_STD, OSTD = -9999.0, 3.0, 50.0


@pytest.fixture(scope="module")
def rasters():
    rng = np.random.default_rng(17)
    dsm = (400.0 + 5.0 * rng.standard_normal((H, W))).astype(np.float32)
    dsm[rng.random((H, W)) < 0.03] = NODATA
    dsm[48:80, 48:80] = NODATA                      # tile (48, 48) of both strides: all nodata
    orthos = (110.0 + 40.0 * rng.standard_normal((3, H, W))).astype(np.float32)
    return dsm, orthos


def _sampler(rasters, ortho_mean=110.0):
    from resdepth_amd import GpuPatchSampler
    dsm, orthos = rasters
    return GpuPatchSampler(dsm, None, orthos, tile_size=T, nodata=NODATA, dsm_std=DSM_STD, ortho_mean=ortho_mean, ortho_std=OSTD)


def _loader(rasters, channels="geom-stereo", stride=16, ortho_mean=110.0, **kw):
    from resdepth_amd import GpuGridTiles
    pairs = None if channels == "geom" else [[0, 1]]
    return GpuGridTiles(_sampler(rasters, ortho_mean), "test", AREA, channels, pairs, stride=stride, **kw)


def _collect(loader):
    out = {}
    for b in loader:
        for k, v in b.items():
            out.setdefault(k, []).append(v.cpu())
    return {k: torch.cat(v).numpy() for k, v in out.items()}


def _np_apply(x, code):
    from resdepth_amd import tiling
    return tiling.tta_apply(x, code)


def _t_apply(x, code):
    y = torch.rot90(x, code & 3, (-2, -1))
    if code & 4:
        y = torch.flip(y, (-2,))
    if code & 8:
        y = torch.flip(y, (-1,))
    return y.contiguous()


def _t_undo(y, code):
    if code & 8:
        y = torch.flip(y, (-1,))
    if code & 4:
        y = torch.flip(y, (-2,))
    return torch.rot90(y, -(code & 3), (-2, -1)).contiguous()


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


# ---- 1. assembly -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels,stride,tta,swap,ortho_mean", [
    ("geom-stereo", 16, "d4", False, 110.0), ("geom-stereo", 24, "flips", False, 110.0), ("geom-stereo", 16, "none", False, 110.0),
    ("geom-stereo", 16, "d4", True, 110.0), ("geom-stereo", 24, [3, 6, 13, 15], True, 110.0), ("geom-stereo", 16, None, True, 110.0),
    ("geom", 16, "d4", False, 110.0), ("stereo", 24, "d4", False, None), ("geom-stereo", 16, list(range(16)), False, None),
    ("geom-stereo", 24, "flips", True, None)])      # swapped views with a per-tile ortho mean: summed in the other view order
def test_oriented_tiles_are_the_plain_tiles_permuted(rasters, channels, stride, tta, swap, ortho_mean):
    from resdepth_amd import tiling
    plain = _collect(_loader(rasters, channels, stride, ortho_mean, batch_size=16))
    ld = _loader(rasters, channels, stride, ortho_mean, batch_size=24, tta=tta, tta_swap_views=swap)
    got = _collect(ld)
    codes = tiling.tta_codes(tta) * (2 if swap else 1)
    G, n = len(codes), plain["input"].shape[0]
    ds = ld.dataset
    assert ds.tta == codes and len(ds) == G * n == got["input"].shape[0] and len(ld) == -(-G * n // 24)
    assert "target" not in got and "loss_mask" not in got
    assert got["tta"].dtype == np.int32 and got["tta"].tolist() == list(codes) * n == list(ds.tta_code)
    assert ds.tta_swap == ([0] * (G // 2) + [1] * (G // 2) if swap else [0] * G) * n
    assert np.isnan(plain["dsm_mean"]).sum() == 1                      # the all-nodata tile
    dsm_ch = 0 if channels == "stereo" else 1
    for i in range(n):
        for g, code in enumerate(codes):
            s = i * G + g
            want = plain["input"][i]
            if swap and g >= G // 2:
                want = np.concatenate([want[:dsm_ch], want[dsm_ch:][::-1]])
            assert np.array_equal(got["input"][s], _np_apply(want, code), equal_nan=True), (i, code)
            assert np.array_equal(got["dsm_mean"][s], plain["dsm_mean"][i], equal_nan=True)
            assert tuple(ds.pos[s]) == (got["patch_offset_y"][s], got["patch_offset_x"][s]) == \
                (plain["patch_offset_y"][i], plain["patch_offset_x"][i])
            assert tuple(ds.reg[s]) == (plain["patch_valid_pixels_uly"][i], plain["patch_valid_pixels_ulx"][i],
                                        plain["patch_valid_pixels_lry"][i], plain["patch_valid_pixels_lrx"][i])
    for k in ("dsm_std", "nodata", "patch_valid_pixels_uly", "patch_valid_pixels_lrx"):
        assert np.array_equal(got[k], np.repeat(plain[k], G))


def test_orientation_is_rd_assemble_patches_orientation(rasters):
    """one code per 90-degree class (with different flips): the oriented input is what the training assembler writes for the
    same position, code and means"""
    from resdepth_amd import _lib
    codes = (0 | 8, 1 | 4, 2, 3 | 12)
    ld = _loader(rasters, "geom-stereo", 16, 110.0, batch_size=24, tta=codes)
    src, n = ld.source, len(ld.dataset)
    got = torch.cat([b["input"] for b in ld])
    mean = torch.cat([b["dsm_mean"] for b in ld]).contiguous()
    pos = torch.tensor(ld.dataset.pos, dtype=torch.int32, device=DEV)
    aug = torch.tensor(ld.dataset.tta_code, dtype=torch.int32, device=DEV)
    pair = torch.tensor([[0, 1]] * n, dtype=torch.int32, device=DEV)
    omean = torch.full((n,), 110.0, device=DEV)
    want = torch.empty_like(got)
    _lib.check(_lib.load().rd_assemble_patches(src.dsm_in.data_ptr(), None, src.orthos.data_ptr(), H * W, pair.data_ptr(), 2,
                                               pos.data_ptr(), aug.data_ptr(), mean.data_ptr(), DSM_STD, omean.data_ptr(), OSTD,
                                               NODATA, n, T, W, want.data_ptr(), None, None, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want.cpu().numpy(), equal_nan=True)


def test_without_tta_the_loader_is_todays(rasters):
    from resdepth_amd import _lib
    ld = _loader(rasters, batch_size=16)
    assert ld.dataset.tta is None and not ld.tta
    b = next(iter(ld))
    assert "tta" not in b and b["input"].shape == (16, 3, T, T)
    # the plain entry point, called directly with the loader's table, gives the same bits
    inp, mean = torch.empty_like(b["input"]), torch.empty_like(b["dsm_mean"])
    ws = torch.empty(_lib.load().rd_assemble_grid_tiles_ws_bytes(16, T), dtype=torch.uint8, device=DEV)
    src = ld.source
    _lib.check(_lib.load().rd_assemble_grid_tiles(
        src.dsm_in.data_ptr(), None, src.orthos.data_ptr(), 3, H, W, ld._table.data_ptr(), ld._pair_planes.data_ptr(), 1, 2, 1, 16,
        T, NODATA, 2, 0.0, DSM_STD, 1, 110.0, OSTD, inp.data_ptr(), None, None, mean.data_ptr(), ws.data_ptr(), ws.numel(),
        _lib.stream_ptr()))
    assert torch.equal(inp.view(torch.int32), b["input"].view(torch.int32))


# ---- 2. the blend kernel -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blend_case():
    """72 samples: the 35 stride-16 tiles twice + 2 (the reference's order per pixel matters: overlapping tiles, repeated
    positions), random predictions / means / codes"""
    from resdepth_amd import tiling
    _, pos, reg, _ = tiling.grid_samples(AREA["x_extent"], AREA["y_extent"], T, "test", 16)
    pos, reg = (pos * 3)[:72], (reg * 3)[:72]
    g = torch.Generator().manual_seed(9)
    pred = torch.randn(72, 1, T, T, generator=g)
    mean = 400.0 + torch.randn(72, generator=g)
    std = torch.full((72,), DSM_STD)
    aug = torch.randint(0, 16, (72,), generator=g, dtype=torch.int32)
    aug[:16] = torch.arange(16, dtype=torch.int32)
    base = torch.randn(H, W, generator=g, dtype=torch.float64)
    unoriented = torch.stack([_t_undo(pred[i], int(aug[i])) for i in range(72)])
    d = lambda t: t.to(DEV).contiguous()
    return dict(pred=d(pred), mean=d(mean), std=d(std), aug=d(aug), base=d(base), unoriented=d(unoriented),
                pos=d(torch.tensor(pos, dtype=torch.int32)), reg=d(torch.tensor(reg, dtype=torch.int32)))


def _blend(c, pred, sl=slice(None), raster=None, **kw):
    from resdepth_amd import ops
    raster = c["base"].clone() if raster is None else raster
    kw = {k: (v[sl] if torch.is_tensor(v) else v) for k, v in kw.items()}
    return ops.blend_accumulate(pred[sl], c["mean"][sl], c["std"][sl], c["pos"][sl], c["reg"][sl], T, 16, raster, **kw)


@pytest.mark.parametrize("n", [24, 64, 72])
def test_blend_without_orientation_is_the_existing_blend(blend_case, n):
    c = blend_case
    want = _blend(c, c["pred"], slice(0, n))
    zero = torch.zeros(72, dtype=torch.int32, device=DEV)
    assert torch.equal(_blend(c, c["pred"], slice(0, n), aug=zero), want)
    # NULL aug with a weight: 2^-0 is covered above; log2_variants > 0 without aug scales only
    half = _blend(c, c["pred"], slice(0, n), raster=torch.zeros_like(c["base"]), log2_variants=1)
    full = _blend(c, c["pred"], slice(0, n), raster=torch.zeros_like(c["base"]))
    assert torch.equal(half, full * 0.5)


@pytest.mark.parametrize("log2_variants", [0, 1, 2, 3, 4])
def test_blend_is_the_scaled_existing_blend_of_unoriented_predictions(blend_case, log2_variants):
    c = blend_case
    zero = torch.zeros_like(c["base"])
    for n in (24, 72):
        want = _blend(c, c["unoriented"], slice(0, n), raster=zero.clone()) * 2.0 ** -log2_variants
        got = _blend(c, c["pred"], slice(0, n), raster=zero.clone(), aug=c["aug"], log2_variants=log2_variants)
        assert torch.equal(got, want)
    # on a raster that already holds something: only what the call adds is scaled
    got = _blend(c, c["pred"], aug=c["aug"], log2_variants=log2_variants)
    want = _blend(c, c["unoriented"], raster=c["base"] * 2.0 ** log2_variants) * 2.0 ** -log2_variants
    assert torch.equal(got, want) and not torch.equal(got, c["base"])


def test_blend_bits_do_not_depend_on_the_call_split_or_the_run(blend_case):
    c = blend_case
    one = _blend(c, c["pred"], aug=c["aug"], log2_variants=3)
    again = _blend(c, c["pred"], aug=c["aug"], log2_variants=3)
    assert torch.equal(one, again)
    r = c["base"].clone()
    for k in range(0, 72, 24):
        _blend(c, c["pred"], slice(k, k + 24), raster=r, aug=c["aug"], log2_variants=3)
    assert torch.equal(r, one)


# ---- 3. the whole sweep ----------------------------------------------------------------------------------------------------
def _composed_sweep(rasters, model, stride, codes):
    """plain tile -> torch transform -> model (one image per forward) -> torch inverse -> the existing blend, then x 1 / G"""
    from resdepth_amd import ops
    raster = torch.zeros(H, W, dtype=torch.float64, device=DEV)
    i32 = lambda *cols: torch.stack(cols, 1).to(torch.int32).contiguous()
    with torch.no_grad():
        for b in _loader(rasters, stride=stride, batch_size=16):
            pos = i32(b["patch_offset_y"], b["patch_offset_x"])
            reg = i32(b["patch_valid_pixels_uly"], b["patch_valid_pixels_ulx"], b["patch_valid_pixels_lry"], b["patch_valid_pixels_lrx"])
            for i in range(b["input"].shape[0]):
                for code in codes:
                    y = _t_undo(model(_t_apply(b["input"][i:i + 1], code)), code)
                    ops.blend_accumulate(y, b["dsm_mean"][i:i + 1].contiguous(), b["dsm_std"][i:i + 1].contiguous(),
                                         pos[i:i + 1].contiguous(), reg[i:i + 1].contiguous(), T, stride, raster)
    return (raster * (1.0 / len(codes))).cpu().numpy()


@pytest.mark.parametrize("stride", [16, 24])
def test_d4_sweep_is_the_composition_of_its_parts(rasters, model, stride):
    from resdepth_amd import predict_linear_blend, tiling
    got = predict_linear_blend(_loader(rasters, stride=stride, batch_size=24, tta="d4"), model)
    want = _composed_sweep(rasters, model, stride, tiling.tta_codes("d4"))
    assert got.shape == (H, W) and np.isnan(want).any() and not np.isnan(want).all()
    assert np.array_equal(got, want, equal_nan=True)


def test_none_is_the_plain_sweep_and_flips_is_not(rasters, model):
    from resdepth_amd import predict_linear_blend
    plain = predict_linear_blend(_loader(rasters, batch_size=24), model)
    none = predict_linear_blend(_loader(rasters, batch_size=24, tta="none"), model)
    flips = predict_linear_blend(_loader(rasters, batch_size=24, tta="flips"), model)
    assert np.array_equal(plain, none, equal_nan=True)
    ok = ~np.isnan(plain)
    assert np.array_equal(np.isnan(flips), ~ok)
    assert not np.array_equal(plain[ok], flips[ok])


def test_a_host_loader_with_the_tta_column_sweeps_the_same(rasters, model):
    from torch.utils.data import DataLoader, Dataset
    from resdepth_amd import predict_linear_blend
    ld = _loader(rasters, batch_size=24, tta="flips")
    want = predict_linear_blend(ld, model)
    rows = {k: torch.cat([b[k].cpu() for b in ld]) for k in next(iter(ld))}

    class Host(Dataset):
        tile_size, stride, raster_shape, pos, tta = T, 16, (H, W), ld.dataset.pos, ld.dataset.tta

        def __len__(self):
            return len(self.pos)

        def __getitem__(self, i):
            return {k: v[i] for k, v in rows.items()}
    got = predict_linear_blend(DataLoader(Host(), batch_size=10, shuffle=False), model)
    assert np.array_equal(got, want, equal_nan=True)
    Host.tta = (0, 4, 8)
    with pytest.raises(ValueError, match="dataset.tta"):
        predict_linear_blend(DataLoader(Host(), batch_size=10, shuffle=False), model)


# ---- 4. sharding ---------------------------------------------------------------------------------------------------------
def test_banded_route_at_world_one_returns_the_same_raster(rasters, model, tmp_path):
    import torch.distributed as dist
    from resdepth_amd import predict_linear_blend
    want = predict_linear_blend(_loader(rasters, batch_size=24, tta="flips"), model)
    os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
    dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        ld = _loader(rasters, batch_size=24, tta="flips", shard=(0, 1))
        assert ld.dataset.shard_plan and ld.dataset.shard_plan[0]["monotonic"]
        got = np.array(predict_linear_blend(ld, model))
    finally:
        dist.destroy_process_group()
    assert np.array_equal(got, want, equal_nan=True)


# ---- 5. errors -----------------------------------------------------------------------------------------------------------
def test_refusals(rasters, blend_case):
    from resdepth_amd import GpuGridTiles, GpuPatchSampler, _lib, ops
    dsm, orthos = rasters
    val = GpuPatchSampler(dsm, dsm.copy(), orthos, tile_size=T, nodata=NODATA, dsm_std=DSM_STD, ortho_mean=110.0, ortho_std=OSTD)
    with pytest.raises(ValueError, match="strategy='test'"):
        GpuGridTiles(val, "val", AREA, "geom-stereo", [[0, 1]], tta="d4")
    with pytest.raises(ValueError, match="strategy='test'"):
        GpuGridTiles(val, "val", AREA, "geom-stereo", [[0, 1]], tta_swap_views=True)
    for tta, swap in (([0, 1, 2], False), (list(range(16)), True), ([0, 1, 2, 3, 4, 5], True)):
        with pytest.raises(ValueError, match="1, 2, 4, 8 or 16"):
            _loader(rasters, tta=tta, tta_swap_views=swap)
    with pytest.raises(ValueError, match="two or more views"):
        GpuGridTiles(_sampler(rasters), "test", AREA, "geom-mono", [[0]], tta="flips", tta_swap_views=True)
    with pytest.raises(ValueError, match="two or more views"):
        _loader(rasters, "geom", tta_swap_views=True)
    # the C entry point: target / mask are refused with an error string, nothing is launched
    ld = _loader(rasters, batch_size=4, tta="flips")
    src, lib = ld.source, _lib.load()
    inp = torch.empty(4, 3, T, T, device=DEV)
    tgt, msk = torch.full((4, 1, T, T), 7.0, device=DEV), torch.full((4, 1, T, T), 7, dtype=torch.uint8, device=DEV)
    mean = torch.empty(4, device=DEV)
    ws = torch.empty(lib.rd_assemble_grid_tiles_ws_bytes(4, T), dtype=torch.uint8, device=DEV)
    for t_, m_ in ((tgt, msk), (tgt, None), (None, msk)):
        rc = lib.rd_assemble_grid_tiles_aug(
            src.dsm_in.data_ptr(), None, src.orthos.data_ptr(), 3, H, W, ld._table.data_ptr(), ld._pair_planes.data_ptr(), 1, 2, 1,
            4, T, NODATA, 2, 0.0, DSM_STD, 1, 110.0, OSTD, ld._aug.data_ptr(), inp.data_ptr(),
            None if t_ is None else t_.data_ptr(), None if m_ is None else m_.data_ptr(), mean.data_ptr(), ws.data_ptr(),
            ws.numel(), _lib.stream_ptr())
        assert rc == 1 and b"target / mask" in lib.rd_last_error_string()        # RD_ERR_ARG
    torch.cuda.synchronize()
    assert bool((tgt == 7.0).all()) and bool((msk == 7).all())
    c = blend_case
    before = c["base"].clone()
    for bad in (5, -1):
        with pytest.raises(RuntimeError, match="log2_variants"):
            ops.blend_accumulate(c["pred"], c["mean"], c["std"], c["pos"], c["reg"], T, 16, before, aug=c["aug"], log2_variants=bad)
    assert torch.equal(before, c["base"])
    with pytest.raises(TypeError):
        ops.blend_accumulate(c["pred"], c["mean"], c["std"], c["pos"], c["reg"], T, 16, before, aug=c["aug"].long())
