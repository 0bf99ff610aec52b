"""Validation / inference grid tiles assembled on the GPU (GpuGridTiles, rd_assemble_grid_tiles; -m gpu): every sample of the
reference's own 'val' / 'test' datasets (g19 fixture), tiled inference and validation fed from HBM-resident rasters against
the same pipelines fed by a host DataLoader over the numpy stand-in (tests/grid_tiles_ref.py)."""
import json
import os
import types

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import grid_tiles_ref as R
from conftest import load_npz

pytestmark = pytest.mark.gpu


def _sampler(dsm, gt, orthos_hwv, tile, nodata, dsm_std, ortho_mean, ortho_std):
    from resdepth_amd import GpuPatchSampler
    orth = np.ascontiguousarray(orthos_hwv.transpose(2, 0, 1))
    return GpuPatchSampler(dsm, gt, orth, tile_size=tile, nodata=float(nodata), dsm_std=float(dsm_std), ortho_mean=ortho_mean,
                           ortho_std=float(ortho_std))


def _collect(loader):
    out = {}
    for b in loader:
        for k, v in b.items():
            out.setdefault(k, []).append(v.cpu())
    return {k: torch.cat(v).numpy() for k, v in out.items()}


def test_every_reference_sample_in_every_mode():
    from resdepth_amd import GpuGridTiles
    g = load_npz("g19_grid.npz")
    orthos = g["orthos_u8"].astype(np.float32)
    t = int(g["tile"])
    for name in g["cases"]:
        name = str(name)
        c = json.loads(str(g[f"{name}/settings"]))
        smp = _sampler(g["dsm_in"], g["dsm_gt"] if c["gt"] else None, orthos, t, g["nodata"], g["dsm_std"], c["ortho_mean"],
                       g["ortho_std"])
        loader = GpuGridTiles(smp, c["strategy"], c["area"], c["channels"], c["pairs"], dsm_mean=c["dsm_mean"],
                              transform_dsm=c.get("transform_dsm", True), transform_orthos=c.get("transform_orthos", True),
                              batch_size=5)
        n = len(g[f"{name}/pos"])
        assert len(loader.dataset) == n and len(loader) == -(-n // 5), name
        assert loader.dataset.stride == int(g[f"{name}/stride"]) and loader.dataset.raster_shape == g["dsm_in"].shape
        np.testing.assert_array_equal(np.array(loader.dataset.pos), g[f"{name}/pos"])
        b = _collect(loader)
        assert b["input"].shape == g[f"{name}/input"].shape, name
        np.testing.assert_allclose(b["input"], g[f"{name}/input"], rtol=0, atol=3e-5, err_msg=name)
        want_mean = g[f"{name}/dsm_mean"]
        assert np.all(np.abs(b["dsm_mean"] - want_mean) <= 1e-6 * np.abs(want_mean)), name
        if c["gt"]:
            np.testing.assert_allclose(b["target"], g[f"{name}/target"], rtol=0, atol=3e-5, err_msg=name)
            assert b["loss_mask"].dtype == np.bool_
            np.testing.assert_array_equal(b["loss_mask"], g[f"{name}/loss_mask"], err_msg=name)
        else:
            assert "target" not in b and "loss_mask" not in b
        for j, k in enumerate(R.META):
            np.testing.assert_array_equal(b[k], g[f"{name}/meta"][:, j], err_msg=f"{name} {k}")
        np.testing.assert_array_equal(b["nodata"], g[f"{name}/scalars"][:, 0].astype(np.float32))
        np.testing.assert_array_equal(b["dsm_std"], g[f"{name}/scalars"][:, 1].astype(np.float32))
        # a given mean involves no reduction: bit-exact
        views = slice(0 if c["channels"] == "stereo" else 1, None)
        if c["ortho_mean"] or not c.get("transform_orthos", True):
            assert np.array_equal(b["input"][:, views], g[f"{name}/input"][:, views]), name
        if c["dsm_mean"] or not c.get("transform_dsm", True):
            assert np.array_equal(b["input"][:, 0], g[f"{name}/input"][:, 0]), name
            assert np.array_equal(b["target"], g[f"{name}/target"]), name


def test_out_of_scope_options_are_refused():
    from resdepth_amd import GpuGridTiles
    g = load_npz("g19_grid.npz")
    smp = _sampler(g["dsm_in"], g["dsm_gt"], g["orthos_u8"].astype(np.float32), 16, g["nodata"], 3.0, None, 40.0)
    area = {"x_extent": [(0, 63)], "y_extent": [(0, 47)]}
    for kw in (dict(augment=True), dict(permute_images_within_pair=True), dict(strategy="val", shard=(0, 2)),
               dict(strategy="train"), dict(area_defn={"x_extent": [(0, 200)], "y_extent": [(0, 47)]})):
        args = dict(strategy="test", area_defn=area, input_channels="geom-stereo", image_pairs=[[0, 1]])
        args.update(kw)
        with pytest.raises(ValueError):
            GpuGridTiles(smp, **args)
    with pytest.raises(ValueError):
        GpuGridTiles([smp, smp], "test", area, "geom")


# ---- a 1024^2 raster: three planes, nodata holes, two areas ---------------------------------------------------------------
ROWS, COLS, T = 1024, 1040, 64
AREAS = {"x_extent": [(0, 1039), (100, 803)], "y_extent": [(0, 611), (600, 1023)]}


@pytest.fixture(scope="module")
def scene():
    rng = np.random.RandomState(7)
    dsm = (rng.randn(ROWS, COLS) * 4 + 420).astype(np.float32)
    gt = (dsm + rng.randn(ROWS, COLS) * 1.5).astype(np.float32)
    dsm[100:140, 200:260] = -9999.0
    dsm[700:705, 20:900] = -9999.0
    gt[300:330, 400:470] = -9999.0
    gt[::97, ::89] = 0.0
    orthos = (rng.rand(ROWS, COLS, 2) * 200 + 20).astype(np.float32)
    return dsm, gt, orthos


def _model(seed=0):
    from resdepth_amd import UNet
    torch.manual_seed(seed)
    return UNet(n_input_channels=3, start_kernel=8, depth=3, bias_conv_layer=True).to("cuda:0").eval()


def test_inference_sweep_matches_the_host_dataloader_and_is_batch_invariant(scene):
    from resdepth_amd import GpuGridTiles, predict_linear_blend
    dsm, gt, orthos = scene
    smp = _sampler(dsm, None, orthos, T, -9999.0, 3.0, None, 50.0)
    model = _model()
    mk = lambda **kw: GpuGridTiles(smp, "test", AREAS, "geom-stereo", [[1, 0]], **kw)      # noqa: E731
    gpu = mk(batch_size=32)
    ds = gpu.dataset
    host = R.StandInGridDataset(dsm, None, orthos, ds.pos, ds.reg, [[1, 0]] * len(ds), T, ds.stride, -9999.0, 3.0, None, 50.0,
                                "geom-stereo")
    out = predict_linear_blend(gpu, model)
    ref = predict_linear_blend(DataLoader(host, batch_size=32, shuffle=False), model)
    assert np.abs(out).max() > 100                                   # the areas were swept
    # inputs that differ in the last bits of the per-tile means: the bar of test_blend_gpu.py, away from the tiles that hold
    # input nodata (there the network sees (-9999 - mean) / std = -3.5e3, and its relative noise becomes millimetres)
    holes = np.zeros(out.shape, dtype=bool)
    for y, x in ds.pos:
        if (dsm[y:y + T, x:x + T] == -9999.0).any():
            holes[y:y + T, x:x + T] = True
    assert 0.05 < holes.mean() < 0.5
    assert np.abs(out - ref)[~holes].max() <= 1e-4, np.abs(out - ref)[~holes].max()
    # a given ortho mean, and the stand-in given the GPU loader's DSM means: bit-identical inputs, the same raster everywhere
    fixed = GpuGridTiles(_sampler(dsm, None, orthos, T, -9999.0, 3.0, 120.0, 50.0), "test", AREAS, "geom-stereo", [[1, 0]])
    host2 = R.StandInGridDataset(dsm, None, orthos, ds.pos, ds.reg, [[1, 0]] * len(ds), T, ds.stride, -9999.0, 3.0, 120.0,
                                 50.0, "geom-stereo", mean_override=_collect(fixed)["dsm_mean"])
    a = predict_linear_blend(fixed, model)
    b = predict_linear_blend(DataLoader(host2, batch_size=32, shuffle=False), model)
    assert np.abs(a - b).max() <= 1e-9, np.abs(a - b).max()
    for kw in (dict(batch_size=5), dict(batch_size=32, prefetch=0), dict(batch_size=7, prefetch=3)):
        again = predict_linear_blend(mk(**kw), model)
        assert np.abs(out - again).max() <= 1e-9, (kw, np.abs(out - again).max())
    parts = [mk(batch_size=32, shard=(r, 3)) for r in range(3)]
    assert sum(len(p.dataset) for p in parts) == len(ds) and all(p.dataset.shard_plan == parts[0].dataset.shard_plan for p in parts)
    total = sum(predict_linear_blend(p, model, reduce_to_rank0=False).copy() for p in parts)
    assert np.abs(out - total).max() <= 1e-9, np.abs(out - total).max()


def _trainer_args(tmp, model, opt, train, val, n_epochs):
    return types.SimpleNamespace(
        model=model, optimizer=opt, scheduler=None, criterion=torch.nn.L1Loss(reduction="mean"), trainloader=train,
        valloader=val, n_epochs=n_epochs, evaluate_rate=1, save_model_rate=10 ** 9, freq_average_train_loss=20,
        save_dir=str(tmp), log_file=None, checkpoint_dir=os.path.join(str(tmp), "checkpoints"),
        tboard_log_dir=os.path.join(str(tmp), "tb"), pretrained_path=None)


def test_validation_metric_matches_host_batches_and_training_runs(scene, tmp_path):
    from resdepth_amd import FusedAdam, GpuGridTiles, SamplerLoader, Trainer
    dsm, gt, orthos = scene
    smp = _sampler(dsm, gt, orthos, T, -9999.0, 3.0, 110.0, 50.0)
    val_area = {"x_extent": [(0, 1039), (0, 1039)], "y_extent": [(0, 255), (768, 1023)]}
    val = GpuGridTiles(smp, "val", val_area, "geom-stereo", [[0, 1], [1, 0]], batch_size=12)
    ds = val.dataset
    assert len(ds) == 2 * (4 + 4) * 17 and ds.pair_idx[len(ds) // 2] == 1
    train = SamplerLoader(smp, n_batches=3, batch_size=8, pairs=[0, 1], generator=torch.Generator().manual_seed(1))
    model = _model(1).train()
    opt = FusedAdam(model.parameters(), lr=1e-3)
    tr = Trainer(_trainer_args(tmp_path / "a", model, opt, train, val, 2))
    tr.logger.handlers.clear()
    pairs = [[[0, 1], [1, 0]][i] for i in ds.pair_idx]
    host = lambda mo=None: DataLoader(R.StandInGridDataset(dsm, gt, orthos, ds.pos, ds.reg, pairs, T, ds.stride, -9999.0, 3.0,  # noqa: E731
                                                           110.0, 50.0, "geom-stereo", mean_override=mo),
                                      batch_size=12, shuffle=False)
    m_gpu = tr.inference_one_epoch(0, "val")["MAE_metric"].avg
    gpu_means = _collect(val)["dsm_mean"]
    tr.loader["val"] = host()
    m_host = tr.inference_one_epoch(0, "val")["MAE_metric"].avg
    assert abs(m_gpu - m_host) <= 1e-4 * abs(m_host), (m_gpu, m_host)
    tr.loader["val"] = host(gpu_means)                   # the GPU loader's means: bit-identical inputs, the same metric
    assert tr.inference_one_epoch(0, "val")["MAE_metric"].avg == m_gpu
    # the full loop: SamplerLoader for training, GpuGridTiles for validation, one resident raster set
    tr.loader["val"] = val
    tr.train()
    assert os.path.isfile(os.path.join(str(tmp_path / "a"), "checkpoints", "Model_best.pth"))
    assert np.isfinite(tr.best_loss)
