"""The training set and its normalisation statistics on the GPU (GpuTrainSet, rd_assemble_train_patches, rd_patch_moments,
rd_region_moments; -m gpu): the reference's own 'train' sample lists, samples and statistics (g20 fixture), mixed-raster
batches against GpuPatchSampler.sample, epochs that do not depend on batch size or prefetch depth, the Trainer loop, and the
statistics against the float128 values of the reference and the fp64 stand-in (tests/train_set_ref.py)."""
import json
import os
import types

import numpy as np
import pytest
import torch

import train_set_ref as R
from conftest import load_npz

pytestmark = pytest.mark.gpu

REL = 1e-12          # the statistics' bar: two orders above the rounding bound of an fp64 centred sum over 256 terms
KEYS = {"input", "target", "loss_mask", "dsm_mean", "dsm_std", "patch_offset_x", "patch_offset_y", "nodata",
        "patch_valid_pixels_uly", "patch_valid_pixels_ulx", "patch_valid_pixels_lry", "patch_valid_pixels_lrx"}


@pytest.fixture(scope="module")
def g():
    return load_npz("g20_train.npz")


def _sampler(g, raster, ortho_mean, gt=True, tile=None):
    from resdepth_amd import GpuPatchSampler
    orth = np.ascontiguousarray(g[f"{raster}/orthos_u8"].astype(np.float32).transpose(2, 0, 1))
    return GpuPatchSampler(g[f"{raster}/dsm_in"], g[f"{raster}/dsm_gt"] if gt else None, orth, tile_size=tile or int(g["tile"]),
                           nodata=float(g["nodata"]), dsm_std=float(g[f"{raster}/dsm_std"]), ortho_mean=ortho_mean,
                           ortho_std=float(g[f"{raster}/ortho_std"]))


def _collect(loader):
    out = {}
    for b in loader:
        for k, v in b.items():
            out.setdefault(k, []).append(v.cpu())
    return {k: torch.cat(v).numpy() for k, v in out.items()}


def _fixture_set(g, name, c, **kw):
    from resdepth_amd import GpuTrainSet
    np.random.seed(c["seed"])
    datasets = [dict(sampler=_sampler(g, d["raster"], c["ortho_mean"]), area_defn=d["area"], n_samples=d["n_samples"],
                     image_pairs=d["pairs"]) for d in c["datasets"]]
    args = dict(use_all_stereo_pairs=c["use_all"], augment=False, shuffle=False, dsm_mean=c["dsm_mean"],
                transform_dsm=c.get("transform_dsm", True), transform_orthos=c.get("transform_orthos", True), batch_size=5)
    args.update(kw)
    return GpuTrainSet(datasets, c["channels"], **args)


def test_every_reference_sample_list_and_sample(g):
    for name in g["cases"]:
        name = str(name)
        c = json.loads(str(g[f"{name}/settings"]))
        loader = _fixture_set(g, name, c)
        ids, pos, pidx = loader.sample_list()
        np.testing.assert_array_equal(ids, g[f"{name}/dataset_id"], err_msg=name)            # the sample list: exact
        np.testing.assert_array_equal(pos, g[f"{name}/pos"], err_msg=name)
        np.testing.assert_array_equal(pidx, g[f"{name}/pair_idx"], err_msg=name)
        n = len(pos)
        assert len(loader.dataset) == n and len(loader) == -(-n // 5) and loader.batch_size == 5 and not loader.drop_last
        b = _collect(loader)
        assert set(b) == KEYS, name
        assert b["input"].shape == g[f"{name}/input"].shape and b["input"].dtype == np.float32, name
        err = np.abs(b["input"] - g[f"{name}/input"]).max(), np.abs(b["target"] - g[f"{name}/target"]).max()
        print(name, "max |input| / |target| error", err)
        np.testing.assert_allclose(b["input"], g[f"{name}/input"], rtol=0, atol=3e-5, err_msg=name)
        np.testing.assert_allclose(b["target"], g[f"{name}/target"], rtol=0, atol=3e-5, err_msg=name)
        assert b["loss_mask"].dtype == np.bool_
        np.testing.assert_array_equal(b["loss_mask"], g[f"{name}/loss_mask"], err_msg=name)
        want_mean = g[f"{name}/dsm_mean"]
        assert b["dsm_mean"].dtype == np.float32 and np.all(np.abs(b["dsm_mean"] - want_mean) <= 1e-6 * np.abs(want_mean)), name
        np.testing.assert_array_equal(b["patch_offset_y"], g[f"{name}/offsets"][:, 0])
        np.testing.assert_array_equal(b["patch_offset_x"], g[f"{name}/offsets"][:, 1])
        assert b["patch_offset_x"].dtype == np.int64
        np.testing.assert_array_equal(b["nodata"], g[f"{name}/scalars"][:, 0].astype(np.float32))
        np.testing.assert_array_equal(b["dsm_std"], g[f"{name}/scalars"][:, 1].astype(np.float32))      # per sample: the rasters' own
        for k in ("uly", "ulx", "lry", "lrx"):
            v = b[f"patch_valid_pixels_{k}"]
            assert v.dtype == np.float64 and v.shape == (n,) and np.isnan(v).all()
        # a given mean involves no reduction: bit-exact
        views = slice(0 if c["channels"] == "stereo" else 1, None)
        if c["ortho_mean"] or not c.get("transform_orthos", True):
            assert np.array_equal(b["input"][:, views], g[f"{name}/input"][:, views]), name
        if c["dsm_mean"] or not c.get("transform_dsm", True):
            assert np.array_equal(b["input"][:, 0], g[f"{name}/input"][:, 0]), name
            assert np.array_equal(b["target"], g[f"{name}/target"]), name
    # without a ground-truth raster: no target, no mask
    from resdepth_amd import GpuTrainSet
    np.random.seed(0)
    nogt = GpuTrainSet([dict(sampler=_sampler(g, "city", None, gt=False), area_defn={"x_extent": [(0, 111)], "y_extent": [(0, 79)]},
                             n_samples=7, image_pairs=[[0, 1]])], "geom-stereo", batch_size=4, augment=False)
    b = _collect(nogt)
    assert set(b) == KEYS - {"target", "loss_mask"} and b["input"].shape == (7, 3, 16, 16) and np.isfinite(b["input"]).all()


def _two_rasters(tile):
    """Two synthetic rasters of different shape (one with rows that are not 16-byte multiples), nodata holes, zeros in the target."""
    from resdepth_amd import GpuPatchSampler
    out = []
    for k, (h, w) in enumerate(((256, 272), (300, 262))):
        rng = np.random.RandomState(40 + k)
        dsm = (rng.randn(h, w) * 4 + 420 + 900 * k).astype(np.float32)
        gt = (dsm + rng.randn(h, w)).astype(np.float32)
        dsm[20:40, 50:90] = -9999.0
        gt[100:120, 30:60] = -9999.0
        gt[::37, ::41] = 0.0
        orthos = (rng.rand(3, h, w) * 200 + 20).astype(np.float32)
        out.append(GpuPatchSampler(dsm, gt, orthos, tile_size=tile, nodata=-9999.0, dsm_std=3.0 + k, ortho_mean=None if k else 110.0,
                                   ortho_std=50.0 - 5 * k))
    return out


def test_mixed_raster_batch_equals_the_per_raster_sampler_bit_for_bit(g):
    from resdepth_amd import GpuTrainSet
    for tile, samplers in ((16, [_sampler(g, "flat", None), _sampler(g, "city", 51.5)]), (64, _two_rasters(64))):
        np.random.seed(11)
        datasets = [dict(sampler=s, area_defn={"x_extent": [(0, s.w - 1)], "y_extent": [(0, s.h - 1)]}, n_samples=20,
                         image_pairs=[[0, 1], [1, 2], [2, 0]]) for s in samplers]
        ts = GpuTrainSet(datasets, "geom-stereo", batch_size=40)
        ids, pos, pidx = ts.sample_list()
        n = len(ids)
        assert n == 40
        pos = pos.copy()
        pos[::3, 1] &= ~3                                    # some patches with 16-byte aligned rows
        ts._cols[2] = pos[:, 1]
        aug = np.array([[j % 4, (j // 4) % 2, (j // 8) % 2] for j in range(n)])             # every code, on both rasters
        aug[20:] = np.array([[(j + 1) % 4, (j // 8) % 2, (j // 4) % 2] for j in range(20)])
        assert len({tuple(a) for a in aug[:20]}) == 16 and len({tuple(a) for a in aug[20:]}) == 16
        planes = np.array([[0, 1], [1, 2], [2, 0]])[pidx]
        planes[1::2] = planes[1::2, ::-1]                    # permuted pairs
        order = np.random.RandomState(3).permutation(n)      # the rasters interleaved in one batch
        b = ts.assemble(order, aug[order], planes[order])
        for k, s in enumerate(samplers):
            sel = np.nonzero(ids[order] == k)[0]
            ref = s.sample(pos[order][sel], planes[order][sel], aug[order][sel])
            for key in ("input", "target", "loss_mask", "dsm_mean"):
                assert torch.equal(b[key][sel], ref[key]), (tile, k, key)
            assert torch.equal(b["dsm_std"][sel], ref["dsm_std"]) and torch.equal(b["nodata"][sel], ref["nodata"])
        # the stand-in, augmentation included
        o = order[5]
        s = samplers[ids[o]]
        want = R.train_sample(s.dsm_in.cpu().numpy(), s.dsm_gt.cpu().numpy(), s.orthos.cpu().numpy().transpose(1, 2, 0), pos[o],
                              planes[o], tile, -9999.0, s.dsm_std, s.ortho_mean, s.ortho_std, "geom-stereo", aug=aug[o])
        np.testing.assert_allclose(b["input"][5].cpu().numpy(), want["input"], rtol=0, atol=3e-5)
        np.testing.assert_array_equal(b["loss_mask"][5].cpu().numpy(), want["loss_mask"])
        # a sample's bits do not depend on its batch mates
        one = ts.assemble(order[7:8], aug[order[7:8]], planes[order[7:8]])
        assert torch.equal(one["input"][0], b["input"][7]) and torch.equal(one["target"][0], b["target"][7])


def _epoch_set(g, batch_size, prefetch, seed=5, **kw):
    from resdepth_amd import GpuTrainSet
    np.random.seed(21)
    datasets = [dict(sampler=_sampler(g, "flat", None), area_defn={"x_extent": [(0, 63)], "y_extent": [(0, 47)]}, n_samples=30,
                     image_pairs=[[0, 1], [1, 2]]),
                dict(sampler=_sampler(g, "city", None), area_defn={"x_extent": [(0, 31), (70, 105)], "y_extent": [(0, 15), (40, 71)]},
                     n_samples=37, image_pairs=[[0, 1], [1, 2], [0, 2]])]
    args = dict(batch_size=batch_size, prefetch=prefetch, permute_images_within_pair=True,
                generator=torch.Generator().manual_seed(seed))
    args.update(kw)
    return GpuTrainSet(datasets, "geom-stereo", **args)


def test_an_epoch_does_not_depend_on_batch_size_or_prefetch_depth(g):
    ref = _collect(_epoch_set(g, 32, 1))
    assert ref["input"].shape == (67, 3, 16, 16) and np.isfinite(ref["input"]).all()
    for bs, pf in ((1, 0), (5, 2), (32, 0), (32, 2)):
        loader = _epoch_set(g, bs, pf)
        assert len(loader) == -(-67 // bs)
        sizes = [b["input"].shape[0] for b in loader]                 # a second epoch: the last batch is ragged
        assert sizes == [bs] * (67 // bs) + ([67 % bs] if 67 % bs else [])
        got = _collect(_epoch_set(g, bs, pf))
        for k, v in ref.items():
            assert np.array_equal(got[k], v, equal_nan=True), (bs, pf, k)
    # shards: equally many samples per rank, together the cut permutation
    parts = [_collect(_epoch_set(g, 8, 1, augment=False, permute_images_within_pair=False, shard=(r, 3))) for r in range(3)]
    assert all(p["input"].shape[0] == 22 for p in parts)
    whole = _collect(_epoch_set(g, 8, 1, augment=False, permute_images_within_pair=False))
    inter = np.stack([p["input"] for p in parts], 1).reshape(66, 3, 16, 16)
    assert np.array_equal(inter, whole["input"][:66])


def test_two_epochs_reshuffle_the_same_samples(g):
    loader = _epoch_set(g, 16, 1, augment=False, permute_images_within_pair=False)
    a, b = _collect(loader), _collect(loader)                          # one generator: its state advances

    def key(d):
        return np.lexsort((d["input"].reshape(67, -1).sum(1), d["patch_offset_x"], d["patch_offset_y"], d["dsm_std"]))
    assert not np.array_equal(a["patch_offset_y"], b["patch_offset_y"]) or not np.array_equal(a["patch_offset_x"], b["patch_offset_x"])
    ka, kb = key(a), key(b)
    for k in a:
        assert np.array_equal(a[k][ka], b[k][kb], equal_nan=True), k
    fixed = _collect(_epoch_set(g, 16, 1, augment=False, permute_images_within_pair=False, shuffle=False))
    ids, pos, _ = loader.sample_list()
    np.testing.assert_array_equal(fixed["patch_offset_y"], pos[:, 0])


def test_trainer_runs_from_a_train_set_and_grid_tiles(tmp_path):
    from resdepth_amd import FusedAdam, GpuGridTiles, GpuTrainSet, Trainer, UNet
    s0, s1 = _two_rasters(64)
    np.random.seed(2)
    train = GpuTrainSet([dict(sampler=s0, area_defn={"x_extent": [(0, 271)], "y_extent": [(0, 191)]}, n_samples=13,
                              image_pairs=[[0, 1], [1, 2]]),
                         dict(sampler=s1, area_defn={"x_extent": [(0, 261)], "y_extent": [(0, 299)]}, n_samples=10,
                              image_pairs=[[0, 1], [1, 2]])], "geom-stereo", batch_size=8, permute_images_within_pair=True,
                        generator=torch.Generator().manual_seed(1))
    assert len(train) == 3 and len(train.dataset) == 23
    val = GpuGridTiles(s0, "val", {"x_extent": [(0, 271)], "y_extent": [(192, 255)]}, "geom-stereo", [[0, 1]], batch_size=4)
    torch.manual_seed(1)
    model = UNet(n_input_channels=3, start_kernel=8, depth=3, bias_conv_layer=True).to("cuda:0").train()
    opt = FusedAdam(model.parameters(), lr=1e-3)
    args = types.SimpleNamespace(
        model=model, optimizer=opt, scheduler=None, criterion=torch.nn.L1Loss(reduction="mean"), trainloader=train,
        valloader=val, n_epochs=2, evaluate_rate=1, save_model_rate=10 ** 9, freq_average_train_loss=20,
        save_dir=str(tmp_path), log_file=None, checkpoint_dir=os.path.join(str(tmp_path), "checkpoints"),
        tboard_log_dir=os.path.join(str(tmp_path), "tb"), pretrained_path=None)
    tr = Trainer(args)
    tr.logger.handlers.clear()
    assert tr.batch_size == 8
    tr.train()
    assert os.path.isfile(os.path.join(str(tmp_path), "checkpoints", "Model_best.pth")) and np.isfinite(tr.best_loss)


def test_bad_arguments_are_refused(g):
    from resdepth_amd import GpuTrainSet, normalization as N
    city, flat = _sampler(g, "city", None), _sampler(g, "flat", None)
    area = {"x_extent": [(0, 111)], "y_extent": [(0, 79)]}
    ok = dict(sampler=city, area_defn=area, n_samples=5, image_pairs=[[0, 1]])
    GpuTrainSet([ok], "geom-stereo", batch_size=4)
    for ds, kw in (([dict(ok, area_defn={"x_extent": [(0, 200)], "y_extent": [(0, 79)]})], {}),      # outside the raster
                   ([dict(ok, area_defn={"x_extent": [(0, 14)], "y_extent": [(0, 79)]})], {}),       # holds no tile
                   ([dict(ok, n_samples=10 ** 6)], {}),
                   ([dict(ok, image_pairs=[[0, 7]])], {}),
                   ([dict(ok, image_pairs=None)], {}),
                   ([ok, dict(ok, sampler=_sampler(g, "flat", None, tile=8), area_defn={"x_extent": [(0, 63)], "y_extent": [(0, 47)]})], {}),
                   ([ok, dict(ok, image_pairs=[[0]])], {}),                                           # view counts differ
                   ([ok, dict(ok, sampler=_sampler(g, "city", None, gt=False))], {}),
                   ([dict(ok, sampler="city")], {}), ([], {}),
                   ([ok], dict(input_channels="rgb")), ([ok], dict(batch_size=0)), ([ok], dict(shard=(2, 2)))):
        args = dict(input_channels="geom-stereo", batch_size=4)
        args.update(kw)
        with pytest.raises(ValueError):
            GpuTrainSet(ds, **args)
    with pytest.raises(ValueError):
        N.compute_local_dsm_std_per_centered_patch([(flat, [[40, 10]])])                  # outside the raster
    with pytest.raises(ValueError):
        N.compute_local_dsm_std_per_centered_patch([(flat, [[0, 0]])], raster_identifier="raster")
    with pytest.raises(ValueError):
        N.compute_satellite_image_normalization([(flat, [[0, 1]], {"x_extent": [(0, 64)], "y_extent": [(0, 47)]})])
    with pytest.raises(ValueError):
        N.compute_satellite_image_normalization([(flat, [[0, 3]], {"x_extent": [(0, 63)], "y_extent": [(0, 47)]})])


def test_statistics_match_the_float128_reference(g):
    from resdepth_amd import normalization as N
    samplers = {rn: _sampler(g, rn, None) for rn in ("flat", "city")}
    for name in ("std21", "std30"):
        ids, pos = g[f"{name}/dataset_id"], g[f"{name}/pos"]
        groups = [(samplers[rn], pos[ids == k]) for k, rn in enumerate(("flat", "city"))]
        for ident in ("raster_in", "raster_gt"):
            want = g[f"{name}/{ident}/stds"]
            stds = N.local_dsm_stds(groups, ident)
            rel = np.abs(stds - want) / want
            print(name, ident, "per-patch std: max rel err", rel.max(), "flat raster", rel[ids == 0].max())
            assert np.all(rel <= REL), (name, ident, rel.max())
            value, ref = N.compute_local_dsm_std_per_centered_patch(groups, ident), float(g[f"{name}/{ident}/std"])
            print(name, ident, "trimmed mean", value, "reference", ref, "rel err", abs(value - ref) / ref)
            assert isinstance(value, float) and abs(value - ref) <= REL * ref
    # one position list passed whole, reversed, and in chunks of 1 and 7: the same bits
    pos = np.concatenate([g["std30/pos"][g["std30/dataset_id"] == 0], g["std21/pos"][g["std21/dataset_id"] == 0]])
    for ident in ("raster_in", "raster_gt"):
        whole = N.patch_moments(samplers["flat"], pos, ident).cpu()
        assert torch.equal(N.patch_moments(samplers["flat"], pos[::-1].copy(), ident).cpu().flip(0), whole)
        for step in (1, 7):
            parts = [N.patch_moments(samplers["flat"], pos[k:k + step], ident).cpu() for k in range(0, len(pos), step)]
            assert torch.equal(torch.cat(parts), whole), (ident, step)
    # ortho-image mean / std: the fp64 stand-in at the statistics' bar, the reference's float32 reduction at 1e-6
    norm = json.loads(str(g["norm/settings"]))
    mean, std = N.compute_satellite_image_normalization([(samplers[d["raster"]], d["pairs"], d["area"]) for d in norm])
    m64, s64 = R.image_normalization([(g[f"{d['raster']}/orthos_u8"].astype(np.float32), d["pairs"], d["area"]) for d in norm])
    print("ortho mean / std", mean, std, "stand-in", m64, s64, "reference", float(g["norm/mean"]), float(g["norm/std"]))
    assert abs(mean - m64) <= REL * m64 and abs(std - s64) <= REL * s64
    assert abs(mean - float(g["norm/mean"])) <= 1e-6 * mean and abs(std - float(g["norm/std"])) <= 1e-6 * std


def test_statistics_on_a_1024_raster_with_256_tiles():
    from resdepth_amd import GpuPatchSampler, normalization as N
    rng = np.random.RandomState(12)
    h = w = 1024
    yy, xx = np.mgrid[0:h, 0:w]
    dsm = (2400.0 + 0.4 * np.sin(yy / 90.0) * np.cos(xx / 70.0) + rng.rand(h, w) * 0.2).astype(np.float32)     # flat and high
    gt = (dsm + rng.randn(h, w) * 0.05).astype(np.float32)
    dsm[100:140, 200:260] = -9999.0
    dsm[700:705, 20:900] = -9999.0
    gt[300:330, 400:470] = -9999.0
    orthos = rng.randint(0, 2048, (3, h, w)).astype(np.float32)
    smp = GpuPatchSampler(dsm, gt, orthos, tile_size=256, nodata=-9999.0)
    pos = np.stack([rng.randint(0, h - 255, 2000), rng.randint(0, w - 255, 2000)], 1)
    pos[::5, 1] &= ~3
    for ident, plane in (("raster_in", dsm), ("raster_gt", gt)):
        want = R.patch_stds(plane, pos, 256, -9999.0)
        got = N.local_dsm_stds([(smp, pos)], ident)
        rel = np.abs(got - want) / want
        print(ident, "2000 patches of 256^2: max rel err", rel.max())
        assert np.all(rel <= REL), rel.max()
        value = N.compute_local_dsm_std_per_centered_patch([(smp, pos[:1000]), (smp, pos[1000:])], ident)
        assert abs(value - R.trimmed_mean(want)) <= REL * value
        m = N.patch_moments(smp, pos[:50], ident).cpu().numpy()
        ref = R.patch_moments(plane, pos[:50], 256, -9999.0)
        assert np.array_equal(m[:, 0], ref[:, 0]) and np.all(np.abs(m[:, 1] - ref[:, 1]) <= REL * ref[:, 1])
    area = {"x_extent": [(3, 1000), (513, 1023)], "y_extent": [(0, 611), (600, 1023)]}
    mean, std = N.compute_satellite_image_normalization([(smp, [[0, 2], [2, 1]], area), (smp, [[1, 1]], {"x_extent": [(0, 1023)], "y_extent": [(5, 5)]})])
    hwv = orthos.transpose(1, 2, 0)
    m64, s64 = R.image_normalization([(hwv, [[0, 2], [2, 1]], area), (hwv, [[1, 1]], {"x_extent": [(0, 1023)], "y_extent": [(5, 5)]})])
    print("1024^2 ortho mean / std rel err", abs(mean - m64) / m64, abs(std - s64) / s64)
    assert abs(mean - m64) <= REL * m64 and abs(std - s64) <= REL * s64
    hole = GpuPatchSampler(np.full((300, 300), -9999.0, dtype=np.float32), None, None, tile_size=256, nodata=-9999.0)
    with pytest.raises(ValueError, match="valid pixels"):
        N.compute_local_dsm_std_per_centered_patch([(smp, pos[:3]), (hole, [[10, 20]])])
