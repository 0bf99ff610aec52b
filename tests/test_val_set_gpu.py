"""The multi-dataset, rank-sharded validation set on the GPU (GpuValSet, rd_assemble_train_patches with RD_TRAIN_AUG_BOX;
-m gpu): every sample of the reference's own ConcatDataset of 'val' datasets (g21 fixture), each dataset's part against
GpuGridTiles on that dataset alone, the extended entry point on ragged shapes inside guard bands, rank shards against the
unsharded loader, and the Trainer's validation metric against a host DataLoader over the numpy stand-in."""
import json
import os
import struct
import types

import numpy as np
import pytest
import torch
from torch.utils.data import ConcatDataset, DataLoader

import grid_tiles_ref as R
from arena import Arena, nbytes_of
from conftest import load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = {"input", "target", "loss_mask", "dsm_mean", "dsm_std", "nodata"} | set(R.META)


@pytest.fixture(scope="module")
def g():
    return load_npz("g21_valset.npz")


def _settings(g):
    return [json.loads(str(g[f"d{d}/settings"])) for d in range(int(g["n_datasets"]))]


def _g21_datasets(g, pairs=None):
    """The fixture's datasets for GpuValSet (module-level cache of the resident rasters); pairs: per dataset, how many of its
    pairs to keep."""
    from resdepth_amd import GpuPatchSampler
    out = []
    for d, c in enumerate(_settings(g)):
        key = ("g21", d)
        if key not in _SAMPLERS:
            orth = np.ascontiguousarray(g[f"d{d}/orthos_u8"].astype(np.float32).transpose(2, 0, 1))
            _SAMPLERS[key] = GpuPatchSampler(g[f"d{d}/dsm_in"], g[f"d{d}/dsm_gt"], orth, tile_size=int(g["tile"]), nodata=c["nodata"],
                                             dsm_std=c["dsm_std"], ortho_mean=c["ortho_mean"], ortho_std=c["ortho_std"])
        out.append(dict(sampler=_SAMPLERS[key], area_defn=c["area"], image_pairs=c["pairs"][:pairs[d]] if pairs else c["pairs"],
                        dsm_mean=c["dsm_mean"]))
    return out


_SAMPLERS = {}


def _batches(loader):
    return [{k: v.cpu() for k, v in b.items()} for b in loader]


def _cat(batches):
    return {k: torch.cat([b[k] for b in batches]).numpy() for k in batches[0]}


def test_every_reference_sample_and_the_dataloaders_batches(g):
    from resdepth_amd import GpuValSet
    loader = GpuValSet(_g21_datasets(g), str(g["channels"]), batch_size=5)
    n = len(g["pos"])
    n0 = int((g["dataset_id"] == 0).sum())
    assert n0 % 5 != 0                                               # a batch straddles the two rasters
    ds = loader.dataset
    assert len(ds) == n and len(loader) == len(g["batch_sizes"]) and not loader.drop_last and ds.tile_size == int(g["tile"])
    np.testing.assert_array_equal(ds.dataset_id, g["dataset_id"])
    np.testing.assert_array_equal(ds.pos, g["pos"])
    np.testing.assert_array_equal(ds.reg, g["reg"])
    np.testing.assert_array_equal(ds.pair_idx, g["pair_idx"])
    batches = _batches(loader)
    assert [len(b["input"]) for b in batches] == g["batch_sizes"].tolist()          # the reference DataLoader's batching
    assert all(set(b) == KEYS for b in batches)
    b = _cat(batches)
    assert b["input"].shape == g["input"].shape and b["input"].dtype == np.float32
    print("max |input| / |target| error", np.abs(b["input"] - g["input"]).max(), np.abs(b["target"] - g["target"]).max())
    np.testing.assert_allclose(b["input"], g["input"], rtol=0, atol=3e-5)
    np.testing.assert_allclose(b["target"], g["target"], rtol=0, atol=3e-5)
    assert b["dsm_mean"].dtype == np.float32 and np.all(np.abs(b["dsm_mean"] - g["dsm_mean"]) <= 1e-6 * np.abs(g["dsm_mean"]))
    assert b["loss_mask"].dtype == np.bool_
    np.testing.assert_array_equal(b["loss_mask"], g["loss_mask"])
    assert g["loss_mask"].any() and not g["loss_mask"].all()
    for j, k in enumerate(R.META):
        assert b[k].dtype == np.int64
        np.testing.assert_array_equal(b[k], g["meta"][:, j], err_msg=k)
    np.testing.assert_array_equal(b["nodata"], g["scalars"][:, 0].astype(np.float32))          # per sample: the rasters' own
    np.testing.assert_array_equal(b["dsm_std"], g["scalars"][:, 1].astype(np.float32))
    assert len(set(b["nodata"])) == 2 and len(set(b["dsm_std"])) == 2
    # a given mean involves no reduction: bit-exact planes
    for d, c in enumerate(_settings(g)):
        sel = g["dataset_id"] == d
        if c["ortho_mean"]:
            assert np.array_equal(b["input"][sel, 1:], g["input"][sel, 1:]), d
        if c["dsm_mean"]:
            assert np.array_equal(b["input"][sel, 0], g["input"][sel, 0]) and np.array_equal(b["target"][sel], g["target"][sel]), d
    assert [bool(c["ortho_mean"]) for c in _settings(g)] == [True, False]
    assert [bool(c["dsm_mean"]) for c in _settings(g)] == [False, True]
    # batch size and prefetch depth do not change a sample
    for kw in (dict(batch_size=7, prefetch=0), dict(batch_size=48, prefetch=3)):
        again = _cat(_batches(GpuValSet(_g21_datasets(g), str(g["channels"]), **kw)))
        assert all(np.array_equal(again[k], b[k], equal_nan=True) for k in KEYS), kw


def test_each_datasets_part_equals_gpu_grid_tiles_on_it_alone(g):
    """Against the code that exists.  The two paths sum a tile in different orders (train_patch_sums: one block per tile;
    grid_tile_sums: slabs), but the g21 rasters hold multiples of 0.25 below 2^10 and integer radiances below 2^8: any partial
    sum of 3 * 256 such values is exact in fp64, so the order cannot matter and the means -- hence every normalised plane --
    must be the same bits."""
    from resdepth_amd import GpuGridTiles, GpuValSet
    datasets = _g21_datasets(g)
    b = _cat(_batches(GpuValSet(datasets, str(g["channels"]), batch_size=5)))
    for d, ds in enumerate(datasets):
        alone = GpuGridTiles(ds["sampler"], "val", ds["area_defn"], str(g["channels"]), ds["image_pairs"], dsm_mean=ds["dsm_mean"],
                             batch_size=7)
        a = _cat(_batches(alone))
        sel = g["dataset_id"] == d
        assert set(a) == KEYS and len(a["input"]) == sel.sum()
        for k in KEYS:
            assert a[k].dtype == b[k].dtype, k
            assert np.array_equal(a[k], b[k][sel], equal_nan=True), (d, k)


# ---- the extended entry point, directly, on ragged shapes inside guard bands ------------------------------------------------
def _raster(h, w, seed, nodata):
    rng = np.random.RandomState(seed)
    dsm = (rng.randn(h, w) * 3 + 50).astype(np.float32)
    gt = (dsm + rng.randn(h, w)).astype(np.float32)
    dsm[rng.rand(h, w) < 0.05] = nodata
    gt[rng.rand(h, w) < 0.08] = nodata
    gt[rng.rand(h, w) < 0.05] = 0.0
    return dsm, gt, (rng.rand(3, h, w) * 200).astype(np.float32)


def _augmented(a, aug):
    a = np.rot90(a, aug & 3)
    if aug & 4:
        a = np.flipud(a)
    if aug & 8:
        a = np.fliplr(a)
    return a


@pytest.mark.parametrize("tile,bad_box", [(8, (5, 1, 4, 6)), (8, (1, 6, 6, 5)), (12, (0, 0, 11, 12)), (12, (0, -1, 11, 11))])
def test_entry_point_flagged_and_unflagged_samples_inside_guard_bands(tile, bad_box):
    from resdepth_amd._lib import check, load, ptr, stream_ptr
    lib = load()
    n, views, nodata = 5, 2, -9999.0
    dims = [(37, 45), (33, 19)]
    ras = [_raster(h, w, 60 + r, nodata) for r, (h, w) in enumerate(dims)]
    f32 = lambda v: struct.unpack("<i", struct.pack("<f", v))[0]      # noqa: E731
    good = (1, 2, tile - 2, tile - 4)
    # (flagged, aug bits, box): an unflagged sample carries garbage where a box would be
    plan = [(0, 5, (1 << 30, -7, 1 << 30, 99)), (1, 0, good), (1, 2 | 8, (0, 3, tile - 1, 3)), (1, 3, bad_box), (0, 12, (-5, -5, -5, -5))]
    cols = []
    for i, (flag, aug, box) in enumerate(plan):
        r = i % 2
        h, w = dims[r]
        y, x = (h - tile, w - tile) if i >= 3 else ((5 * i + 1) % (h - tile + 1), (3 * i + 2) % (w - tile + 1))
        cols.append([r, y, x, aug | (16 if flag else 0), i % 3, f32(49.5), 0, 0] + [(i + j) % 3 for j in range(views)] + list(box))
    tab_new = torch.tensor(cols, dtype=torch.int32).t().contiguous()                         # [8 + V + 4, n]
    tab_old = tab_new[:8 + views].clone()
    tab_old[3] &= 15                                                                         # today's layout, nobody flagged
    shapes = {"input": ((n, 1 + views, tile, tile), torch.float32), "target": ((n, 1, tile, tile), torch.float32),
              "mask": ((n, 1, tile, tile), torch.uint8), "dsm_mean_out": ((n,), torch.float32), "sums": ((n, 4), torch.float64)}
    ins = [t_ for r_ in ras for t_ in r_]
    sizes = [nbytes_of(s, d) for s, d in shapes.values()] + [a.nbytes for a in ins] + [64 * 2, tab_new.numel() * 4]

    def launch(table):
        ar = Arena(DEV, sizes)
        dev = [[ar.alloc(a.shape, torch.float32, fill=torch.from_numpy(a), name=f"r{r}_{j}") for j, a in enumerate(r_)]
               for r, r_ in enumerate(ras)]
        desc = b"".join(struct.pack("<QQQiiiffiffii", a.data_ptr(), b_.data_ptr(), c.data_ptr(), h, w, 3, nodata, 2.5 + r, r + 1,
                                    110.0, 60.0, 0, 0) for r, ((a, b_, c), (h, w)) in enumerate(zip(dev, dims)))
        d_desc = ar.alloc(len(desc), torch.uint8, fill=torch.frombuffer(bytearray(desc), dtype=torch.uint8), name="rasters")
        d_tab = ar.alloc(table.shape, torch.int32, fill=table, name="samples")          # the guard band follows its last column
        out = {k: ar.alloc(s, d, kind="output" if k != "sums" else "scratch", name=k) for k, (s, d) in shapes.items()}
        check(lib.rd_assemble_train_patches(ptr(d_desc), 2, ptr(d_tab), n, views, 1, tile, ptr(out["input"]), ptr(out["target"]),
                                            ptr(out["mask"]), ptr(out["dsm_mean_out"]), ptr(out["sums"]), stream_ptr()), "call")
        ar.check()                         # synchronises; every guard byte and every input (rasters, tables) unchanged
        assert all(ar.unwritten(out[k]) == 0 for k in ("input", "target", "mask", "dsm_mean_out"))
        return {k: v.cpu().numpy().copy() for k, v in out.items() if k != "sums"}

    with torch.cuda.device(DEV):
        old, new = launch(tab_old), launch(tab_new)
    # nothing but the flagged samples' masks depends on the flag or the extra columns
    for k in ("input", "target", "dsm_mean_out"):
        assert np.array_equal(old[k], new[k], equal_nan=True) and np.isfinite(new[k]).all(), k
    for i, (flag, aug, box) in enumerate(plan):
        y, x = cols[i][1], cols[i][2]
        gt = ras[i % 2][1][y:y + tile, x:x + tile]
        valid = _augmented((gt != 0) & (gt != np.float32(nodata)), aug)
        assert np.array_equal(old["mask"][i, 0].astype(bool), valid), i        # today's layout: the whole tile
        if not flag:
            assert np.array_equal(new["mask"][i], old["mask"][i]), i
            continue
        inside = np.zeros((tile, tile), dtype=bool)
        uly, ulx, lry, lrx = box
        if 0 <= uly <= lry < tile and 0 <= ulx <= lrx < tile:
            inside[uly:lry + 1, ulx:lrx + 1] = True
        assert np.array_equal(new["mask"][i, 0].astype(bool), valid & inside), (i, box)
        assert set(np.unique(new["mask"][i])) <= {0, 1}
        if box == bad_box:
            assert not new["mask"][i].any() and valid.any()
        else:
            assert new["mask"][i].any() and (valid & ~inside).any()          # the box cuts something off


# ---- shards in one process ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,cases", [(2, [((2, 2), 4, "split"), ((1, 1), 3, "replicated")]),
                                         (3, [((3, 1), 3, "split"), ((2, 2), 2, "replicated")])])
def test_rank_shards_concatenate_to_the_global_batches(g, world, cases):
    from resdepth_amd import GpuValSet
    ch = str(g["channels"])
    seen = set()
    for pairs, b, tail in cases:
        datasets = _g21_datasets(g, pairs)
        for d in datasets:
            d["area_defn"] = dict(d["area_defn"])
        datasets[1]["area_defn"] = {"x_extent": [(3, 50)], "y_extent": [(2, 41)]}          # 9 positions: odd sample counts occur
        whole = GpuValSet(datasets, ch, batch_size=b * world)
        n = len(whole.dataset)
        ranks = [GpuValSet(datasets, ch, batch_size=b, shard=(r, world)) for r in range(world)]
        assert all(len(x) == len(whole) for x in ranks)
        rest = n % (b * world)
        assert rest and (rest % world == 0) == (tail == "split"), (n, b, world)
        assert all(len(x.dataset) == n // (b * world) * b + (rest // world if tail == "split" else rest) for x in ranks)
        got = [_batches(x) for x in ranks]
        for k, full in enumerate(_batches(whole)):
            parts = [got[r][k] for r in range(world)]
            assert len({len(p["input"]) for p in parts}) == 1
            if k == len(whole) - 1 and tail == "replicated":
                for p in parts:
                    for key in KEYS:
                        assert np.array_equal(p[key].numpy(), full[key].numpy(), equal_nan=True), (k, key)
                seen.add("replicated")
            else:
                for key in KEYS:
                    cat = torch.cat([p[key] for p in parts])
                    assert np.array_equal(cat.numpy(), full[key].numpy(), equal_nan=True), (k, key)
                if k == len(whole) - 1:
                    seen.add("split")
        # a rank's sample list is what it yields
        for r, x in enumerate(ranks):
            np.testing.assert_array_equal(_cat(got[r])["patch_offset_y"], x.dataset.pos[:, 0])
            np.testing.assert_array_equal(x.dataset.dataset_id, whole.dataset.dataset_id[x.dataset.index])
    assert seen == {"split", "replicated"}


# ---- the Trainer -------------------------------------------------------------------------------------------------------------
T = 64
SHAPES = ((256, 320), (192, 256))
PAIRS = ([[0, 1], [1, 0]], [[1, 0]])
NODATA, STD, OMEAN, OSTD = (-9999.0, -5000.0), (3.0, 4.5), (110.0, 95.0), (50.0, 44.0)


@pytest.fixture(scope="module")
def scene():
    out = []
    for k, (h, w) in enumerate(SHAPES):
        rng = np.random.RandomState(70 + k)
        dsm = (rng.randn(h, w) * 4 + 420 + 300 * k).astype(np.float32)
        gt = (dsm + rng.randn(h, w) * 1.5).astype(np.float32)
        dsm[100:104, 20:200] = NODATA[k]
        gt[30:60, 140:170] = NODATA[k]
        gt[::37, ::41] = 0.0
        out.append((dsm, gt, (rng.rand(h, w, 2) * 200 + 20).astype(np.float32)))
    return out


def _model(seed=0):
    from resdepth_amd import UNet
    torch.manual_seed(seed)
    return UNet(n_input_channels=3, start_kernel=8, depth=3, bias_conv_layer=True).to(DEV).eval()


def _trainer_args(tmp, model, opt, train, val, n_epochs):
    return types.SimpleNamespace(
        model=model, optimizer=opt, scheduler=None, criterion=torch.nn.L1Loss(reduction="mean"), trainloader=train,
        valloader=val, n_epochs=n_epochs, evaluate_rate=1, save_model_rate=10 ** 9, freq_average_train_loss=20,
        save_dir=str(tmp), log_file=None, checkpoint_dir=os.path.join(str(tmp), "checkpoints"),
        tboard_log_dir=os.path.join(str(tmp), "tb"), pretrained_path=None)


def scene_datasets(scene):
    from resdepth_amd import GpuPatchSampler
    out = []
    for k, (dsm, gt, orthos) in enumerate(scene):
        h, w = dsm.shape
        smp = GpuPatchSampler(dsm, gt, np.ascontiguousarray(orthos.transpose(2, 0, 1)), tile_size=T, nodata=NODATA[k], dsm_std=STD[k],
                              ortho_mean=OMEAN[k], ortho_std=OSTD[k])
        out.append(dict(sampler=smp, area_defn={"x_extent": [(0, w - 1)], "y_extent": [(0, h - 1)]}, image_pairs=PAIRS[k], n_samples=8))
    return out


def test_validation_metric_matches_host_batches_and_training_runs(scene, tmp_path):
    from resdepth_amd import FusedAdam, GpuTrainSet, GpuValSet, Trainer
    datasets = scene_datasets(scene)
    val = GpuValSet(datasets, "geom-stereo", batch_size=12)
    ds = val.dataset
    n0 = int((ds.dataset_id == 0).sum())
    assert len(ds) == 4 * 5 * 2 + 3 * 4 and n0 == 40 and n0 % 12 != 0                 # a batch straddles the rasters
    train = GpuTrainSet(datasets, "geom-stereo", batch_size=8, generator=torch.Generator().manual_seed(1),
                        rng=np.random.RandomState(3))
    model = _model(1).train()
    opt = FusedAdam(model.parameters(), lr=1e-3)
    tr = Trainer(_trainer_args(tmp_path / "a", model, opt, train, val, 1))
    tr.logger.handlers.clear()

    def host(means=None):
        parts = []
        for k, (dsm, gt, orthos) in enumerate(scene):
            sel = np.flatnonzero(ds.dataset_id == k)
            pairs = [PAIRS[k][i] for i in ds.pair_idx[sel]]
            parts.append(R.StandInGridDataset(dsm, gt, orthos, [tuple(p) for p in ds.pos[sel]], [tuple(r) for r in ds.reg[sel]], pairs, T,
                                              T, NODATA[k], STD[k], OMEAN[k], OSTD[k], "geom-stereo",
                                              mean_override=None if means is None else means[sel]))
        return DataLoader(ConcatDataset(parts), batch_size=12, shuffle=False)

    m_gpu = tr.inference_one_epoch(0, "val")["MAE_metric"].avg
    gpu_means = _cat(_batches(val))["dsm_mean"]
    tr.loader["val"] = host()
    m_host = tr.inference_one_epoch(0, "val")["MAE_metric"].avg
    print("validation metric: GpuValSet", m_gpu, "host DataLoader", m_host)
    assert abs(m_gpu - m_host) <= 1e-4 * abs(m_host), (m_gpu, m_host)
    tr.loader["val"] = host(gpu_means)                   # the GPU loader's means: bit-identical inputs, the same metric
    assert tr.inference_one_epoch(0, "val")["MAE_metric"].avg == m_gpu
    # the full loop: GpuTrainSet for training, GpuValSet for validation, one resident raster set
    tr.loader["val"] = val
    tr.train()
    assert os.path.isfile(os.path.join(str(tmp_path / "a"), "checkpoints", "Model_best.pth"))
    assert np.isfinite(tr.best_loss)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(g):
    from resdepth_amd import GpuGridTiles, GpuPatchSampler, GpuValSet
    ch = str(g["channels"])
    base = _g21_datasets(g)
    GpuValSet(base, ch, batch_size=4)                                                      # the arguments below differ in one thing
    s0 = base[0]["sampler"]
    orth = s0.orthos.cpu().numpy()
    other_tile = GpuPatchSampler(s0.dsm_in.cpu(), s0.dsm_gt.cpu(), orth, tile_size=8)
    no_gt = GpuPatchSampler(s0.dsm_in.cpu(), None, orth, tile_size=16)
    swap = lambda d, **kw: [dict(base[0], **kw) if d == 0 else base[0], dict(base[1], **kw) if d == 1 else base[1]]    # noqa: E731
    bad = [
        dict(datasets=[]),
        dict(datasets=swap(1, sampler=other_tile)),                                                       # tile size
        dict(datasets=swap(1, image_pairs=[[0], [1]])),                                                   # view count
        dict(datasets=swap(0, sampler=no_gt)),                                                            # mixed ground truth
        dict(datasets=[dict(base[0], sampler=no_gt)]),                                                    # no ground truth at all
        dict(datasets=swap(1, area_defn={"x_extent": [(3, 96)], "y_extent": [(2, 41)]})),                 # outside its raster
        dict(datasets=swap(1, area_defn={"x_extent": [(3, 17)], "y_extent": [(2, 41)]})),                 # smaller than a tile
        dict(datasets=swap(1, area_defn={"x_extent": [(3, 60), (0, 20)], "y_extent": [(2, 41)]})),
        dict(datasets=swap(1, image_pairs=[[0, 2]])),                                                     # plane index (2 planes)
        dict(datasets=swap(0, image_pairs=[[0, -1]])),
        dict(datasets=swap(0, image_pairs=[[0, 1], [2]])),                                                # ragged pairs
        dict(datasets=swap(0, image_pairs=None)),
        dict(augment=True), dict(permute_images_within_pair=True),
        dict(shard=(2, 2)), dict(batch_size=0), dict(input_channels="rgb"), dict(stride=17),
    ]
    if torch.cuda.device_count() > 1:
        bad.append(dict(datasets=swap(1, sampler=GpuPatchSampler(s0.dsm_in.cpu(), s0.dsm_gt.cpu(), orth, tile_size=16, device="cuda:1"))))
    for kw in bad:
        args = dict(datasets=base, input_channels=ch, batch_size=4)
        args.update(kw)
        with pytest.raises(ValueError):
            GpuValSet(**args)
    # GpuGridTiles keeps refusing what GpuValSet now serves
    with pytest.raises(ValueError):
        GpuGridTiles([s0, s0], "val", base[0]["area_defn"], ch, base[0]["image_pairs"])
    with pytest.raises(ValueError):
        GpuGridTiles(s0, "val", base[0]["area_defn"], ch, base[0]["image_pairs"], shard=(0, 2))
