"""Host side of the training set (no GPU): the numpy stand-in (tests/train_set_ref.py) against the reference's own samples and
statistics (g20 fixture), and the index logic of resdepth_amd.tiling -- train_position / train_position_count against a
brute-force enumeration, draw_train_samples against the reference's sample lists, epoch_order's shards, the percentile rule."""
import json

import numpy as np
import pytest
import torch

import train_set_ref as R
from conftest import load_npz

REL = 1e-12          # the statistics' bar: two orders above the rounding bound of an fp64 centred sum over 256 terms


@pytest.fixture(scope="module")
def g():
    return load_npz("g20_train.npz")


def _cases(g):
    for name in g["cases"]:
        yield str(name), json.loads(str(g[f"{name}/settings"]))


def _raster(g, name):
    return g[f"{name}/dsm_in"], g[f"{name}/dsm_gt"], g[f"{name}/orthos_u8"].astype(np.float32)


def test_stand_in_reproduces_every_reference_sample(g):
    t = int(g["tile"])
    for name, c in _cases(g):
        ids, pos, pidx = g[f"{name}/dataset_id"], g[f"{name}/pos"], g[f"{name}/pair_idx"]
        for i in range(len(pos)):
            d = c["datasets"][ids[i]]
            dsm, gt, orthos = _raster(g, d["raster"])
            views = d["pairs"][pidx[i]] if d["pairs"] else None
            s = R.train_sample(dsm, gt, orthos, pos[i], views, t, g["nodata"], g[f"{d['raster']}/dsm_std"], c["ortho_mean"],
                               g[f"{d['raster']}/ortho_std"], c["channels"], dsm_mean=c["dsm_mean"],
                               transform_dsm=c.get("transform_dsm", True), transform_orthos=c.get("transform_orthos", True))
            np.testing.assert_allclose(s["input"], g[f"{name}/input"][i], rtol=0, atol=3e-5, err_msg=f"{name} {i}")
            np.testing.assert_allclose(s["target"], g[f"{name}/target"][i], rtol=0, atol=3e-5, err_msg=f"{name} {i}")
            np.testing.assert_array_equal(s["loss_mask"], g[f"{name}/loss_mask"][i])
            want = g[f"{name}/dsm_mean"][i]
            assert abs(s["dsm_mean"] - want) <= 1e-6 * abs(want), (name, i)
            assert tuple(g[f"{name}/offsets"][i]) == tuple(pos[i])


def test_stand_in_statistics_match_the_float128_reference_and_a_naive_sum_of_squares_does_not(g):
    t = int(g["tile"])
    flat_naive = []
    for name in ("std21", "std30"):
        ids, pos = g[f"{name}/dataset_id"], g[f"{name}/pos"]
        for ident, key in (("raster_in", "dsm_in"), ("raster_gt", "dsm_gt")):
            groups = [(g[f"{rn}/{key}"], pos[ids == k]) for k, rn in enumerate(("flat", "city"))]
            value, stds = R.local_dsm_std(groups, t, g["nodata"])
            want = g[f"{name}/{ident}/stds"]
            print(name, ident, "stand-in max rel err", np.abs(stds / want - 1).max())
            assert np.all(np.abs(stds - want) <= REL * want), (name, ident)
            assert abs(value - float(g[f"{name}/{ident}/std"])) <= REL * value
            naive = R.patch_stds_naive(groups[0][0], groups[0][1], t, g["nodata"])          # the flat, high raster
            flat_naive.append(np.abs(naive / want[ids == 0] - 1).max())
    print("naive sum of squares, flat raster: max rel err", flat_naive)
    assert min(flat_naive) > 100 * REL            # the bar does separate the formulations
    norm = json.loads(str(g["norm/settings"]))
    mean, std = R.image_normalization([(g[f"{d['raster']}/orthos_u8"].astype(np.float32), d["pairs"], d["area"]) for d in norm])
    assert abs(mean - float(g["norm/mean"])) <= 1e-6 * mean and abs(std - float(g["norm/std"])) <= 1e-6 * std


def test_percentile_rule_on_both_sample_counts(g):
    from resdepth_amd import normalization as N
    for name, n in (("std21", 21), ("std30", 30)):
        for ident in ("raster_in", "raster_gt"):
            stds = g[f"{name}/{ident}/stds"]
            assert len(stds) == n
            want = float(g[f"{name}/{ident}/std"])
            assert abs(N.trimmed_mean(stds) - want) <= 1e-15 * want
            srt = np.sort(stds)
            lo, hi = (n - 1) * 0.05, (n - 1) * 0.95
            if name == "std21":                  # the percentiles fall on samples 1 and 19: both are kept
                assert np.isclose(lo, 1.0) and np.isclose(hi, 19.0)
                assert abs(srt[1:20].mean() - want) <= 1e-14 * want
            else:                                # interpolated: the samples strictly outside [p5, p95] go
                keep = srt[int(np.ceil(lo)):int(np.floor(hi)) + 1]
                assert abs(keep.mean() - want) <= 1e-14 * want and len(keep) == 26


def test_train_position_enumerates_the_reference_list():
    from resdepth_amd import tiling
    areas = [{"x_extent": [(0, 31), (70, 105)], "y_extent": [(0, 15), (40, 71)]}, {"x_extent": [(3, 40)], "y_extent": [(5, 20)]},
             {"x_extent": [(0, 15), (0, 15), (7, 30)], "y_extent": [(0, 15), (2, 40), (9, 24)]}]
    for area in areas:
        for t in (8, 16):
            want = R.position_list(area, t)
            assert tiling.train_position_count(area, t) == len(want)
            got = tiling.train_position(area, t, np.arange(len(want)))
            np.testing.assert_array_equal(got, np.array(want))
            assert tiling.train_position(area, t, len(want) - 1) == want[-1] and tiling.train_position(area, t, 0) == want[0]
            with pytest.raises(IndexError):
                tiling.train_position(area, t, len(want))
    with pytest.raises(ValueError):
        tiling.train_position_count({"x_extent": [(0, 14)], "y_extent": [(0, 40)]}, 16)
    big = {"x_extent": [(0, 8191)], "y_extent": [(0, 8191)]}
    assert tiling.train_position_count(big, 256) == 7937 ** 2             # arithmetic: the list is never built
    assert tiling.train_position(big, 256, 7937 ** 2 - 1) == (7936, 7936)


def test_draw_train_samples_reproduces_the_reference_lists(g):
    from resdepth_amd import tiling
    t = int(g["tile"])
    for name, c in _cases(g):
        np.random.seed(c["seed"])
        pos, pidx = [], []
        for d in c["datasets"]:                                   # one seed, the datasets draw one after the other
            p, i = tiling.draw_train_samples(d["area"], t, d["n_samples"], c["channels"], d["pairs"], c["use_all"])
            pos.append(p)
            pidx.append(i)
        np.testing.assert_array_equal(np.concatenate(pos), g[f"{name}/pos"], err_msg=name)
        np.testing.assert_array_equal(np.concatenate(pidx), g[f"{name}/pair_idx"], err_msg=name)
        np.random.seed(c["seed"])                                 # and the brute-force stand-in
        ref = [R.sample_list(d["area"], t, d["n_samples"], c["channels"], d["pairs"], c["use_all"]) for d in c["datasets"]]
        np.testing.assert_array_equal(np.concatenate([r[0] for r in ref]), g[f"{name}/pos"], err_msg=name)
        np.testing.assert_array_equal(np.concatenate([r[1] for r in ref]), g[f"{name}/pair_idx"], err_msg=name)
    assert g["stereo_all/pair_idx"].tolist() == [0, 1, 2] * 3 and len(set(g["stereo_rand/pair_idx"].tolist())) > 1
    assert not g["mono/pair_idx"].any() and not g["views_only/pair_idx"].any()       # several pairs listed, pair 0 used
    rs = np.random.RandomState(5)
    a = tiling.draw_train_samples(json.loads(str(g["geom/settings"]))["datasets"][0]["area"], t, 7, "geom", None, False, rng=rs)
    assert a[0].shape == (7, 2) and len({tuple(p) for p in a[0]}) == 7
    with pytest.raises(ValueError):
        tiling.draw_train_samples({"x_extent": [(0, 16)], "y_extent": [(0, 16)]}, 16, 5, "geom")      # four positions only


def test_epoch_order_shards_are_disjoint_equal_and_cover_the_cut_permutation():
    from resdepth_amd import tiling
    n = 103
    whole = tiling.epoch_order(n, torch.Generator().manual_seed(9))
    assert torch.equal(whole, torch.randperm(n, generator=torch.Generator().manual_seed(9)))
    for world in (2, 3, 8):
        parts = [tiling.epoch_order(n, torch.Generator().manual_seed(9), shard=(r, world)) for r in range(world)]
        assert all(len(p) == n // world for p in parts)
        cut = whole[:(n // world) * world]
        inter = torch.stack(parts, 1).reshape(-1)
        assert torch.equal(inter, cut)
        assert len(set(inter.tolist())) == len(inter)
    assert torch.equal(tiling.epoch_order(7, None, shuffle=False), torch.arange(7))
    assert torch.equal(tiling.epoch_order(7, None, shard=(1, 2), shuffle=False), torch.tensor([1, 3, 5]))
    g1 = torch.Generator().manual_seed(1)
    assert not torch.equal(tiling.epoch_order(50, g1), tiling.epoch_order(50, g1))      # the generator advances per epoch
    with pytest.raises(ValueError):
        tiling.epoch_order(5, None, shard=(2, 2))
