"""Validation / inference grid tiles (GpuGridTiles), host side: the sample planner (tiling.grid_samples / grid_shard /
batch_bounds) and the numpy stand-in against samples produced by the reference's own DsmOrthoDataset._determine_patches and
__getitem__ (tests/golden/g19_grid.npz)."""
import json

import numpy as np
import pytest
from torch.utils.data import BatchSampler, SequentialSampler

import grid_tiles_ref as R
from conftest import load_npz
from oracle import sample_oracle as S
from resdepth_amd import tiling


@pytest.fixture(scope="module")
def g19():
    g = load_npz("g19_grid.npz")
    g["orthos"] = g["orthos_u8"].astype(np.float32)
    return g


def _cases(g):
    return [(str(n), json.loads(str(g[f"{n}/settings"]))) for n in g["cases"]]


def _plan(c, t):
    a = c["area"]
    n_pairs = len(c["pairs"]) if c["pairs"] else 1
    return tiling.grid_samples(a["x_extent"], a["y_extent"], t, c["strategy"], None, n_pairs, c["channels"] != "geom")


def test_planner_reproduces_reference_sample_order(g19):
    t = int(g19["tile"])
    assert len(_cases(g19)) == 7
    for name, c in _cases(g19):
        stride, pos, reg, pair_idx = _plan(c, t)
        assert stride == int(g19[f"{name}/stride"]), name
        np.testing.assert_array_equal(np.array(pos).reshape(-1, 2), g19[f"{name}/pos"], err_msg=name)
        np.testing.assert_array_equal(np.array(reg).reshape(-1, 4), g19[f"{name}/reg"], err_msg=name)
        np.testing.assert_array_equal(np.array(pair_idx), g19[f"{name}/pair_idx"], err_msg=name)
        np.testing.assert_array_equal(g19[f"{name}/meta"], np.concatenate([g19[f"{name}/pos"], g19[f"{name}/reg"]], 1))
        p, r, q, plan = tiling.grid_shard(c["strategy"], pos, reg, pair_idx, t, g19["dsm_in"].shape[0])
        assert (p, r, q) == (list(pos), list(reg), list(pair_idx))
        assert (plan is None) == (c["strategy"] == "val")
    # val with views is pair-major: sample k = (position k % P, pair k // P)
    stride, pos, reg, pair_idx = _plan(dict(_cases(g19))["val_stereo"], t)
    npos = len(pos) // 3
    assert all(pos[k] == pos[k % npos] and pair_idx[k] == k // npos for k in range(len(pos)))


@pytest.mark.parametrize("n,bs", [(24, 5), (24, 8), (14, 32), (1, 3), (0, 4)])
def test_batch_bounds_match_the_dataloader(n, bs):
    want = [(b[0], b[-1] + 1) for b in BatchSampler(SequentialSampler(range(n)), bs, drop_last=False)]
    assert tiling.batch_bounds(n, bs) == want


def test_shard_plan_matches_synthetic_raster_tiles():
    from resdepth_amd import SyntheticRasterTiles
    rows, cols, t = 200, 168, 32
    areas = [((0, 167), (0, 95)), ((8, 150), (100, 199))]
    xe, ye = [a[0] for a in areas], [a[1] for a in areas]
    stride, pos, reg, pair_idx = tiling.grid_samples(xe, ye, t, "test")
    assert stride == 16
    for world in (1, 2, 3, 5):
        for rank in range(world):
            syn = SyntheticRasterTiles(rows, cols, 1, tile_size=t, shard=(rank, world), areas=areas)
            p, r, q, plan = tiling.grid_shard("test", pos, reg, pair_idx, t, rows, (rank, world))
            assert p == syn.pos and r == syn.reg and plan == syn.shard_plan
            assert q == [0] * len(p)


def test_sharded_validation_and_bad_strategy_are_refused():
    with pytest.raises(ValueError):
        tiling.grid_shard("val", [(0, 0)], [(0, 0, 15, 15)], [0], 16, 16, (0, 2))
    with pytest.raises(ValueError):
        tiling.grid_samples([(0, 31)], [(0, 31)], 16, "train")


def test_stand_in_reproduces_reference_samples(g19):
    t = int(g19["tile"])
    for name, c in _cases(g19):
        gt = g19["dsm_gt"] if c["gt"] else None
        for k, (pos, box, pi) in enumerate(zip(g19[f"{name}/pos"], g19[f"{name}/reg"], g19[f"{name}/pair_idx"])):
            pair = c["pairs"][pi] if c["pairs"] else []
            s = R.grid_sample(g19["dsm_in"], gt, g19["orthos"], tuple(pos), tuple(box), pair, t, g19["nodata"],
                              g19["dsm_std"], c["ortho_mean"], g19["ortho_std"], c["channels"], c["dsm_mean"],
                              c.get("transform_dsm", True), c.get("transform_orthos", True))
            # quarter-metre heights and integer radiances: every float32 sum of a tile is exact, so are the means
            np.testing.assert_array_equal(s["input"], g19[f"{name}/input"][k], err_msg=f"{name} {k}")
            assert s["dsm_mean"] == g19[f"{name}/dsm_mean"][k], (name, k)
            if c["gt"]:
                np.testing.assert_array_equal(s["target"], g19[f"{name}/target"][k], err_msg=f"{name} {k}")
                np.testing.assert_array_equal(s["loss_mask"], g19[f"{name}/loss_mask"][k], err_msg=f"{name} {k}")
            else:
                assert f"{name}/target" not in g19
        if c["gt"]:
            assert g19[f"{name}/loss_mask"].any() and not g19[f"{name}/loss_mask"].all()
    np.testing.assert_array_equal(g19["test_zero_mean/dsm_mean"], g19["test_stereo/dsm_mean"])     # 0.0: per-tile means


def test_sample_oracle_plus_box_mask_reproduces_reference_samples(g19):
    """The training-sample oracle without augmentation, with the mask cut to the box, is the val / test sample too."""
    t = int(g19["tile"])
    for name in ("val_stereo", "test_stereo"):
        c = dict(_cases(g19))[name]
        for k, (pos, box, pi) in enumerate(zip(g19[f"{name}/pos"], g19[f"{name}/reg"], g19[f"{name}/pair_idx"])):
            s = S.assemble(g19["dsm_in"], g19["dsm_gt"], g19["orthos"], tuple(pos), list(c["pairs"][pi]), t, g19["nodata"],
                           g19["dsm_std"], c["ortho_mean"], g19["ortho_std"], aug=None)
            inside = np.zeros((1, t, t), dtype=bool)
            inside[:, box[0]:box[2] + 1, box[1]:box[3] + 1] = True
            np.testing.assert_array_equal(s["loss_mask"] & inside, g19[f"{name}/loss_mask"][k])
            np.testing.assert_array_equal(s["input"], g19[f"{name}/input"][k])
            np.testing.assert_array_equal(s["target"], g19[f"{name}/target"][k])
