"""The multi-dataset, rank-sharded validation set (GpuValSet), host side: the per-rank batch plan
(tiling.val_shard_batches) and the concatenated sample list (tiling.concat_val_samples) against the reference's own
ConcatDataset of 'val' DsmOrthoDatasets (tests/golden/g21_valset.npz)."""
import json

import numpy as np
import pytest

from conftest import load_npz
from resdepth_amd import tiling


@pytest.mark.parametrize("world", [1, 2, 3, 4])
@pytest.mark.parametrize("b", [1, 2, 3, 4, 5, 6, 7])
def test_val_shard_batches(b, world):
    saw = set()
    for n in list(range(0, 31)) + [48, 61, 97]:
        big = b * world
        n_batches = -(-n // big)
        ranks = [tiling.val_shard_batches(n, b, (r, world)) for r in range(world)]
        assert all(len(x) == n_batches for x in ranks), (n, b, world)
        if world == 1:
            assert ranks[0] == tiling.batch_bounds(n, b)
        for k in range(n_batches):
            g0, g1 = k * big, min((k + 1) * big, n)
            runs = [x[k] for x in ranks]
            sizes = {k1 - k0 for k0, k1 in runs}
            assert len(sizes) == 1 and min(sizes) >= 1, (n, b, world, k, runs)      # equal per-rank sizes, nobody idles
            seen = np.concatenate([np.arange(k0, k1) for k0, k1 in runs])
            if (g1 - g0) % world == 0:
                # split: contiguous runs in rank order, every sample of the global batch exactly once
                np.testing.assert_array_equal(seen, np.arange(g0, g1))
                if g1 - g0 == big:
                    assert runs == [(g0 + r * b, g0 + (r + 1) * b) for r in range(world)]
                saw.add("split")
            else:
                assert k == n_batches - 1 and runs == [(g0, g1)] * world           # replicated: the whole tail on every rank
                np.testing.assert_array_equal(seen, np.tile(np.arange(g0, g1), world))
                saw.add("replicated")
    assert saw == ({"split"} if world == 1 else {"split", "replicated"})


def test_val_shard_batches_refuses_bad_arguments():
    for shard in ((2, 2), (-1, 2), (0, 0)):
        with pytest.raises(ValueError):
            tiling.val_shard_batches(10, 2, shard)
    with pytest.raises(ValueError):
        tiling.val_shard_batches(10, 0, (0, 1))


def test_concatenated_list_is_the_references_concat_dataset():
    g = load_npz("g21_valset.npz")
    t = int(g["tile"])
    sets = [json.loads(str(g[f"d{d}/settings"])) for d in range(int(g["n_datasets"]))]
    areas = [(c["area"]["x_extent"], c["area"]["y_extent"], len(c["pairs"])) for c in sets]
    stride, ids, pos, reg, pair_idx = tiling.concat_val_samples(areas, t)
    assert stride == t
    np.testing.assert_array_equal(np.array(ids), g["dataset_id"])
    np.testing.assert_array_equal(np.array(pos).reshape(-1, 2), g["pos"])
    np.testing.assert_array_equal(np.array(reg).reshape(-1, 4), g["reg"])
    np.testing.assert_array_equal(np.array(pair_idx), g["pair_idx"])
    np.testing.assert_array_equal(g["meta"], np.concatenate([g["pos"], g["reg"]], 1))
    # the fixture shows something only if a batch of 5 straddles the two datasets
    n0 = int((g["dataset_id"] == 0).sum())
    assert n0 % 5 != 0 and 0 < n0 < len(ids)
    assert g["batch_sizes"].tolist() == [k1 - k0 for k0, k1 in tiling.batch_bounds(len(ids), 5)]
    # every dataset's part is its own grid_samples list, pair indices counted within the dataset
    first = 0
    for d, (xe, ye, n_pairs) in enumerate(areas):
        _, p, r, q = tiling.grid_samples(xe, ye, t, "val", None, n_pairs, True)
        assert pos[first:first + len(p)] == p and reg[first:first + len(p)] == r and pair_idx[first:first + len(p)] == q
        assert max(q) == n_pairs - 1
        first += len(p)
    assert first == len(ids)
    # without views ('geom') every position is taken once
    _, ids_g, pos_g, _, pair_g = tiling.concat_val_samples(areas, t, views=False)
    assert len(ids_g) == sum(len(tiling.regular_grid(xe, ye, t, t)[0]) for xe, ye, _ in areas) and set(pair_g) == {0}
