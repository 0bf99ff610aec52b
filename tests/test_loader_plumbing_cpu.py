"""The pure pieces every GPU-resident loader shares (resdepth_amd/sampler.py): the prefetch queue's discipline, the transform
mode, the augmentation code and its draws, the image-pair checks.  No device and no library load."""
import itertools
import types

import numpy as np
import pytest
import torch

from resdepth_amd import tiling
from resdepth_amd.sampler import _aug_code, _check_image_pairs, _draw_aug, _queued, _transform_mode


@pytest.mark.parametrize("depth", [-1, 0, 1, 3])
@pytest.mark.parametrize("n", [0, 1, 2, 7])
def test_queue_runs_depth_jobs_ahead_in_job_order(depth, n):
    ahead = max(0, depth)
    made = []
    produce = lambda job: made.append(job) or ("item", job)        # noqa: E731
    out = []
    for k, item in enumerate(_queued(range(n), produce, depth)):
        assert item == ("item", k)
        assert len(made) == min(n, k + ahead + 1)                   # k = 0: min(n, depth + 1) draws before the first yield
        out.append(item[1])
    assert out == made == list(range(n))
    # an iterator abandoned after its first item has produced no more than that
    made.clear()
    it = _queued(range(n), produce, depth)
    if n:
        next(it)
    it.close()
    assert made == list(range(min(n, ahead + 1)))


def test_transform_mode():
    for mean in (None, 0.0, 110.0):
        assert _transform_mode(False, mean) == (0, 0.0)
    assert _transform_mode(True, None) == (2, 0.0)
    assert _transform_mode(True, 0.0) == (2, 0.0)
    assert _transform_mode(True, 110.0) == (1, 110.0)
    assert all(type(_transform_mode(e, m)[1]) is float for e in (False, True) for m in (None, 0, np.float32(110.0)))


def test_aug_code_packs_k_and_flips():
    combos = list(itertools.product(range(4), (0, 1), (0, 1)))                      # (k, flip_v, flip_h)
    want = [k | fv << 2 | fh << 3 for k, fv, fh in combos]
    assert sorted(want) == list(range(16))
    for aug in (combos, np.array(combos, dtype=np.int64), torch.tensor(combos, dtype=torch.int64)):
        code = _aug_code(aug)
        assert code.dtype == (torch.int32 if torch.is_tensor(aug) else np.int32)
        assert code.tolist() == want
    assert _aug_code(np.array(combos).reshape(-1), 16).tolist() == want
    with pytest.raises((ValueError, RuntimeError)):
        _aug_code(combos, 15)                                                       # not the n samples of the batch
    # tiling's "d4" set: k = 0..3, each without and with fliplr
    d4 = [(k, 0, h) for k in range(4) for h in (0, 1)]
    assert tuple(_aug_code(d4).tolist()) == tiling.tta_codes("d4")


@pytest.mark.parametrize("n", [0, 1, 37])
def test_draw_aug_is_three_randint_calls_in_order(n):
    g, h = torch.Generator().manual_seed(1234), torch.Generator().manual_seed(1234)
    want = torch.stack([torch.randint(0, 4, (n,), generator=h), torch.randint(0, 2, (n,), generator=h),
                        torch.randint(0, 2, (n,), generator=h)], 1)
    got = _draw_aug(n, g)
    assert got.dtype == want.dtype and got.shape == (n, 3) and torch.equal(got, want)
    assert torch.equal(g.get_state(), h.get_state())


def test_check_image_pairs():
    s = types.SimpleNamespace(orthos=types.SimpleNamespace(shape=(5, 8, 8)))
    assert _check_image_pairs("GpuValSet", s, [(0, 4), np.array([3, 1])], " (dataset 2)") == [[0, 4], [3, 1]]
    for bad in ([[0, 1], [2]], [[], []]):                                           # ragged, empty
        with pytest.raises(ValueError, match="^GpuTrainSet: every image pair must have the same number of views$"):
            _check_image_pairs("GpuTrainSet", s, bad, " (dataset 0)")
    for bad in ([[0, 5]], [[-1, 0]]):
        with pytest.raises(ValueError, match=r"^GpuValSet: an image index is outside the 5 ortho planes \(dataset 2\)$"):
            _check_image_pairs("GpuValSet", s, bad, " (dataset 2)")
    with pytest.raises(ValueError, match="^GpuGridTiles: an image index is outside the 5 ortho planes$"):
        _check_image_pairs("GpuGridTiles", s, [[0, 5]])
