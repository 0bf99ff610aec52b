"""Test-time augmentation, host side (resdepth_amd/tiling.py): the variant sets, the numpy restatement of the orientation
codes against torch.rot90 / flip, the expanded sample lists of a sharded sweep, and the rounding identity that makes the
1 / variants weight exact."""
import os
import re

import numpy as np
import pytest
import torch

from resdepth_amd import tiling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_variant_sets():
    assert tiling.tta_codes(None) == (0,)
    assert tiling.tta_codes("none") == (0,)
    assert tiling.tta_codes("flips") == (0, 4, 8, 12)
    assert tiling.tta_codes("d4") == (0, 8, 1, 9, 2, 10, 3, 11)
    assert tiling.tta_codes("d4") == tuple(k | (h << 3) for k in range(4) for h in (0, 1))
    assert tiling.tta_codes([3, 15]) == (3, 15)
    assert tiling.tta_codes(np.array([0, 5, 10, 15])) == (0, 5, 10, 15)
    assert tiling.tta_codes(range(16)) == tuple(range(16))
    assert tiling.tta_codes("d4", swap_views=True) == tiling.tta_codes("d4")          # 16 variants: still a power of two


def test_the_eight_d4_codes_are_the_whole_group_once():
    x = np.arange(16.0).reshape(4, 4)
    seen = {tiling.tta_apply(x, c).tobytes() for c in tiling.tta_codes("d4")}
    assert len(seen) == 8
    assert seen == {tiling.tta_apply(x, c).tobytes() for c in range(16)}              # the 16 codes name each element twice


def test_the_view_swap_counts_as_variants_but_adds_no_codes():
    assert tiling.tta_codes("flips", True) == tiling.tta_codes("flips")               # 8 variants from 4 codes


@pytest.mark.parametrize("spec,swap", [([0, 1, 2], False), ([], False), (range(16), True), ([0] * 5, False),
                                       ([0, 1, 2, 3, 4, 5], True)])
def test_variant_counts_that_are_no_power_of_two_are_refused(spec, swap):
    with pytest.raises(ValueError, match="1, 2, 4, 8 or 16"):
        tiling.tta_codes(spec, swap)


@pytest.mark.parametrize("spec", ["D4", "rot", [16], [-1], [0.5], [True], 7])
def test_bad_variant_specs_are_refused(spec):
    with pytest.raises(ValueError):
        tiling.tta_codes(spec)


def _torch_apply(x, code):
    y = torch.rot90(x, code & 3, (-2, -1))
    if code & 4:
        y = torch.flip(y, (-2,))
    if code & 8:
        y = torch.flip(y, (-1,))
    return y


def _torch_undo(y, code):
    if code & 8:
        y = torch.flip(y, (-1,))
    if code & 4:
        y = torch.flip(y, (-2,))
    return torch.rot90(y, -(code & 3), (-2, -1))


@pytest.mark.parametrize("code", range(16))
def test_numpy_restatement_is_torch_rot90_flipud_fliplr(code):
    rng = np.random.default_rng(code)
    x = rng.standard_normal((2, 3, 8, 8)).astype(np.float32)
    x[0, 0, 1, 2] = np.nan
    fwd, inv = tiling.tta_apply(x, code), tiling.tta_undo(x, code)
    assert fwd.flags["C_CONTIGUOUS"] and inv.flags["C_CONTIGUOUS"]
    assert np.array_equal(fwd, _torch_apply(torch.from_numpy(x), code).numpy(), equal_nan=True)
    assert np.array_equal(inv, _torch_undo(torch.from_numpy(x), code).numpy(), equal_nan=True)
    assert np.array_equal(tiling.tta_undo(fwd, code), x, equal_nan=True)
    assert np.array_equal(tiling.tta_apply(inv, code), x, equal_nan=True)
    # the index form the kernels use (csrc/rd_tile_dev.h: aug_src): oriented (r, c) shows plain (sr, sc)
    T, k = 8, code & 3
    for r, c in [(0, 0), (1, 5), (7, 2)]:
        c1, r1 = (T - 1 - c if code & 8 else c), (T - 1 - r if code & 4 else r)
        sr, sc = [(r1, c1), (c1, T - 1 - r1), (T - 1 - r1, T - 1 - c1), (T - 1 - c1, r1)][k]
        assert fwd[1, 2, r, c] == x[1, 2, sr, sc]


def test_expanded_lists_keep_a_tiles_variants_together_on_its_rank():
    T, stride, rows, cols = 32, 16, 88, 120
    _, pos, reg, pair = tiling.grid_samples([(0, cols - 1)], [(0, rows - 1)], T, "test", stride)
    assert len(pos) == 35
    codes = tiling.tta_codes("d4")
    whole = tiling.tta_expand(pos, reg, pair, codes)
    assert len(whole[0]) == 280 and whole[5] == codes
    assert whole[0] == [p for p in pos for _ in codes] and whole[1] == [r for r in reg for _ in codes]
    assert whole[3] == list(codes) * 35 and whole[4] == [0] * 280
    for world in (1, 2, 3):
        got_pos, got_reg, got_code = [], [], []
        for rank in range(world):
            p, r, pi, plan = tiling.grid_shard("test", pos, reg, pair, T, rows, (rank, world))
            ep, er, epi, code, swap, variants = tiling.tta_expand(p, r, pi, codes)
            assert len(ep) == 8 * len(p) and variants == codes
            for k in range(len(p)):                # tile-major, variant-minor: 8 consecutive samples are ONE tile
                assert ep[8 * k:8 * k + 8] == [p[k]] * 8 and er[8 * k:8 * k + 8] == [r[k]] * 8
                assert tuple(code[8 * k:8 * k + 8]) == codes
            # the band plan is the plain sweep's: the rank's expanded samples stay inside its band's rows
            me = plan[rank]
            assert all(me["y0"] <= y < me["y1"] for y, _ in ep)
            got_pos += ep
            got_reg += er
            got_code += code
        assert (got_pos, got_reg, got_code) == (whole[0], whole[1], whole[3])


def test_view_swap_doubles_the_variants():
    pos, reg, pair = [(0, 0), (0, 16)], [(0, 0, 15, 15), (0, 16, 15, 31)], [0, 0]
    ep, er, epi, code, swap, variants = tiling.tta_expand(pos, reg, pair, (0, 8), swap_views=True)
    assert variants == (0, 8, 0, 8)
    assert code == [0, 8, 0, 8] * 2 and swap == [0, 0, 1, 1] * 2
    assert ep == [(0, 0)] * 4 + [(0, 16)] * 4 and epi == [0] * 8


def test_a_power_of_two_weight_commutes_with_the_rounding():
    """fl(fl(a w) 2^-k) == fl(a w) 2^-k, and the same through an fp64 accumulation: what makes the sum over a tile's variants
    times 1 / variants equal to the sum of the weighted variants, bit for bit."""
    rng = np.random.default_rng(3)
    a = (rng.standard_normal(4096) * 3.0 + 400.0).astype(np.float32).astype(np.float64)
    w = rng.random(4096) * rng.random(4096)
    for k in range(5):
        s = 2.0 ** -k
        assert np.array_equal((a * w) * s, (a * s) * w)
        assert np.array_equal((a * w) * s, a * (w * s))
        acc, acc_s = 0.0, 0.0
        for ai, wi in zip(a[:512], w[:512]):
            acc = acc + ai * wi
            acc_s = acc_s + (ai * wi) * s
        assert acc_s == acc * s


def test_tta_header_and_bindings_agree():
    """include/resdepth_hip_tta.h declares what _lib.SIGNATURES_TTA binds, and the library exports it."""
    from resdepth_amd import _lib
    text = open(os.path.join(ROOT, "include", "resdepth_hip_tta.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    declared = set(re.findall(r"\b(rd_\w+)\s*\(", text))
    assert declared == set(_lib.SIGNATURES_TTA) == {"rd_blend_accumulate_tta", "rd_assemble_grid_tiles_aug"}
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name)
    assert lib.rd_version() >= 111
    main = open(os.path.join(ROOT, "include", "resdepth_hip.h")).read()
    assert '#include "resdepth_hip_tta.h"' in main
