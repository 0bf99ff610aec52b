"""All image pairs in one sweep, host side: the expanded sample list (tiling.pair_expand, alone and under tta_expand) and the
side header include/resdepth_hip_pairs.h against its bindings and the library's exports."""
import os
import re

import pytest

from resdepth_amd import tiling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grid():
    T, stride, rows, cols = 32, 16, 88, 120
    _, pos, reg, pair = tiling.grid_samples([(0, cols - 1)], [(0, rows - 1)], T, "test", stride)
    assert len(pos) == 35 and pair == [0] * 35
    return pos, reg


@pytest.mark.parametrize("n_pairs", [1, 3, 4, 16])
def test_pair_expand_is_tile_major_and_pair_minor(n_pairs):
    pos, reg = _grid()
    ep, er, epi = tiling.pair_expand(pos, reg, n_pairs)
    want = [(p, r, k) for p, r in zip(pos, reg) for k in range(n_pairs)]
    assert list(zip(ep, er, epi)) == want
    assert len(ep) == 35 * n_pairs


def test_pair_expand_under_tta_is_tile_then_pair_then_variant():
    pos, reg = _grid()
    codes = tiling.tta_codes("flips")
    ep, er, epi, code, swap, variants = tiling.tta_expand(*tiling.pair_expand(pos, reg, 3), codes, swap_views=True)
    want = [(p, r, k, c, s) for p, r in zip(pos, reg) for k in range(3) for s in (0, 1) for c in codes]
    assert list(zip(ep, er, epi, code, swap)) == want
    assert variants == codes * 2


def test_pair_expand_after_grid_shard_keeps_a_tiles_pairs_on_its_rank():
    pos, reg = _grid()
    whole = tiling.pair_expand(pos, reg, 3)
    got = [[], [], []]
    for rank in range(2):
        p, r, _, plan = tiling.grid_shard("test", pos, reg, [0] * len(pos), 32, 88, (rank, 2))
        part = tiling.pair_expand(p, r, 3)
        assert all(plan[rank]["y0"] <= y < plan[rank]["y1"] for y, _ in part[0])
        for k in range(3):
            got[k] += part[k]
    assert tuple(got) == tuple(whole)


@pytest.mark.parametrize("bad", [0, -2])
def test_pair_expand_refuses_an_empty_pair_list(bad):
    with pytest.raises(ValueError, match="n_pairs"):
        tiling.pair_expand([(0, 0)], [(0, 0, 31, 31)], bad)


def test_pairs_header_and_bindings_agree():
    """include/resdepth_hip_pairs.h declares what _lib.SIGNATURES_PAIRS binds, and the library exports it."""
    from resdepth_amd import _lib
    text = open(os.path.join(ROOT, "include", "resdepth_hip_pairs.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    declared = set(re.findall(r"\b(rd_\w+)\s*\(", text))
    assert declared == set(_lib.SIGNATURES_PAIRS) == {"rd_blend_accumulate_planes", "rd_fuse_planes"}
    # one ctypes argument per declared parameter
    for name, (_, args) in _lib.SIGNATURES_PAIRS.items():
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, text, flags=re.S).group(1)
        assert len(args) == len(params.split(",")), name
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name)
    assert lib.rd_version() >= 112
    main = open(os.path.join(ROOT, "include", "resdepth_hip.h")).read()
    assert '#include "resdepth_hip_pairs.h"' in main
    # the mode numbers the Python surface passes are the header's
    from resdepth_amd import ops
    defs = dict(re.findall(r"#define (RD_(?:FUSE|SPREAD)_\w+) (\d+)", text))
    assert {k: int(v) for k, v in defs.items()} == {
        "RD_FUSE_MEAN": ops.FUSE_MODES["mean"], "RD_FUSE_MEDIAN": ops.FUSE_MODES["median"], "RD_SPREAD_NONE": ops.SPREAD_MODES[None],
        "RD_SPREAD_RANGE": ops.SPREAD_MODES["range"], "RD_SPREAD_STD": ops.SPREAD_MODES["std"]}
