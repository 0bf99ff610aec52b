"""The memory contract of include/resdepth_hip.h for the entry points of include/resdepth_hip_pairs.h: the guard-band cases that
tests/test_memory_contract_gpu.py runs for every entry point of the main header (its driver and judgement are used as they
are), plus the ledger over the side header: an entry point cannot arrive there without a case here.

This module leans on that file's helpers (_case, _full, _ops and the Case methods inp / pos / out / inout / call / wrapper /
ref / first), as tests/test_tta_contract_gpu.py does: a change to them is a change to these cases too.
test_the_borrowed_helpers_are_there names what is used.  Once the two entry points move into resdepth_hip.h and
_lib.SIGNATURES (see resdepth_hip_pairs.h), the case builders below move into that file's table and this module goes away."""
import os
import re

import pytest
import torch

import test_memory_contract_gpu as T
from test_memory_contract_gpu import F64, I32

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_borrowed_helpers_are_there():
    for name in ("_case", "_full", "_ops", "F64", "I32"):
        assert hasattr(T, name), name


def c_blend_planes(k, n, tile, stride, rows, cols, log2_variants, n_planes):
    """tiles in every orientation on n_planes rasters with odd sides, some reaching past the right / lower border (skipped
    pixels), planes round-robin with every 11th sample on a plane that does not exist (skipped samples); the planes are
    exactly rows x cols doubles apart, so a pixel past a raster's last row would land in the next plane or the guard band"""
    ops = T._ops()
    pred, mean, std = k.inp("pred", (n, 1, tile, tile)), k.inp("mean", n), k.pos("std", n)
    per_row = (cols - tile) // stride + 2                     # the last one of a row sticks out of the raster
    pos_l = [[(i // per_row) * stride, (i % per_row) * stride] for i in range(n)]
    pos = k.inp("pos", (n, 2), fn=lambda: torch.tensor(pos_l), dtype=I32)
    reg = k.inp("reg", (n, 4), fn=lambda: torch.tensor([[0, 0, rows - 1, cols - 1]] * n), dtype=I32)
    aug = k.inp("aug", n, fn=lambda: torch.arange(n) % 16, dtype=I32)
    plane_l = [(n_planes if i % 22 == 10 else -1) if i % 11 == 10 else i % n_planes for i in range(n)]
    plane = k.inp("plane", n, fn=lambda: torch.tensor(plane_l), dtype=I32)
    raster = k.inout("raster", (n_planes, rows, cols), dtype=F64)
    k.call("rd_blend_accumulate_planes", pred, mean, std, pos, reg, aug, plane, n, tile, stride, log2_variants, raster, n_planes,
           rows * cols, rows, cols)
    k.wrapper(lambda: {"raster": ops.blend_accumulate(pred, mean, std, pos, reg, tile, stride, k.first("raster"), aug=aug,
                                                      log2_variants=log2_variants, plane=plane, n_planes=n_planes)})


def c_fuse_planes(k, n, n_planes, pad, fuse_mode, spread_mode):
    """n pixels (odd: the scalar tail is the last element of the outputs' allocations; 1 200 001: past one pass of the grid) in
    planes n + pad doubles apart; the last plane ends where its allocation ends"""
    ops = T._ops()
    stride = n + pad
    planes = k.inp("planes", (n_planes - 1) * stride + n, dtype=F64, scale=3.0)
    fused = k.out("fused", n, dtype=F64)
    spread = k.out("spread", n, dtype=F64) if spread_mode else None
    k.call("rd_fuse_planes", planes, stride, n_planes, n, fuse_mode, fused, spread_mode, spread)

    def wrap():
        view = torch.as_strided(planes, (n_planes, n), (stride, 1))
        f, s = ops.fuse_planes(view, ["mean", "median"][fuse_mode], [None, "range", "std"][spread_mode])
        return {"fused": f, "spread": s} if spread_mode else {"fused": f}
    k.wrapper(wrap)


CASES = []
for s_ in [(3, 16, 8, 33, 41, 1, 2), (70, 8, 4, 45, 37, 3, 3), (5, 40, 24, 61, 93, 0, 1), (130, 8, 4, 45, 37, 2, 16)]:
    CASES.append(T._case(c_blend_planes, s_, ["rd_blend_accumulate_planes"], short=False))
for s_ in [(1961, 4, 0, 1, 2), (1961, 3, 1, 1, 1), (1961, 16, 7, 0, 2), (1, 2, 0, 1, 2), (1960, 5, 2, 1, 0), (777, 1, 0, 1, 1),
           (1200001, 2, 0, 1, 2)]:
    CASES.append(T._case(c_fuse_planes, s_, ["rd_fuse_planes"], short=False))


@pytest.fixture()
def lib():
    from resdepth_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("case", [pytest.param(c, id=c["id"]) for c in CASES])
def test_memory_contract(lib, case):
    T._full(lib, case)


def test_every_function_of_the_side_header_has_a_case():
    from resdepth_amd import _lib
    text = open(os.path.join(ROOT, "include", "resdepth_hip_pairs.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    exported = set(re.findall(r"\b(rd_\w+)\s*\(", text))
    assert exported == set(_lib.SIGNATURES_PAIRS)
    covered = {f for c in CASES for f in c["covers"]}
    assert covered == exported, covered ^ exported
