"""The memory contract of include/resdepth_hip.h for the entry points of include/resdepth_hip_tta.h: the guard-band cases that
tests/test_memory_contract_gpu.py runs for every entry point of the main header (its driver and judgement are used as they
are), plus the ledger over the side header: an entry point cannot arrive there without a case here.

This module leans on that file's helpers (_case, _full, _run_case, _ops, _with_nodata, _rand and the Case methods inp / pos /
inout / call / wrapper / first): a change to them is a change to these cases too.  test_the_borrowed_helpers_are_there names
what is used, so a rename there fails here by name and not somewhere inside a case.  Once the two entry points move into
resdepth_hip.h and _lib.SIGNATURES (see resdepth_hip_tta.h), the two case builders below move into that file's table and this
module goes away."""
import os
import re

import pytest
import torch

import test_memory_contract_gpu as T
from test_memory_contract_gpu import F64, I32

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_borrowed_helpers_are_there():
    for name in ("_case", "_full", "_run_case", "_ops", "_with_nodata", "_rand", "F64", "I32"):
        assert hasattr(T, name), name


def c_blend_tta(k, n, tile, stride, rows, cols, log2_variants):
    """tiles in every orientation on a raster with odd sides, some reaching past its right / lower border (skipped pixels)"""
    ops = T._ops()
    pred, mean, std = k.inp("pred", (n, 1, tile, tile)), k.inp("mean", n), k.pos("std", n)
    per_row = (cols - tile) // stride + 2                     # the last one of a row sticks out of the raster
    pos_l = [[(i // per_row) * stride, (i % per_row) * stride] for i in range(n)]
    pos = k.inp("pos", (n, 2), fn=lambda: torch.tensor(pos_l), dtype=I32)
    reg = k.inp("reg", (n, 4), fn=lambda: torch.tensor([[0, 0, rows - 1, cols - 1]] * n), dtype=I32)
    aug = k.inp("aug", n, fn=lambda: torch.arange(n) % 16, dtype=I32)
    raster = k.inout("raster", (rows, cols), dtype=F64)
    k.call("rd_blend_accumulate_tta", pred, mean, std, pos, reg, aug, n, tile, stride, log2_variants, raster, rows, cols)
    k.wrapper(lambda: {"raster": ops.blend_accumulate(pred, mean, std, pos, reg, tile, stride, k.first("raster"), aug=aug,
                                                      log2_variants=log2_variants)})


def c_grid_tiles_aug(k, n, tile, height, width, views, mode):
    lib = k.lib
    planes, n_pairs = views + 1, 2
    dsm_in = k.inp("dsm_in", (height, width), fn=lambda: T._with_nodata(height, width, 5))
    ortho = k.inp("ortho", (planes, height, width), fn=lambda: T._rand(3, planes, height, width) * 255)
    smp = [[(7 * i) % (height - tile + 1), (3 * i) % (width - tile + 1), 1, 1, tile - 2, tile - 2, i % n_pairs, 0] for i in range(n - 1)]
    smp.append([height - tile, width - tile, 0, 0, tile - 1, tile - 1, 1, 0])
    samples = k.inp("samples", (n, 8), fn=lambda: torch.tensor(smp), dtype=I32)
    pairs = k.inp("pair_planes", (n_pairs, views), fn=lambda: torch.tensor([[(p + j) % planes for j in range(views)] for p in range(n_pairs)]),
                  dtype=I32)
    aug = k.inp("aug", n, fn=lambda: (torch.arange(n) * 5 + 1) % 16, dtype=I32)
    inp_, dmo = k.out("input", (n, 1 + views, tile, tile)), k.out("dsm_mean_out", n)
    ws, nb = k.ws("ws", lib.rd_assemble_grid_tiles_ws_bytes(n, tile), short=(mode == 2))
    k.call("rd_assemble_grid_tiles_aug", dsm_in, None, ortho, planes, height, width, samples, pairs, n_pairs, views, 1, n, tile,
           -9999.0, mode, 1.5, 2.5, mode, 110.0, 60.0, aug, inp_, None, None, dmo, ws, nb, refuses_short=(mode == 2))

    def ref():
        from resdepth_amd import tiling
        if mode == 1:
            for i in (0, n - 1):
                y, x = smp[i][0], smp[i][1]
                plain = ((dsm_in[y:y + tile, x:x + tile].cpu() - 1.5) / 2.5).numpy()
                assert (inp_[i, 0].cpu().numpy() == tiling.tta_apply(plain, (i * 5 + 1) % 16)).all()
    k.ref(ref)


CASES = []
for s_ in [(3, 16, 8, 33, 41, 1), (70, 8, 4, 45, 37, 3), (5, 40, 24, 61, 93, 0)]:
    CASES.append(T._case(c_blend_tta, s_, ["rd_blend_accumulate_tta"], short=False))
for s_ in [(4, 8, 37, 45, 2, 2), (3, 16, 33, 19, 1, 1), (2, 72, 75, 131, 2, 2), (2, 8, 9, 11, 2, 0)]:
    CASES.append(T._case(c_grid_tiles_aug, s_, ["rd_assemble_grid_tiles_aug"], short=(s_[5] == 2)))


@pytest.fixture()
def lib():
    from resdepth_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("case", [pytest.param(c, id=c["id"]) for c in CASES])
def test_memory_contract(lib, case):
    T._full(lib, case)


@pytest.mark.parametrize("case", [pytest.param(c, id=c["id"]) for c in CASES if c["short"]])
def test_undersized_scratch_is_refused_and_nothing_is_written(lib, case):
    k, res = T._run_case(lib, case, fill="sentinel", short=True)
    assert k.short_seen and res is None, "the case never reached its undersized call"


def test_every_function_of_the_side_header_has_a_case():
    from resdepth_amd import _lib
    text = open(os.path.join(ROOT, "include", "resdepth_hip_tta.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    exported = set(re.findall(r"\b(rd_\w+)\s*\(", text))
    assert exported == set(_lib.SIGNATURES_TTA)
    covered = {f for c in CASES for f in c["covers"]}
    assert covered == exported, covered ^ exported
