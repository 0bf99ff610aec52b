"""The memory contract of include/resdepth_hip.h for the entry points of include/resdepth_hip_wloss.h: the guard-band cases that
tests/test_memory_contract_gpu.py runs for every entry point of the main header (its driver and judgement are used as they
are) -- guards intact, no sentinel left in an output, the same bits at shifted arena offsets and through the ops wrappers --
an undersized scratch that must be refused with nothing written, and the ledger over the side header: an entry point cannot
arrive there without a case here.

This module leans on that file's helpers (_case, _full, _run_case, _ops, _rand, _randint and the Case methods inp / pos / out /
ws / call / wrapper / ref), as tests/test_loss_contract_gpu.py does; test_the_borrowed_helpers_are_there names what is used."""
import os
import re
import struct

import pytest
import torch

import test_memory_contract_gpu as T
from test_memory_contract_gpu import F64, I32, U8

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_borrowed_helpers_are_there():
    for name in ("_case", "_full", "_run_case", "_ops", "_rand", "_randint", "F64", "U8", "I32"):
        assert hasattr(T, name), name


def c_weighted_loss(k, n, h, w, want, kind, lam):
    """both entry points on an [n][1][h][w] batch; want: which of d(yp), l(oss), m(ae) the finishing call is given (the others
    are NULL).  Shapes: scalar path (w % 4 != 0), single rows / columns / pixels (no pairs in one or both directions), the
    vector path, and a row wider than one tile.  Weights in [0, 1) with exact zeros."""
    lib, ops = k.lib, T._ops()
    yp, y = k.inp("yp", (n, 1, h, w)), k.inp("y", (n, 1, h, w))
    mask = k.inp("mask", (n, 1, h, w), dtype=U8)
    wt = k.inp("weight", (n, 1, h, w), fn=lambda: T._rand(17, n, 1, h, w) * (T._rand(18, n, 1, h, w) > 0.2))
    mean, std = k.inp("mean", n), k.pos("std", n)
    gout = k.inp("gout", 1, fn=lambda: torch.tensor([0.75]))
    sums = k.out("sums", 8, F64)
    ws, nb = k.ws("ws", lib.rd_weighted_loss_ws_bytes(n, h, w), short=True)
    k.call("rd_weighted_loss_partial", yp, y, mask, wt, mean, std, sums, n, h, w, kind, 0.5, 1.0, ws, nb, refuses_short=True)
    loss = k.out("loss", 1) if "l" in want else None
    mae = k.out("mae", 1) if "m" in want else None
    dyp = k.out("dyp", (n, 1, h, w)) if "d" in want else None
    k.call("rd_weighted_loss_finish", yp, y, mask, wt, mean, std, sums, float(n * h * w), kind, 0.5, 1.0, lam, gout, loss, mae,
           dyp, n, h, w)

    def wrap():
        s = ops.weighted_loss_partial(yp, y, mask, wt, mean, std, kind, 0.5, 1.0)
        lo, ma, d = ops.weighted_loss_finish(yp, y, mask, wt, mean, std, s, n * h * w, kind, 0.5, 1.0, lam, gout=gout,
                                             want_loss="l" in want, want_mae="m" in want, want_grad="d" in want)
        res = {"sums": s, "loss": lo, "mae": ma, "dyp": d}
        return {name: t for name, t in res.items() if t is not None}
    k.wrapper(wrap)


def c_train_weights(k, n, tile, views):
    """rd_assemble_train_weights over two rasters (fp32 weights with rows of 45 floats: never 16-byte rows; uint8 classes with
    rows of 36 bytes and a table), every orientation code, box-flagged samples, tiles in the rasters' last rows and columns, and
    one invalid row (it must be written too: NaN)."""
    dims = [(37, 45), (51, 36)]
    planes = [k.inp("weights0", dims[0], fn=lambda: T._rand(50, *dims[0]) * 4.0),
              k.inp("classes1", dims[1], fn=lambda: T._randint(51, 7, *dims[1]), dtype=U8)]
    table = k.inp("table1", 256, fn=lambda: T._rand(52, 256) * 3.0)
    rows = []
    if not k.plan:
        rows.append(struct.pack("<QQiiii", planes[0].data_ptr(), 0, 0, dims[0][0], dims[0][1], 0))
        rows.append(struct.pack("<QQiiii", planes[1].data_ptr(), table.data_ptr(), 1, dims[1][0], dims[1][1], 0))
    desc = k.inp("rasters", 32 * len(dims), fn=lambda: torch.frombuffer(bytearray(b"".join(rows)), dtype=U8), dtype=U8)
    cols = []
    for i in range(n):
        r = i % 2
        hh, ww = dims[r]
        last = i >= n - 2
        y0 = hh - tile if last else (5 * i) % (hh - tile + 1)
        x0 = ww - tile if last else (4 * i) % (ww - tile + 1)
        cols.append([r if i != 2 else 9, y0, x0, i % 32, i % 3, 0, 0, 0] + [0] * views)
    samples = k.inp("samples", ((8 + views) * n,), fn=lambda: torch.tensor(cols).t().contiguous().reshape(-1), dtype=I32)
    out = k.out("out", (n, 1, tile, tile))
    k.call("rd_assemble_train_weights", desc, len(dims), samples, n, views, tile, out)

    def wrap():
        return {"out": T._ops().assemble_train_weights(desc, len(dims), samples.view(8 + views, n), views, tile)}
    k.wrapper(wrap)

    def ref():
        assert bool(torch.isnan(out[2]).all()) and bool(torch.isfinite(out[:2]).all()) and bool(torch.isfinite(out[3:]).all())
        # sample 0: raster 0 at (0, 0), code 0; sample 1: raster 1, code 1 = rot90(k = 1) of the looked-up classes
        assert torch.equal(out[0, 0], planes[0][:tile, :tile])
        y1, x1 = cols[1][1], cols[1][2]
        assert torch.equal(out[1, 0], torch.rot90(table[planes[1][y1:y1 + tile, x1:x1 + tile].long()], 1))
    k.ref(ref)


SHAPES = [(3, 5, 7), (2, 1, 9), (2, 9, 1), (1, 1, 1), (2, 8, 16), (1, 6, 300)]
LOSS = ["rd_weighted_loss_ws_bytes", "rd_weighted_loss_partial", "rd_weighted_loss_finish"]
CASES = []
for i_, s_ in enumerate(SHAPES):
    for j_, want_ in enumerate(["dlm", "lm", "dm", "dl"]):
        # kinds 0, 1, 2 (l1, l2, huber) and both finishing kernels (with / without the halo ring) on every shape
        CASES.append(T._case(c_weighted_loss, s_ + (want_, (i_ + j_) % 3, 0.3 if j_ % 2 == 0 else 0.0), LOSS))
for s_ in SHAPES:
    CASES.append(T._case(c_weighted_loss, s_ + ("dlm", 0, 0.0), LOSS))          # plain L1 with a weight
TILES = [T._case(c_train_weights, a_, ["rd_assemble_train_weights"]) for a_ in [(34, 8, 2), (7, 12, 0), (5, 36, 1)]]


@pytest.fixture()
def lib():
    from resdepth_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("case", [pytest.param(c, id=c["id"]) for c in CASES + TILES])
def test_memory_contract(lib, case):
    T._full(lib, case)


@pytest.mark.parametrize("case", [pytest.param(c, id=c["id"]) for c in CASES if c["args"][3] == "dlm" and c["args"][5] > 0.0])
def test_undersized_scratch_is_refused_and_nothing_is_written(lib, case):
    k, res = T._run_case(lib, case, fill="sentinel", short=True)
    assert k.short_seen and res is None, "the case never reached its undersized call"


def test_every_function_of_the_side_header_has_a_case():
    from resdepth_amd import _lib
    text = open(os.path.join(ROOT, "include", "resdepth_hip_wloss.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    exported = set(re.findall(r"\b(rd_\w+)\s*\(", text))
    assert exported == set(_lib.SIGNATURES_WLOSS)
    covered = {f for c in CASES + TILES for f in c["covers"]}
    assert covered == exported, covered ^ exported
