"""The memory contract of include/resdepth_hip.h for the entry points of include/resdepth_hip_loss.h: the guard-band cases that
tests/test_memory_contract_gpu.py runs for every entry point of the main header (its driver and judgement are used as they
are), an undersized scratch that must be refused with nothing written, and the ledger over the side header: an entry point
cannot arrive there without a case here.

This module leans on that file's helpers (_case, _full, _run_case, _ops and the Case methods inp / pos / out / ws / call /
wrapper), as tests/test_pairs_contract_gpu.py does; test_the_borrowed_helpers_are_there names what is used."""
import os
import re

import pytest
import torch

import test_memory_contract_gpu as T
from test_memory_contract_gpu import F64, U8

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_borrowed_helpers_are_there():
    for name in ("_case", "_full", "_run_case", "_ops", "F64", "U8"):
        assert hasattr(T, name), name


def c_masked_loss(k, n, h, w, want, kind, lam):
    """both entry points on an [n][1][h][w] batch; want: which of d(yp), l(oss), m(ae) the finishing call is given (the others
    are NULL).  Shapes: scalar path (w % 4 != 0), single rows / columns / pixels (no pairs in one or both directions), the
    vector path, and a row wider than one tile."""
    lib, ops = k.lib, T._ops()
    yp, y = k.inp("yp", (n, 1, h, w)), k.inp("y", (n, 1, h, w))
    mask = k.inp("mask", (n, 1, h, w), dtype=U8)
    mean, std = k.inp("mean", n), k.pos("std", n)
    gout = k.inp("gout", 1, fn=lambda: torch.tensor([0.75]))
    sums = k.out("sums", 8, F64)
    ws, nb = k.ws("ws", lib.rd_masked_loss_ws_bytes(n, h, w), short=True)
    k.call("rd_masked_loss_partial", yp, y, mask, mean, std, sums, n, h, w, kind, 0.5, 1.0, ws, nb, refuses_short=True)
    loss = k.out("loss", 1) if "l" in want else None
    mae = k.out("mae", 1) if "m" in want else None
    dyp = k.out("dyp", (n, 1, h, w)) if "d" in want else None
    k.call("rd_masked_loss_finish", yp, y, mask, mean, std, sums, float(n * h * w), kind, 0.5, 1.0, lam, gout, loss, mae, dyp,
           n, h, w)

    def wrap():
        s = ops.masked_loss_partial(yp, y, mask, mean, std, kind, 0.5, 1.0)
        lo, ma, d = ops.masked_loss_finish(yp, y, mask, mean, std, s, n * h * w, kind, 0.5, 1.0, lam, gout=gout,
                                           want_loss="l" in want, want_mae="m" in want, want_grad="d" in want)
        res = {"sums": s, "loss": lo, "mae": ma, "dyp": d}
        return {name: t for name, t in res.items() if t is not None}
    k.wrapper(wrap)


SHAPES = [(3, 5, 7), (2, 1, 9), (2, 9, 1), (1, 1, 1), (2, 8, 16), (1, 6, 300)]
ALL = ["rd_masked_loss_ws_bytes", "rd_masked_loss_partial", "rd_masked_loss_finish"]
CASES = []
for i_, s_ in enumerate(SHAPES):
    for j_, want_ in enumerate(["dlm", "lm", "dm", "dl"]):
        # kinds 0, 1, 2 (l1, l2, huber) and both finishing kernels (with / without the halo ring) on every shape
        CASES.append(T._case(c_masked_loss, s_ + (want_, (i_ + j_) % 3, 0.3 if j_ % 2 == 0 else 0.0), ALL))
for s_ in SHAPES:
    CASES.append(T._case(c_masked_loss, s_ + ("dlm", 2, 0.0), ALL))


@pytest.fixture()
def lib():
    from resdepth_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("case", [pytest.param(c, id=c["id"]) for c in CASES])
def test_memory_contract(lib, case):
    T._full(lib, case)


@pytest.mark.parametrize("case", [pytest.param(c, id=c["id"]) for c in CASES if c["args"][3] == "dlm" and c["args"][5] > 0.0])
def test_undersized_scratch_is_refused_and_nothing_is_written(lib, case):
    k, res = T._run_case(lib, case, fill="sentinel", short=True)
    assert k.short_seen and res is None, "the case never reached its undersized call"


def test_every_function_of_the_side_header_has_a_case():
    from resdepth_amd import _lib
    text = open(os.path.join(ROOT, "include", "resdepth_hip_loss.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    exported = set(re.findall(r"\b(rd_\w+)\s*\(", text))
    assert exported == set(_lib.SIGNATURES_LOSS)
    covered = {f for c in CASES for f in c["covers"]}
    assert covered == exported, covered ^ exported
