"""The memory contract of include/resdepth_hip.h for the entry points of include/resdepth_hip_optim.h: the guard-band cases that
tests/test_memory_contract_gpu.py runs for every entry point of the main header (its driver and judgement are used as they
are), an undersized scratch that must be refused with nothing written, and the ledger over the side header: an entry point
cannot arrive there without a case here.

This module leans on that file's helpers (_case, _full, _run_case, _ops and the Case methods inp / out / ws / call / wrapper /
ref), as tests/test_loss_contract_gpu.py does; test_the_borrowed_helpers_are_there names what is used."""
import os
import re

import pytest

import test_memory_contract_gpu as T
from test_memory_contract_gpu import F64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _defines():
    text = open(os.path.join(ROOT, "include", "resdepth_hip_optim.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define\s+(RD_\w+)\s+(\d+)", text)}


D = _defines()
VEC = D["RD_GNORM_VEC"]
BLOCK_SHARE = D["RD_GNORM_BLOCK"] * VEC                            # elements of one block of the first launch
NORM_WRAP = D["RD_GNORM_MAX_BLOCKS"] * BLOCK_SHARE                 # beyond it the grid-stride loop wraps


def test_the_borrowed_helpers_are_there():
    for name in ("_case", "_full", "_run_case", "_ops", "F64"):
        assert hasattr(T, name), name
    for name in ("inp", "out", "ws", "call", "wrapper", "ref"):
        assert hasattr(T.K, name), name


def c_grad_norm(k, numel, shift, bad):
    """rd_grad_norm on numel elements that start `shift` floats into their allocation (1: the buffer is not 16-byte aligned, the
    kernel reads element by element); bad: a NaN as the very last element and an Inf as the first (data, not a fault: they are
    counted and left out of the sum)."""
    lib, ops = k.lib, T._ops()
    full = numel + shift
    cut = (lambda t: t) if k.plan else (lambda t: t[shift:])

    def data():
        t = T._rand(numel + 7, full) * 6.0 - 3.0
        if bad:
            t[shift], t[full - 1] = float("inf"), float("nan")
        return t
    g = k.inp("g", full, fn=data)
    stats = k.out("stats", 2, F64)
    ws, nb = k.ws("ws", lib.rd_grad_norm_ws_bytes(numel), short=True)
    k.call("rd_grad_norm", cut(g), numel, stats, ws, nb, refuses_short=True)
    k.wrapper(lambda: {"stats": ops.grad_norm(cut(g))})

    def ref():
        want = (2.0 if numel > 1 else 1.0) if bad else 0.0
        assert float(k.outs["stats"][1]) == want and float(k.outs["stats"][0]) >= 0.0
    k.ref(ref)


ALL = ["rd_grad_norm_ws_bytes", "rd_grad_norm"]
# the smallest sizes at which the indexing can go wrong: single elements, the block size +- 1, one chunk +- 1, one element past
# one block's share, one element past the span of the capped grid (the grid-stride loop wraps) and past four times that span
# (the loop that keeps four chunks in flight runs, and hands its tail to the one-chunk loop)
SIZES = sorted({1, 3, 255, 256, 257, VEC - 1, VEC, VEC + 1, BLOCK_SHARE + 1, NORM_WRAP + 1, 4 * NORM_WRAP + 1})
CASES = [T._case(c_grad_norm, (n_, shift_, bad_), ALL) for n_ in SIZES for shift_ in (0, 1) for bad_ in (False, True)]


@pytest.fixture()
def lib():
    from resdepth_amd import _lib
    return _lib.load()


def test_the_sizes_come_from_the_kernels_constants():
    from resdepth_amd import _lib
    assert (VEC, BLOCK_SHARE, NORM_WRAP) == (_lib.GNORM_VEC, _lib.GNORM_BLOCK * _lib.GNORM_VEC,
                                             _lib.GNORM_MAX_BLOCKS * _lib.GNORM_BLOCK * _lib.GNORM_VEC)
    lib_ = _lib.load()
    assert lib_.rd_grad_norm_ws_bytes(NORM_WRAP) == lib_.rd_grad_norm_ws_bytes(NORM_WRAP + 1) == 16 * _lib.GNORM_MAX_BLOCKS


@pytest.mark.parametrize("case", [pytest.param(c, id=c["id"]) for c in CASES])
def test_memory_contract(lib, case):
    T._full(lib, case)


@pytest.mark.parametrize("case", [pytest.param(c, id=c["id"]) for c in CASES if not c["args"][2]])
def test_undersized_scratch_is_refused_and_nothing_is_written(lib, case):
    k, res = T._run_case(lib, case, fill="sentinel", short=True)
    assert k.short_seen and res is None, "the case never reached its undersized call"


def test_every_function_of_the_side_header_has_a_case():
    from resdepth_amd import _lib
    text = open(os.path.join(ROOT, "include", "resdepth_hip_optim.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    exported = set(re.findall(r"\b(rd_\w+)\s*\(", text))
    assert exported == set(_lib.SIGNATURES_OPTIM)
    covered = {f for c in CASES for f in c["covers"]}
    assert covered == exported, covered ^ exported
