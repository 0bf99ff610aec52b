"""The memory contract of include/resdepth_hip.h for the entry points of include/resdepth_hip_edt.h: the guard-band cases that
tests/test_memory_contract_gpu.py runs for every entry point of the main header (its driver and judgement are used as they are,
as tests/test_coreg_contract_gpu.py does; the arena is tests/arena.py) at ragged shapes, the scratch of rd_edt_sq exactly as its
query sizes it and one byte short, every refusal of the side header with nothing written, and the ledger over the side header: an
entry point cannot arrive there without a case here.

Every case is held bit for bit to the numpy oracles of tests/edt_ref.py."""
import os
import re

import numpy as np
import pytest
import torch

import edt_ref as R
import test_memory_contract_gpu as T
from test_memory_contract_gpu import F32, F64, I32, U8

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = R.BAND_ROWS


def test_the_borrowed_helpers_are_there():
    from arena import Arena, nbytes_of                 # noqa: F401
    for name in ("_case", "_full", "_run_case", "_randint", "F32", "F64", "U8", "I32", "DEV"):
        assert hasattr(T, name), name
    for name in ("inp", "out", "ws", "call", "ref"):
        assert hasattr(T.K, name), name


def c_edt(k, rows, cols, invert, with_idx, one_in):
    n = rows * cols
    mask = k.inp("mask", n, fn=lambda: (T._randint(rows * 131 + cols, one_in, n) == 0) * 3, dtype=U8)
    ws, nb = k.ws("ws", k.lib.rd_edt_ws_bytes(rows, cols), short=True)
    d2 = k.out("d2", n, I32)
    idx = k.out("idx", n, I32) if with_idx else None
    k.call("rd_edt_sq", mask, invert, rows, cols, d2, idx, ws, nb, refuses_short=True)

    def check():
        want = R.separable(mask.view(rows, cols).cpu().numpy(), invert=bool(invert))
        assert np.array_equal(d2.view(rows, cols).cpu().numpy(), want[0])
        assert idx is None or np.array_equal(idx.view(rows, cols).cpu().numpy(), want[1])
    k.ref(check)


def c_fill(k, n, f64, max_d2):
    dsm = k.inp("dsm", n, dtype=F64 if f64 else F32, scale=30.0)
    d2 = k.inp("d2", n, fn=lambda: torch.tensor([0, 1, 4, 25, 26, R.NONE])[T._randint(n, 6, n)], dtype=I32)
    idx = k.inp("idx", n, fn=lambda: T._randint(n + 1, n + 9, n) - 3, dtype=I32)      # -3 .. n + 5: below 0 and beyond n
    out = k.out("filled", n, F64 if f64 else F32)
    k.call("rd_fill_nearest", dsm, int(f64), d2, idx, n, max_d2, out)

    def check():
        want = R.fill_nearest(dsm.cpu().numpy(), d2.cpu().numpy(), idx.cpu().numpy(), max_d2)
        bits = np.uint64 if f64 else np.uint32
        assert np.array_equal(out.cpu().numpy().view(bits), want.view(bits))
    k.ref(check)


CASES = []
# (rows, cols, invert, idx asked for, one pixel in ... set): across the band height and the 256 threads of a block in both
# directions, rasters of one row and one column, an empty and a nearly full mask
for s_ in [(3, 3, 0, True, 3), (4, 70, 1, True, 9), (B + 3, 5, 0, True, 40), (130, 97, 0, False, 50), (1, 1, 0, True, 1), (1, 9, 1, True, 4),
           (9, 1, 0, False, 4), (2 * B + 1, 259, 0, True, 700), (35, 131, 1, True, 1000000), (B, 33, 0, True, 1000000)]:
    CASES.append(T._case(c_edt, s_, ["rd_edt_sq", "rd_edt_ws_bytes"]))
# (n, f64, max_d2): across the 256 threads of a block, no cap and a plain copy
for s_ in [(1, False, 25), (255, True, 1), (257, False, R.NONE - 1), (2311, True, 25), (70 * 33, False, 0), (777, True, R.NONE - 1)]:
    CASES.append(T._case(c_fill, s_, ["rd_fill_nearest"], short=False))


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


# ---- the refusals of the side header: RD_ERR_ARG (1), a message, nothing written -------------------------------------------------
ROWS, COLS = 21, 30
N = ROWS * COLS
GOOD = {
    "edt": dict(mask=1, d2=1, idx=1, ws=1, rows=ROWS, cols=COLS, ws_short=0, d2_at=None, idx_at=None),
    "fill": dict(dsm=1, d2=1, idx=1, out=1, n=N, max_d2=25, out_at=None),
}
BAD = {
    "edt": {
        "null mask": dict(mask=0), "null d2": dict(d2=0), "null ws": dict(ws=0), "no rows": dict(rows=0), "negative cols": dict(cols=-3),
        "too many rows": dict(rows=R.MAX_ROWS + 1), "too many cols": dict(cols=R.MAX_COLS + 1),      # refused before anything is read
        "both beyond the limits": dict(rows=2000000000, cols=2000000000),
        "ws one byte short": dict(ws_short=1), "no ws bytes": dict(ws_short=COLS * 8),
        # byte offsets from the mask's first byte (d2_at, idx_at) or from d2's (idx_at as a string)
        "d2 is the mask": dict(d2_at=0), "d2 begins in the mask's last bytes": dict(d2_at=N - 2), "idx is the mask": dict(idx_at=0),
        "idx ends in the mask's first bytes": dict(idx_at=4 - 4 * N), "idx is d2": dict(idx_at="0"),
        "idx begins in d2's last element": dict(idx_at=str(4 * N - 4)),
    },
    "fill": {
        "null dsm": dict(dsm=0), "null d2": dict(d2=0), "null idx": dict(idx=0), "null out": dict(out=0), "n 0": dict(n=0),
        "negative n": dict(n=-5), "max_d2 -1": dict(max_d2=-1), "max_d2 most negative": dict(max_d2=-2147483648),
        "out is dsm": dict(out_at=0), "out begins in dsm's last element": dict(out_at=8 * N - 8),
        "out ends in dsm's first element": dict(out_at=8 - 8 * N),
    },
}
REFUSALS = [(form, what, spec) for form in ("edt", "fill") for what, spec in BAD[form].items()]


def _refusal(lib, form, spec):
    from arena import Arena, nbytes_of
    a = dict(GOOD[form], **spec)
    ar = Arena(T.DEV, [nbytes_of((N,), F64)] * 6)
    mask = ar.alloc((N,), U8, fill=(T._randint(1, 9, N) == 0).to(U8), kind="input", name="mask")
    dsm = ar.alloc((N,), F64, fill=torch.randn(N, dtype=F64), kind="input", name="dsm")
    d2 = ar.alloc((N,), I32, fill=T._randint(2, 30, N).to(I32), kind="output" if form == "edt" else "input", name="d2")
    idx = ar.alloc((N,), I32, fill=T._randint(3, N, N).to(I32), kind="output" if form == "edt" else "input", name="idx")
    ws = ar.alloc((COLS * 8,), U8, fill="sentinel", kind="scratch", name="ws")
    out = ar.alloc((N,), F64, fill="sentinel", kind="output", name="out")
    p = lambda flag, t: t.data_ptr() if flag else None
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    snap = ar.snapshot()
    if form == "edt":
        nb = lib.rd_edt_ws_bytes(ROWS, COLS)
        assert nb == COLS * 8                           # 21 rows: one band
        d2_p, idx_p = p(a["d2"], d2), p(a["idx"], idx)
        if a["d2_at"] is not None:
            d2_p = mask.data_ptr() + a["d2_at"]
        if isinstance(a["idx_at"], str):
            idx_p = d2.data_ptr() + int(a["idx_at"])
        elif a["idx_at"] is not None:
            idx_p = mask.data_ptr() + a["idx_at"]
        rc = lib.rd_edt_sq(p(a["mask"], mask), 0, a["rows"], a["cols"], d2_p, idx_p, p(a["ws"], ws), nb - a["ws_short"], stream)
    else:
        out_p = p(a["out"], out) if a["out_at"] is None else dsm.data_ptr() + a["out_at"]
        rc = lib.rd_fill_nearest(p(a["dsm"], dsm), 1, p(a["d2"], d2), p(a["idx"], idx), a["n"], a["max_d2"], out_p, stream)
    msg = lib.rd_last_error_string()
    torch.cuda.synchronize()
    assert ar.same_as(snap), "the refused call changed memory"
    ar.check()
    return rc, msg


@pytest.mark.parametrize("form,what,spec", [pytest.param(f, w, s, id=f"{f}-{w.replace(' ', '_')}") for f, w, s in REFUSALS])
def test_refusals_write_nothing(lib, form, what, spec):
    rc, msg = _refusal(lib, form, spec)
    assert rc == 1 and msg, (what, rc, msg)


@pytest.mark.parametrize("form,spec", [("edt", {}), ("edt", dict(idx=0)), ("fill", {})], ids=["edt", "edt_without_idx", "fill"])
def test_the_refusal_driver_accepts_what_is_right(lib, form, spec):
    """the same driver with nothing wrong: the call goes through and writes -- the refusals above are refusals of their one defect"""
    with pytest.raises(AssertionError, match="changed memory"):
        _refusal(lib, form, spec)


def ledger_check():
    """every function of the side header is bound, exported and covered"""
    from resdepth_amd import _lib
    text = open(os.path.join(ROOT, "include", "resdepth_hip_edt.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    exported = set(re.findall(r"\b(rd_\w+)\s*\(", text))
    assert exported == set(_lib.SIGNATURES_EDT), exported ^ set(_lib.SIGNATURES_EDT)
    lib = _lib.load()
    for name in exported:
        assert hasattr(lib, name), name
    covered = {f for c in CASES for f in c["covers"]}
    assert covered == exported, covered ^ exported


def test_every_function_of_the_side_header_has_a_case():
    ledger_check()
