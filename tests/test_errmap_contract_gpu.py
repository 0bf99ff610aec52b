"""The memory contract of include/resdepth_hip.h for the entry points of include/resdepth_hip_errmap.h: the guard-band cases that
tests/test_memory_contract_gpu.py runs for every entry point of the main header (its driver and judgement are used as they are,
as tests/test_dist_contract_gpu.py does) at ragged shapes, every refusal of the side header with nothing written, and the ledger
over the side header: an entry point cannot arrive there without a case here.

Every case is held to a torch restatement of what needs no sort: counts, maxima and minima of the cells; the NaN pattern of the
slope; the bytes of the bins.  tests/test_errmap_gpu.py has the rest."""
import ctypes as C
import os
import re

import pytest
import torch

import test_memory_contract_gpu as T
from test_memory_contract_gpu import F32, F64, U8

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def test_the_borrowed_helpers_are_there():
    for name in ("_case", "_full", "_run_case", "_randint", "F32", "F64", "U8", "DEV"):
        assert hasattr(T, name), name
    for name in ("inp", "out", "call", "ref"):
        assert hasattr(T.K, name), name


def c_cell_stats(k, rows, cols, cell_h, cell_w, need, thr):
    n = rows * cols
    src = k.inp("src", n, dtype=F64, scale=2.0)
    cls = k.inp("cls", n, fn=lambda: T._randint(6, 64, n), dtype=U8)
    ncy, ncx = -(-rows // cell_h), -(-cols // cell_w)
    out = k.out("cells", (ncy, ncx, 8), F64)
    k.call("rd_cell_stats", src, cls, rows, cols, cell_h, cell_w, need, float(thr), out)

    def ref():
        r, c = src.view(rows, cols), cls.view(rows, cols).int()
        for cy in range(ncy):
            for cx in range(ncx):
                win = (slice(cy * cell_h, (cy + 1) * cell_h), slice(cx * cell_w, (cx + 1) * cell_w))
                ok = (c[win] & need) == need
                if thr > 0:
                    ok &= r[win].abs() <= thr
                v = r[win][ok]
                row = out[cy, cx]
                assert int(row[0]) == v.numel(), (cy, cx, float(row[0]), v.numel())
                if v.numel():
                    assert float(row[1]) == float(v.max()) and float(row[2]) == float(v.min()), (cy, cx)
                    assert float(v.min()) <= float(row[6]) <= float(v.max()) and 0 <= float(row[5]) <= float(v.abs().max())
                    assert bool(torch.isfinite(row).all())
                else:
                    assert bool(torch.isnan(row[1:]).all())
    k.ref(ref)


def c_dsm_slope(k, rows, cols, f64):
    dt = F64 if f64 else F32
    n = rows * cols

    def heights():
        z = torch.randn(n, generator=torch.Generator().manual_seed(rows * 131 + cols)) * 5.0 + 300.0
        z[T._randint(3, 20, n) == 0] = -9999.0
        return z
    dsm = k.inp("dsm", n, fn=heights, dtype=dt)
    slope = k.out("slope", (rows, cols), F64)
    k.call("rd_dsm_slope", dsm, int(f64), rows, cols, -9999.0, 0.5, 0.25, slope)

    def ref():
        bad = (dsm.view(rows, cols) == -9999.0)
        want = torch.ones((rows, cols), dtype=torch.bool, device=bad.device)
        if rows >= 3 and cols >= 3:
            near = torch.nn.functional.max_pool2d(bad[None, None].float(), 3, 1)[0, 0] > 0
            want[1:-1, 1:-1] = near
        assert torch.equal(torch.isnan(slope), want)
        assert bool((slope[~want] >= 0).all())
    k.ref(ref)


def c_bin_classes(k, n, n_bins, f64):
    dt = F64 if f64 else F32
    by = k.inp("by", n, dtype=dt, scale=4.0)
    cls = k.inp("cls", n, fn=lambda: T._randint(9, 64, n), dtype=U8)
    groups = -(-n_bins // 6)
    out = k.out("planes", (groups, n), U8)
    edges = [-6.0 + 0.5 * i for i in range(n_bins + 1)]
    k.call("rd_bin_classes", by, int(f64), cls, n, (C.c_double * (n_bins + 1))(*edges), n_bins, out)

    def ref():
        v = by.double()
        b = torch.floor((v + 6.0) / 0.5).long()                      # edges on multiples of 0.5: exact
        b[(v < edges[0]) | ~(v < edges[-1])] = -1
        for g in range(groups):
            q = b - 6 * g
            bit = torch.where((b >= 0) & (q >= 0) & (q < 6), torch.bitwise_left_shift(torch.full_like(q, 4), q.clamp(0, 5)),
                              torch.zeros_like(q))
            assert torch.equal(out[g].long(), (cls.long() & 3) | bit), g
    k.ref(ref)


CASES = []
# (rows, cols, cell_h, cell_w, need, thr): ragged borders, one pixel, a cell wider than the raster, the largest cell
for s_ in [(37, 53, 8, 8, 0, 0.0), (1, 1, 4, 4, 0, 0.0), (9, 70, 4, 64, 4, 1.5), (300, 260, 256, 256, 8 | 16, 0.0), (41, 17, 5, 7, 32, 2.5)]:
    CASES.append(T._case(c_cell_stats, s_, ["rd_cell_stats"], short=False))
# (rows, cols, f64): across the 64 x 16 tile in both directions, and rasters with no interior
for s_ in [(3, 3, True), (4, 70, False), (67, 5, True), (130, 97, False), (2, 9, True), (1, 1, False)]:
    CASES.append(T._case(c_dsm_slope, s_, ["rd_dsm_slope"], short=False))
# (n, bins, f64): one to four planes
for s_ in [(1665, 1, True), (1, 6, False), (4097, 7, False), (70001, 24, True)]:
    CASES.append(T._case(c_bin_classes, s_, ["rd_bin_classes"], short=False))


@pytest.fixture()
def lib():
    from resdepth_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("case", [pytest.param(c, id=c["id"]) for c in CASES])
def test_memory_contract(lib, case):
    T._full(lib, case)


# ---- the refusals of the side header: RD_ERR_ARG (1), a message, nothing written -------------------------------------------------
ROWS, COLS, NB = 21, 30, 7
GOOD = {
    "cell": dict(src=1, cls=1, out=1, rows=ROWS, cols=COLS, cell_h=8, cell_w=8, need=1, thr=0.0),
    "slope": dict(dsm=1, slope=1, rows=ROWS, cols=COLS, gsd_x=0.5, gsd_y=0.5),
    "bins": dict(by=1, cls=1, edges=[float(i) for i in range(NB + 1)], out=1, n=ROWS * COLS, n_bins=NB),
}
BAD = {
    "cell": {
        "null src": dict(src=0), "null cls": dict(cls=0), "null out": dict(out=0), "no rows": dict(rows=0),
        "negative cols": dict(cols=-3), "cell_h 3": dict(cell_h=3), "cell_h 257": dict(cell_h=257), "cell_w 3": dict(cell_w=3),
        "cell_w 257": dict(cell_w=257), "need -1": dict(need=-1), "need 256": dict(need=256), "negative thr": dict(thr=-1.0),
        "thr NaN": dict(thr=NAN), "thr Inf": dict(thr=INF),
        "2^24 cells": dict(rows=16384, cols=16384, cell_h=4, cell_w=4),        # refused before anything is read
    },
    "slope": {
        "null dsm": dict(dsm=0), "null slope": dict(slope=0), "no rows": dict(rows=0), "no cols": dict(cols=0),
        "gsd_x 0": dict(gsd_x=0.0), "gsd_y negative": dict(gsd_y=-0.5), "gsd_x NaN": dict(gsd_x=NAN), "gsd_y Inf": dict(gsd_y=INF),
        "too many rows": dict(rows=1048561, cols=1),
    },
    "bins": {
        "null by": dict(by=0), "null cls": dict(cls=0), "null edges": dict(edges=None), "null out": dict(out=0), "n 0": dict(n=0),
        "no bins": dict(n_bins=0), "25 bins": dict(n_bins=25, edges=[float(i) for i in range(26)]),
        "NaN edge": dict(edges=[0.0, 1.0, NAN, 3.0, 4.0, 5.0, 6.0, 7.0]),
        "NaN first edge": dict(edges=[NAN, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]),
        "equal edges": dict(edges=[0.0, 1.0, 1.0, 3.0, 4.0, 5.0, 6.0, 7.0]),
        "falling edges": dict(edges=[0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 7.0, 6.0]),
    },
}
REFUSALS = [(form, what, spec) for form in ("cell", "slope", "bins") for what, spec in BAD[form].items()]


def _refusal(lib, form, spec):
    from arena import Arena, nbytes_of
    a = dict(GOOD[form], **spec)
    n = ROWS * COLS
    ar = Arena(T.DEV, [nbytes_of((n,), F64), nbytes_of((n,), U8), nbytes_of((4 * n,), F64)])
    val = ar.alloc((n,), F64, fill=torch.randn(n, dtype=F64), kind="input", name="values")
    cls = ar.alloc((n,), U8, fill=torch.ones(n, dtype=U8), kind="input", name="cls")
    out = ar.alloc((4 * n,), F64, fill="sentinel", kind="output", name="out")
    p = lambda flag, t: t.data_ptr() if flag else None
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    snap = ar.snapshot()
    if form == "cell":
        rc = lib.rd_cell_stats(p(a["src"], val), p(a["cls"], cls), a["rows"], a["cols"], a["cell_h"], a["cell_w"], a["need"], a["thr"],
                               p(a["out"], out), stream)
    elif form == "slope":
        rc = lib.rd_dsm_slope(p(a["dsm"], val), 1, a["rows"], a["cols"], -9999.0, a["gsd_x"], a["gsd_y"], p(a["slope"], out), stream)
    else:
        edges = None if a["edges"] is None else (C.c_double * len(a["edges"]))(*a["edges"])
        rc = lib.rd_bin_classes(p(a["by"], val), 1, p(a["cls"], cls), a["n"], edges, a["n_bins"], p(a["out"], out), stream)
    msg = lib.rd_last_error_string()
    torch.cuda.synchronize()
    assert ar.same_as(snap), "the refused call changed memory"
    ar.check()
    return rc, msg


@pytest.mark.parametrize("form,what,spec", [pytest.param(f, w, s, id=f"{f}-{w.replace(' ', '_')}") for f, w, s in REFUSALS])
def test_refusals_write_nothing(lib, form, what, spec):
    rc, msg = _refusal(lib, form, spec)
    assert rc == 1 and msg, (what, rc, msg)


@pytest.mark.parametrize("form", ["cell", "slope", "bins"])
def test_the_refusal_driver_accepts_what_is_right(lib, form):
    """the same driver with nothing wrong: the call goes through and writes -- the refusals above are refusals of their one defect"""
    with pytest.raises(AssertionError, match="changed memory"):
        _refusal(lib, form, {})


def ledger_check():
    """every function of the side header is bound, exported and covered"""
    from resdepth_amd import _lib
    text = open(os.path.join(ROOT, "include", "resdepth_hip_errmap.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    exported = set(re.findall(r"\b(rd_\w+)\s*\(", text))
    assert exported == set(_lib.SIGNATURES_ERRMAP), exported ^ set(_lib.SIGNATURES_ERRMAP)
    lib = _lib.load()
    for name in exported:
        assert hasattr(lib, name), name
    covered = {f for c in CASES for f in c["covers"]}
    assert covered == exported, covered ^ exported


def test_every_function_of_the_side_header_has_a_case():
    ledger_check()
