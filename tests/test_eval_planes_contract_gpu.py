"""The memory contract of include/resdepth_hip.h for the entry points of include/resdepth_hip_eval.h: the guard-band cases that
tests/test_memory_contract_gpu.py runs for every entry point of the main header (its driver and judgement are used as they are,
as tests/test_pairs_contract_gpu.py does), plus the ledger over the side header: an entry point cannot arrive there without a
case here.  The cases cover residuals written in place and to a separate destination, planes padded apart by an odd stride,
every nullable pointer given and absent, and ragged n (odd row and column counts, one pixel).

The residual planes are `inout` allocations: the padding between planes must come back as it went in, which the reference
function of each case checks, and every case is held to a torch restatement bit for bit."""
import ctypes as C
import os
import re

import pytest
import torch

import test_memory_contract_gpu as T
from test_memory_contract_gpu import F32, F64, U8

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I16 = torch.int16
NODATA = -9999.0


def test_the_borrowed_helpers_are_there():
    for name in ("_case", "_full", "_run_case", "_rand", "F32", "F64", "U8"):
        assert hasattr(T, name), name


def _raster(seed, n, frac=0.1):
    """seeded values with nodata pixels"""
    v = T._rand(seed, n) * 8.0 - 4.0
    v[T._rand(seed + 100, n) < frac] = NODATA
    return v


def _planes(seed, n_planes, stride, n):
    """(n_planes - 1) * stride + n doubles: plane p at p * stride, every plane with nodata pixels of its own"""
    buf = T._rand(seed, (n_planes - 1) * stride + n).double() * 100.0 + 500.0          # what the padding holds
    for p in range(n_planes):
        buf[p * stride:p * stride + n] = _raster(seed + 7 * p + 1, n, 0.05 + 0.02 * (p % 5)).double()
    if n_planes > 3:
        # plane 3 is nodata wherever plane 2 is: no validity word can then be 0x7FFB (all planes but 2 and 15), which is one
        # half of the arena's sentinel and would read as an element the kernel never wrote
        buf[3 * stride:3 * stride + n][buf[2 * stride:2 * stride + n] == NODATA] = NODATA
    return buf


def c_classify_planes(k, rows, cols, n_planes, pad, in_place, masks, extra, before, f64):
    """rd_eval_classify_planes on a raster with odd sides, planes n + pad doubles apart; the last plane ends where its
    allocation ends"""
    n = rows * cols
    stride = n + pad
    span = (n_planes - 1) * stride + n
    data = lambda: _planes(11, n_planes, stride, n)                                   # noqa: E731
    if in_place:
        planes = res = k.inout("planes", span, fn=data, dtype=F64)
    else:
        planes = k.inp("planes", span, fn=data, dtype=F64)
        res = k.inout("residuals", span, dtype=F64)
    ft = F64 if f64 else F32
    init = k.inp("init", n, fn=lambda: _raster(21, n), dtype=ft)
    gt = k.inp("gt", n, fn=lambda: _raster(22, n), dtype=ft)
    m = {nm: (k.inp(nm, n, dtype=U8) if masks else None) for nm in ("gt_mask", "bdil", "bnod", "water", "forest")}
    ex = k.inp("extra", n, fn=lambda: _raster(23, n).double(), dtype=F64) if extra else None
    r_ex = k.out("r_extra", n, F64) if extra else None
    rb = k.out("r_before", n, F64) if before else None
    cls, valid = k.out("cls", n, U8), k.out("valid", n, I16)
    rects = (C.c_int * 8)(0, rows // 2 + 1, 0, cols, rows // 2, rows, 1, max(cols - 1, 1)) if masks else None
    k.call("rd_eval_classify_planes", planes, stride, n_planes, ex, init, int(f64), gt, int(f64), m["gt_mask"], m["bdil"],
           m["bnod"], m["water"], m["forest"], rects, 2 if masks else -1, rows, cols, NODATA, rb, res, r_ex, cls, valid)

    def ref():
        src = torch.as_tensor(data(), device=res.device)
        g = gt.double()
        y, x = torch.arange(n, device=res.device) // cols, torch.arange(n, device=res.device) % cols
        inside = torch.ones(n, dtype=torch.bool, device=res.device)
        if masks:
            inside = ((y >= 0) & (y < rows // 2 + 1)) | ((y >= rows // 2) & (x >= 1) & (x < max(cols - 1, 1)))
        gok = inside & (g != NODATA) & ((m["gt_mask"] != 0) if masks else True)
        want_v = torch.zeros(n, dtype=torch.int32, device=res.device)
        for p in range(n_planes):
            a = src[p * stride:p * stride + n]
            assert torch.equal(res[p * stride:p * stride + n], a - g), f"plane {p}"
            if p + 1 < n_planes:                                                      # padding as it went in
                first = k.first("planes" if in_place else "residuals")
                assert torch.equal(res[p * stride + n:(p + 1) * stride].view(torch.int64),
                                   first[p * stride + n:(p + 1) * stride].view(torch.int64)), f"padding after plane {p}"
            want_v |= (gok & (a != NODATA)).int() << p
        assert torch.equal(valid.int() & 0xFFFF, want_v)
        c = (gok & (init.double() != NODATA)).int()
        if masks:
            b = m["bdil"] != 0
            t = inside & ~b & (m["bnod"] == 0)
            tw = t & (m["water"] == 0)
            c |= (inside & b).int() * 4 | t.int() * 8 | tw.int() * 16 | (tw & (m["forest"] == 0)).int() * 32
        if extra:
            c |= (gok & (ex != NODATA)).int() * 64
            assert torch.equal(r_ex, ex - g)
        assert torch.equal(cls.int(), c)
        if before:
            assert torch.equal(rb, init.double() - g)
    k.ref(ref)


def c_pooled(k, n, n_planes, pad, p0, p1, with_valid, ns):
    """rd_residual_stats_pooled over planes p0 .. p1 - 1 of n_planes planes n + pad doubles apart: the planes outside the range
    and the padding hold NaN-free garbage that must not enter; the workspace is exactly what the query says"""
    stride = n + pad
    span = (n_planes - 1) * stride + n
    src = k.inp("src", span, dtype=F64, scale=2.0)
    cls = k.inp("cls", n, fn=lambda: T._randint(6, 64, n), dtype=U8)
    valid = k.inp("valid", n, fn=lambda: T._randint(7, 1 << n_planes, n), dtype=I16) if with_valid else None
    out = k.out("sets", (ns, 8), F64)
    need = [0, 4, 8, 8 | 16, 32][:ns]
    thr = [-1.0, 2.5, 0.0, 1.0, -1.0][:ns]
    ws, nb = k.ws("ws", k.lib.rd_residual_stats_pooled_ws_bytes(n, ns), short=True)
    k.call("rd_residual_stats_pooled", src, stride, n_planes, p0, p1, cls, valid, n, (C.c_int * ns)(*need),
           (C.c_double * ns)(*thr), ns, out, ws, nb, refuses_short=True)

    def ref():
        for s in range(ns):
            vals = []
            for p in range(p0, p1):
                r = src[p * stride:p * stride + n]
                ok = (cls.int() & need[s]) == need[s]
                if with_valid:
                    ok &= ((valid.int() >> p) & 1) != 0
                if thr[s] > 0:
                    ok &= r.abs() <= thr[s]
                vals.append(r[ok])
            v = torch.cat(vals).sort().values
            cnt = v.numel()
            assert int(out[s, 0]) == cnt, (s, int(out[s, 0]), cnt)
            if cnt:
                assert float(out[s, 1]) == float(v[-1]) and float(out[s, 2]) == float(v[0])
                assert float(out[s, 6]) == float(0.5 * (v[(cnt - 1) // 2] + v[cnt // 2]))
            else:
                assert bool(torch.isnan(out[s, 1:]).all())
    k.ref(ref)


CASES = []
# (rows, cols, planes, pad, in place, masks, extra, r_before, f64 DSMs)
for s_ in [(37, 45, 3, 0, True, True, True, True, False), (37, 45, 3, 3, False, True, False, True, False),
           (37, 45, 16, 1, True, True, True, False, True), (1, 1, 2, 5, False, False, False, False, False),
           (5, 301, 1, 0, False, False, True, True, True), (129, 257, 4, 7, True, True, False, False, False)]:
    CASES.append(T._case(c_classify_planes, s_, ["rd_eval_classify_planes"], short=False))
# (n, planes, pad, p0, p1, valid given, sets)
for s_ in [(1665, 3, 0, 0, 3, True, 5), (1665, 3, 3, 1, 2, True, 2), (1, 2, 5, 0, 2, False, 1), (4097, 16, 1, 0, 16, True, 5),
           (4097, 16, 1, 15, 16, False, 3), (70001, 4, 9, 1, 4, True, 5)]:
    CASES.append(T._case(c_pooled, s_, ["rd_residual_stats_pooled"]))


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


def ledger_check():
    """every function of the side header is bound, exported and covered (no GPU work: tests/test_eval_pairs_cpu.py runs it in
    the CPU suite too); size queries are exempt as in the main ledger"""
    from resdepth_amd import _lib
    text = open(os.path.join(ROOT, "include", "resdepth_hip_eval.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    exported = set(re.findall(r"\b(rd_\w+)\s*\(", text))
    assert exported == set(_lib.SIGNATURES_EVAL), exported ^ set(_lib.SIGNATURES_EVAL)
    lib = _lib.load()
    for name in exported:
        assert hasattr(lib, name), name
    covered = {f for c in CASES for f in c["covers"]}
    need = {f for f in exported if not re.fullmatch(r"rd_\w+_ws_bytes", f)}
    assert covered == need, covered ^ need


def test_every_function_of_the_side_header_has_a_case():
    ledger_check()
