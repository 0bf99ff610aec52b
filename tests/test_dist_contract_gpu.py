"""The memory contract of include/resdepth_hip.h for the entry points of include/resdepth_hip_dist.h: the guard-band cases that
tests/test_memory_contract_gpu.py runs for every entry point of the main header (its driver and judgement are used as they are,
as tests/test_eval_planes_contract_gpu.py does), every refusal of the side header with nothing written, an undersized scratch,
and the ledger over the side header: an entry point cannot arrive there without a case here.

Every case is held to a torch restatement: counts and shares exactly, quantiles of level 0 and 1 exactly (the smallest and the
largest member) and the others between their two neighbours in the sorted members; tests/test_dist_gpu.py has the bits."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import test_memory_contract_gpu as T
from test_memory_contract_gpu import F64, U8

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I16 = torch.int16
NEED = [0, 4, 8, 8 | 16, 32]
THR = [-1.0, 2.5, 0.0, 1.0, -1.0]
LEVELS, MODES, TAUS = [0.0, 0.9, 1.0, 0.5], [1, 1, 0, 0], [0.0, 1.0, 1e300]


def test_the_borrowed_helpers_are_there():
    for name in ("_case", "_full", "_run_case", "_randint", "F64", "U8"):
        assert hasattr(T, name), name
    for name in ("inp", "out", "ws", "call", "ref"):
        assert hasattr(T.K, name), name


def _arr(ctype, values):
    return (ctype * max(len(values), 1))(*values)


def _judge(out, members, ns, nq, nt):
    """out [ns, 1 + nq + nt] against members(s) -> the set's values as a tensor"""
    for s in range(ns):
        v = members(s)
        cnt = v.numel()
        assert int(out[s, 0]) == cnt, (s, int(out[s, 0]), cnt)
        if not cnt:
            assert bool(torch.isnan(out[s, 1:]).all())
            continue
        for j in range(nq):
            r = (v.abs() if MODES[j] else v).sort().values
            h = (cnt - 1) * LEVELS[j]
            lo, hi = r[int(math.floor(h))], r[int(math.ceil(h))]
            q = float(out[s, 1 + j])
            assert float(lo) <= q <= float(hi), (s, j, float(lo), q, float(hi))
            if LEVELS[j] in (0.0, 1.0):
                assert q == float(lo)
        for t in range(nt):
            assert float(out[s, 1 + nq + t]) == int((v.abs() <= TAUS[t]).sum()) / cnt, (s, t)


def c_dist_sets(k, n, ns, nq, nt, two):
    """rd_residual_dist_sets on n values of two sources (or of one: src1 NULL), the scratch exactly what the query says"""
    src0 = k.inp("src0", n, dtype=F64, scale=2.0)
    src1 = k.inp("src1", n, dtype=F64, scale=2.0) if two else None
    cls = k.inp("cls", n, fn=lambda: T._randint(6, 64, n), dtype=U8)
    out = k.out("dist", (ns, 1 + nq + nt), F64)
    which = [(s & 1) if two else 0 for s in range(ns)]
    ws, nb = k.ws("ws", k.lib.rd_residual_dist_sets_ws_bytes(n, ns, nq, nt), short=True)
    k.call("rd_residual_dist_sets", src0, src1, cls, n, _arr(C.c_int, which), _arr(C.c_int, NEED[:ns]), _arr(C.c_double, THR[:ns]),
           ns, _arr(C.c_double, LEVELS[:nq]), _arr(C.c_int, MODES[:nq]), nq, _arr(C.c_double, TAUS[:nt]), nt, out, ws, nb,
           refuses_short=True)

    def members(s):
        r = src1 if which[s] else src0
        ok = (cls.int() & NEED[s]) == NEED[s]
        if THR[s] > 0:
            ok &= r.abs() <= THR[s]
        return r[ok]
    k.ref(lambda: _judge(out, members, ns, nq, nt))


def c_dist_pooled(k, n, n_planes, pad, p0, p1, with_valid, ns, nq, nt):
    """rd_residual_dist_pooled over planes p0 .. p1 - 1 of n_planes planes n + pad doubles apart: the planes outside the range
    and the padding hold garbage that must not enter"""
    stride = n + pad
    span = (n_planes - 1) * stride + n
    src = k.inp("src", span, dtype=F64, scale=2.0)
    cls = k.inp("cls", n, fn=lambda: T._randint(6, 64, n), dtype=U8)
    valid = k.inp("valid", n, fn=lambda: T._randint(7, 1 << n_planes, n), dtype=I16) if with_valid else None
    out = k.out("dist", (ns, 1 + nq + nt), F64)
    ws, nb = k.ws("ws", k.lib.rd_residual_dist_pooled_ws_bytes(n, ns, nq, nt), short=True)
    k.call("rd_residual_dist_pooled", src, stride, n_planes, p0, p1, cls, valid, n, _arr(C.c_int, NEED[:ns]),
           _arr(C.c_double, THR[:ns]), ns, _arr(C.c_double, LEVELS[:nq]), _arr(C.c_int, MODES[:nq]), nq,
           _arr(C.c_double, TAUS[:nt]), nt, out, ws, nb, refuses_short=True)

    def members(s):
        vals = []
        for p in range(p0, p1):
            r = src[p * stride:p * stride + n]
            ok = (cls.int() & NEED[s]) == NEED[s]
            if with_valid:
                ok &= ((valid.int() >> p) & 1) != 0
            if THR[s] > 0:
                ok &= r.abs() <= THR[s]
            vals.append(r[ok])
        return torch.cat(vals)
    k.ref(lambda: _judge(out, members, ns, nq, nt))


CASES = []
# (n, sets, quantiles, tolerances, two sources): ragged sizes, one value, one histogram round and one more
for s_ in [(1665, 5, 4, 3, True), (1, 1, 1, 1, False), (4097, 5, 4, 0, True), (4097, 3, 0, 3, False), (70001, 5, 4, 3, True)]:
    CASES.append(T._case(c_dist_sets, s_, ["rd_residual_dist_sets"]))
# (n, planes, pad, p0, p1, valid given, sets, quantiles, tolerances)
for s_ in [(1665, 3, 0, 0, 3, True, 5, 4, 3), (1665, 3, 3, 1, 2, True, 2, 4, 3), (1, 2, 5, 0, 2, False, 1, 1, 1),
           (4097, 16, 1, 0, 16, True, 5, 4, 0), (4097, 16, 1, 15, 16, False, 3, 0, 3), (70001, 4, 9, 1, 4, True, 5, 4, 3)]:
    CASES.append(T._case(c_dist_pooled, s_, ["rd_residual_dist_pooled"]))


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
N, NS = 300, 2
NAN, INF = float("nan"), float("inf")
GOOD = dict(n_sets=NS, q=[0.5, 0.9], mode=[0, 1], n_q=2, tau=[1.0], n_t=1, p0=0, p1=2, n=N)
BAD = {
    "nothing asked": dict(q=[], mode=[], n_q=0, tau=[], n_t=0),
    "nine quantiles": dict(q=[0.5] * 9, mode=[0] * 9, n_q=9),
    "nine tolerances": dict(tau=[1.0] * 9, n_t=9),
    "negative n_q": dict(n_q=-1),
    "level above one": dict(q=[0.5, 1.0000001]),
    "level below zero": dict(q=[-1e-9, 0.9]),
    "level NaN": dict(q=[NAN, 0.9]),
    "level Inf": dict(q=[0.5, INF]),
    "mode 2": dict(mode=[0, 2]),
    "mode -1": dict(mode=[-1, 1]),
    "negative tolerance": dict(tau=[-0.5]),
    "tolerance NaN": dict(tau=[NAN]),
    "tolerance Inf": dict(tau=[INF]),
    "no sets": dict(n_sets=0),
    "twenty-one sets": dict(n_sets=21),
}
# 32-bit histogram counters: (p1 - p0) * n = 2^32 in the pooled form, n = 2^32 in the sets form; refused before anything is read
TOO_MANY = {"pooled": dict(n=1 << 31), "sets": dict(n=1 << 32)}
REFUSALS = [(form, what, spec) for form in ("sets", "pooled") for what, spec in list(BAD.items()) + [("2^32 values", TOO_MANY[form])]]


def _refusal(lib, form, spec):
    from resdepth_amd import _lib as L
    from arena import Arena, nbytes_of
    a = dict(GOOD, **spec)
    ar = Arena(T.DEV, [nbytes_of((2 * N + 3,), F64), nbytes_of((N,), U8), nbytes_of((N,), I16), nbytes_of((21 * 17,), F64), 1 << 16])
    src = ar.alloc((2 * N + 3,), F64, fill=torch.randn(2 * N + 3, dtype=F64), kind="input", name="src")
    cls = ar.alloc((N,), U8, fill=torch.ones(N, dtype=U8), kind="input", name="cls")
    valid = ar.alloc((N,), I16, fill=torch.full((N,), 3, dtype=I16), kind="input", name="valid")
    out = ar.alloc((21 * 17,), F64, fill="sentinel", kind="output", name="out")
    ws = ar.alloc((1 << 16,), U8, fill="sentinel", kind="scratch", name="ws")
    need, thr = _arr(C.c_int, [1] * 21), _arr(C.c_double, [-1.0] * 21)
    q, mode, tau = _arr(C.c_double, a["q"]), _arr(C.c_int, a["mode"]), _arr(C.c_double, a["tau"])
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    snap = ar.snapshot()
    if form == "sets":
        rc = lib.rd_residual_dist_sets(src.data_ptr(), src[N + 3:].data_ptr(), cls.data_ptr(), a["n"], _arr(C.c_int, [0] * 21), need,
                                       thr, a["n_sets"], q, mode, a["n_q"], tau, a["n_t"], out.data_ptr(), ws.data_ptr(), ws.numel(),
                                       stream)
    else:
        rc = lib.rd_residual_dist_pooled(src.data_ptr(), max(a["n"], N) + 3, 2, a["p0"], a["p1"], cls.data_ptr(), valid.data_ptr(),
                                         a["n"], need, thr, a["n_sets"], q, mode, a["n_q"], tau, a["n_t"], out.data_ptr(),
                                         ws.data_ptr(), ws.numel(), stream)
    msg = lib.rd_last_error_string()
    torch.cuda.synchronize()
    assert ar.same_as(snap), "the refused call changed memory"
    ar.check()
    return rc, msg


@pytest.mark.parametrize("form,what,spec", [pytest.param(f, w, s, id=f"{f}-{w.replace(' ', '_')}") for f, w, s in REFUSALS])
def test_refusals_write_nothing(lib, form, what, spec):
    rc, msg = _refusal(lib, form, spec)
    assert rc == 1 and msg, (what, rc, msg)


@pytest.mark.parametrize("form", ["sets", "pooled"])
def test_the_refusal_driver_accepts_what_is_right(lib, form):
    """the same driver with nothing wrong: the call goes through and writes -- the refusals above are refusals of their one defect"""
    with pytest.raises(AssertionError, match="changed memory"):
        _refusal(lib, form, {})


def ledger_check():
    """every function of the side header is bound, exported and covered; size queries are exempt as in the main ledger"""
    from resdepth_amd import _lib
    text = open(os.path.join(ROOT, "include", "resdepth_hip_dist.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    exported = set(re.findall(r"\b(rd_\w+)\s*\(", text))
    assert exported == set(_lib.SIGNATURES_DIST), exported ^ set(_lib.SIGNATURES_DIST)
    lib = _lib.load()
    for name in exported:
        assert hasattr(lib, name), name
    covered = {f for c in CASES for f in c["covers"]}
    need = {f for f in exported if not re.fullmatch(r"rd_\w+_ws_bytes", f)}
    assert covered == need, covered ^ need


def test_every_function_of_the_side_header_has_a_case():
    ledger_check()
