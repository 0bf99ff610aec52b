"""The memory contract of include/resdepth_hip.h for the entry points of include/resdepth_hip_coreg.h: the guard-band cases that
tests/test_memory_contract_gpu.py runs for every entry point of the main header (its driver and judgement are used as they are,
as tests/test_errmap_contract_gpu.py does; the arena is tests/arena.py) at ragged shapes, the scratch of rd_shift_sums exactly as
its query sizes it and one byte short, every refusal of the side header with nothing written, and the ledger over the side header:
an entry point cannot arrive there without a case here.

Every case is held to a torch restatement of what needs no care about rounding: the member count of the sums; where the resampler
writes the fill, and its values to 1e-12.  tests/test_coreg_gpu.py has the rest."""
import os
import re

import pytest
import torch

import test_memory_contract_gpu as T
from test_memory_contract_gpu import F32, F64, U8

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
NODATA, FILL = -9999.0, -5.0


def test_the_borrowed_helpers_are_there():
    from arena import Arena, nbytes_of                 # noqa: F401
    for name in ("_case", "_full", "_run_case", "_randint", "F32", "F64", "U8", "DEV"):
        assert hasattr(T, name), name
    for name in ("inp", "out", "ws", "call", "ref"):
        assert hasattr(T.K, name), name


def _heights(rows, cols, salt):
    def make():
        n = rows * cols
        z = torch.randn(n, generator=torch.Generator().manual_seed(rows * 131 + cols + salt)) * 5.0 + 300.0
        z[T._randint(3 + salt, 20, n) == 0] = NODATA
        return z
    return make


def c_shift_sums(k, rows, cols, src_f64, ref_f64, need):
    n = rows * cols
    src = k.inp("src", n, fn=_heights(rows, cols, 0), dtype=F64 if src_f64 else F32)
    ref = k.inp("ref", n, fn=_heights(rows, cols, 7), dtype=F64 if ref_f64 else F32)
    cls = k.inp("cls", n, fn=lambda: T._randint(6, 8, n), dtype=U8) if need else None
    ws, nb = k.ws("ws", k.lib.rd_shift_sums_ws_bytes(rows, cols), short=True)
    out = k.out("sums", 10, F64)
    k.call("rd_shift_sums", src, int(src_f64), ref, int(ref_f64), cls, need, rows, cols, NODATA, 0.5, 0.25, 0.0, 0.0, ws, nb, out,
           refuses_short=True)

    def check():
        want = 0
        if rows >= 3 and cols >= 3:
            bad = (src.view(rows, cols) == NODATA)
            near = torch.nn.functional.max_pool2d(bad[None, None].float(), 3, 1)[0, 0] > 0
            ok = ~near & (ref.view(rows, cols)[1:-1, 1:-1] != NODATA)
            if need:
                ok &= (cls.view(rows, cols)[1:-1, 1:-1].int() & need) == need
            want = int(ok.sum())
        assert int(out[0]) == want, (float(out[0]), want)
        assert bool(torch.isfinite(out).all()) and (want > 0 or not bool(out.any()))
        assert float(out[4]) >= 0 and float(out[6]) >= 0 and float(out[9]) >= 0
    k.ref(check)


def c_translate(k, rows, cols, f64, tx, ty, tz):
    n = rows * cols
    src = k.inp("src", n, fn=_heights(rows, cols, 0), dtype=F64 if f64 else F32)
    moved = k.out("moved", (rows, cols), F64)
    k.call("rd_translate_bilinear", src, int(f64), rows, cols, NODATA, float(tx), float(ty), float(tz), FILL, moved)

    def check():
        s = src.view(rows, cols).double()
        ys = torch.arange(rows, device=s.device, dtype=F64) - ty
        xs = torch.arange(cols, device=s.device, dtype=F64) - tx
        y0, x0 = ys.floor(), xs.floor()
        fy, fx = ys - y0, xs - x0
        oky = (y0 >= 0) & (y0 <= rows - 1 - (fy != 0).double())
        okx = (x0 >= 0) & (x0 <= cols - 1 - (fx != 0).double())
        iy, ix = y0.clamp(0, rows - 1).long(), x0.clamp(0, cols - 1).long()
        iy1, ix1 = (iy + (fy != 0).long()).clamp(max=rows - 1), (ix + (fx != 0).long()).clamp(max=cols - 1)
        tap = lambda a, b: s[a][:, b]
        v00, v01, v10, v11 = tap(iy, ix), tap(iy, ix1), tap(iy1, ix), tap(iy1, ix1)
        undefined = ~(oky[:, None] & okx[None, :]) | (v00 == NODATA) | (v01 == NODATA) | (v10 == NODATA) | (v11 == NODATA)
        assert torch.equal(moved == FILL, undefined)
        top, bot = v00 + fx[None, :] * (v01 - v00), v10 + fx[None, :] * (v11 - v10)
        val = top + fy[:, None] * (bot - top) + tz
        assert torch.allclose(moved[~undefined], val[~undefined], rtol=1e-12, atol=0.0)
    k.ref(check)


CASES = []
# (rows, cols, source f64, reference f64, need): across the 64 x 16 tile in both directions, and rasters with no interior
for s_ in [(3, 3, True, True, 0), (4, 70, False, True, 1), (67, 5, True, False, 0), (130, 97, False, False, 3), (2, 9, True, True, 0),
           (1, 1, False, False, 0), (35, 131, True, True, 4)]:
    CASES.append(T._case(c_shift_sums, s_, ["rd_shift_sums", "rd_shift_sums_ws_bytes"]))
# (rows, cols, f64, tx, ty, tz): sub-pixel shifts in every direction, whole pixels, a shift beyond the raster
for s_ in [(3, 3, True, 0.5, 0.5, 0.0), (4, 70, False, -0.25, 0.75, 1.5), (67, 5, True, 1.0, -2.0, 0.0), (130, 97, False, 2.3, -1.6, -0.5),
           (1, 1, False, 0.0, 0.0, 2.0), (1, 9, True, -0.5, 0.0, 0.0), (9, 1, False, 0.0, 0.5, 0.0), (33, 65, True, 1e300, 0.0, 0.0)]:
    CASES.append(T._case(c_translate, s_, ["rd_translate_bilinear"], short=False))


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
GOOD = {
    "sums": dict(src=1, ref=1, cls=1, ws=1, out=1, rows=ROWS, cols=COLS, need=1, gsd_x=0.5, gsd_y=0.5, thr=0.0, slope_max=0.0,
                 ws_short=0),
    "translate": dict(src=1, out=1, rows=ROWS, cols=COLS, tx=0.5, ty=-0.25, tz=1.0, alias=0),
}
BAD = {
    "sums": {
        "null src": dict(src=0), "null ref": dict(ref=0), "null ws": dict(ws=0), "null out": dict(out=0),
        "null cls with need 1": dict(cls=0), "no rows": dict(rows=0), "negative cols": dict(cols=-3),
        "too many tiles": dict(rows=2000000000, cols=2000000000),        # refused before anything is read
        "gsd_x 0": dict(gsd_x=0.0), "gsd_y negative": dict(gsd_y=-0.5), "gsd_x NaN": dict(gsd_x=NAN), "gsd_y Inf": dict(gsd_y=INF),
        "negative thr": dict(thr=-1.0), "thr NaN": dict(thr=NAN), "thr Inf": dict(thr=INF), "negative slope_max": dict(slope_max=-0.1),
        "slope_max NaN": dict(slope_max=NAN), "slope_max Inf": dict(slope_max=INF), "need -1": dict(need=-1), "need 256": dict(need=256),
        "ws one byte short": dict(ws_short=1), "no ws bytes": dict(ws_short=160),
    },
    "translate": {
        "null src": dict(src=0), "null out": dict(out=0), "out is src": dict(alias=1), "no rows": dict(rows=0), "no cols": dict(cols=0),
        "negative rows": dict(rows=-1), "tx NaN": dict(tx=NAN), "tx Inf": dict(tx=INF), "ty -Inf": dict(ty=-INF), "ty NaN": dict(ty=NAN),
        "tz Inf": dict(tz=INF), "tz NaN": dict(tz=NAN),
    },
}
REFUSALS = [(form, what, spec) for form in ("sums", "translate") for what, spec in BAD[form].items()]


def _refusal(lib, form, spec):
    from arena import Arena, nbytes_of
    a = dict(GOOD[form], **spec)
    n = ROWS * COLS
    ar = Arena(T.DEV, [nbytes_of((n,), F64), nbytes_of((n,), F64), nbytes_of((n,), U8), nbytes_of((64,), F64), nbytes_of((n,), F64)])
    val = ar.alloc((n,), F64, fill=torch.randn(n, dtype=F64), kind="input", name="src")
    ref = ar.alloc((n,), F64, fill=torch.randn(n, dtype=F64), kind="input", name="ref")
    cls = ar.alloc((n,), U8, fill=torch.ones(n, dtype=U8), kind="input", name="cls")
    ws = ar.alloc((64,), F64, fill="sentinel", kind="scratch", name="ws")
    out = ar.alloc((n,), F64, fill="sentinel", kind="output", name="out")
    p = lambda flag, t: t.data_ptr() if flag else None
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    snap = ar.snapshot()
    if form == "sums":
        nb = lib.rd_shift_sums_ws_bytes(ROWS, COLS)
        assert nb == 160                                # 21 x 30: two tiles, one above the other
        rc = lib.rd_shift_sums(p(a["src"], val), 1, p(a["ref"], ref), 1, p(a["cls"], cls), a["need"], a["rows"], a["cols"], NODATA,
                               a["gsd_x"], a["gsd_y"], a["thr"], a["slope_max"], p(a["ws"], ws), nb - a["ws_short"], p(a["out"], out),
                               stream)
    else:
        rc = lib.rd_translate_bilinear(p(a["src"], val), 1, a["rows"], a["cols"], NODATA, a["tx"], a["ty"], a["tz"], FILL,
                                       p(a["src"], val) if a["alias"] else p(a["out"], out), stream)
    msg = lib.rd_last_error_string()
    torch.cuda.synchronize()
    assert ar.same_as(snap), "the refused call changed memory"
    ar.check()
    return rc, msg


@pytest.mark.parametrize("form,what,spec", [pytest.param(f, w, s, id=f"{f}-{w.replace(' ', '_')}") for f, w, s in REFUSALS])
def test_refusals_write_nothing(lib, form, what, spec):
    rc, msg = _refusal(lib, form, spec)
    assert rc == 1 and msg, (what, rc, msg)


@pytest.mark.parametrize("form,spec", [("sums", {}), ("sums", dict(cls=0, need=0)), ("translate", {})],
                         ids=["sums", "sums_without_classes", "translate"])
def test_the_refusal_driver_accepts_what_is_right(lib, form, spec):
    """the same driver with nothing wrong: the call goes through and writes -- the refusals above are refusals of their one defect"""
    with pytest.raises(AssertionError, match="changed memory"):
        _refusal(lib, form, spec)


def ledger_check():
    """every function of the side header is bound, exported and covered"""
    from resdepth_amd import _lib
    text = open(os.path.join(ROOT, "include", "resdepth_hip_coreg.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    exported = set(re.findall(r"\b(rd_\w+)\s*\(", text))
    assert exported == set(_lib.SIGNATURES_COREG), exported ^ set(_lib.SIGNATURES_COREG)
    lib = _lib.load()
    for name in exported:
        assert hasattr(lib, name), name
    covered = {f for c in CASES for f in c["covers"]}
    assert covered == exported, covered ^ exported


def test_every_function_of_the_side_header_has_a_case():
    ledger_check()
