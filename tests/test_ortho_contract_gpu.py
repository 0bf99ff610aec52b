"""The memory contract of include/resdepth_hip.h for the entry point of include/resdepth_hip_ortho.h: the guard-band cases that
tests/test_memory_contract_gpu.py runs for every entry point of the main header (its driver and judgement are used as they are,
as tests/test_coreg_contract_gpu.py does; the arena is tests/arena.py) at ragged shapes, with each nullable output present and
absent, every refusal of the side header with nothing written, and the ledger over the side header: an entry point cannot arrive
there without a case here.

The images, the DSM and the descriptor table are inputs inside guard bands; the descriptors hold the arena addresses of the images
of that run.  A case with coords is held to the numpy oracle as tests/test_ortho_gpu.py holds the front end (coords within 1e-6 px,
valid equal and out within 2^-23 sum |w v| of the oracle's resampler at the kernel's own coords); a case without them to `fill`
exactly where valid is 0."""
import os
import re

import numpy as np
import pytest
import torch

import ortho_ref as R
import test_memory_contract_gpu as T
import test_ortho_gpu as G
from test_memory_contract_gpu import F32, F64, U8

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
NODATA, FILL = -9999.0, -5.0
I16 = torch.int16                                        # the bytes of a uint16 image
# (rows, cols, pitch, arena dtype, numpy dtype, RD_ORTHO_* id, image_nodata)
IMAGES = [(40, 33, 33, U8, np.uint8, 0, NAN), (25, 50, 50, I16, np.uint16, 1, 0.0), (31, 29, 37, F32, np.float32, 2, NAN)]
KIND_IDS = {"nearest": 0, "bilinear": 1, "bicubic": 2}


def test_the_borrowed_helpers_are_there():
    from arena import Arena, nbytes_of                 # noqa: F401
    for name in ("_case", "_full", "_run_case", "_randint", "F32", "F64", "U8", "DEV"):
        assert hasattr(T, name), name
    for name in ("inp", "out", "call", "ref"):
        assert hasattr(T.K, name), name
    for name in ("GRIDS", "_models", "_gt4", "_dsm"):
        assert hasattr(G, name), name


def _image_values(i):
    rows, cols, pitch, _, npdt, _, _ = IMAGES[i]
    rng = np.random.default_rng(40 + i)
    if npdt == np.float32:
        a = rng.normal(50.0, 20.0, (rows, pitch)).astype(np.float32)
    else:
        a = rng.integers(0 if npdt == np.uint16 else 1, 200, (rows, pitch)).astype(npdt)      # the uint16 image has nodata zeros
    return a


def _pack(models, imgs, n_views):
    from resdepth_amd import ortho
    desc = np.zeros(n_views, dtype=ortho._VIEW_DESC)
    for v in range(n_views):
        i = v % len(IMAGES)
        rows, cols, pitch, _, _, dt, nd = IMAGES[i]
        d = desc[v]
        d["image"], d["pitch"], d["rows"], d["cols"], d["dtype"] = imgs[i].data_ptr(), pitch, rows, cols, dt
        d["line0"], d["samp0"], d["image_nodata"] = 0.5 * (v // 3), 0.25 * (v // 3), nd
        for name in R.SCALARS + R.VECTORS:
            d[name] = models[i][name]
    return torch.from_numpy(desc.view(np.uint8).reshape(-1).copy())


def c_ortho(k, rows, cols, grid_name, kind, n_views, with_valid, with_coords):
    g = G.GRIDS[grid_name]
    models = G._models(g, rows, cols, [(r, c) for r, c, *_ in IMAGES])
    imgs = []
    for i, (r, c, pitch, dt, npdt, _, _) in enumerate(IMAGES):
        a = _image_values(i)
        imgs.append(k.inp(f"img{i}", r * pitch, fn=lambda a=a, npdt=npdt: torch.from_numpy(a.view(np.int16) if npdt == np.uint16 else a),
                          dtype=dt))
    dsm_np = G._dsm(rows, cols, seed=rows + cols)
    dsm = k.inp("dsm", rows * cols, fn=lambda: torch.from_numpy(dsm_np))
    views = k.inp("views", n_views * 776, fn=lambda: _pack(models, imgs, n_views), dtype=U8)
    out = k.out("out", (n_views, rows, cols), F32)
    valid = k.out("valid", (n_views, rows, cols), U8) if with_valid else None
    coords = k.out("coords", (n_views, rows, cols, 2), F64) if with_coords else None
    gt = g["gt"]
    k.call("rd_ortho_rpc", dsm, rows, cols, gt[0], gt[1], gt[3], gt[5], 0 if g["crs"] == "geographic" else 1, g["lon0"], g["fn"],
           NODATA, 1.5, views, n_views, KIND_IDS[kind], FILL, out, valid, coords)

    def check():
        o = out.cpu().numpy()
        if valid is not None:
            va = valid.cpu().numpy()
            assert set(np.unique(va)) <= {0, 1}
            assert (o[va == 0] == np.float32(FILL)).all()
        if coords is None:
            return
        co = coords.cpu().numpy()
        origins = [(0.5 * (v // 3), 0.25 * (v // 3)) for v in range(n_views)]
        want, defined = R.coords(dsm_np, NODATA, G._gt4(gt), "geographic" if g["crs"] == "geographic" else "utm", g["lon0"], g["fn"],
                                 1.5, [models[v % 3] for v in range(n_views)], origins)
        assert (np.isnan(co) == np.isnan(want)).all()
        if defined.any():
            assert float(np.nanmax(np.abs(co - want))) <= 1e-6
        for v in range(n_views):
            r, c, pitch, _, _, _, nd = IMAGES[v % 3]
            img = _image_values(v % 3)[:, :c]
            val, ok, mag = R.resample(img, None if nd != nd else nd, co[v, ..., 0], co[v, ..., 1], kind)
            if valid is not None:
                assert (va[v].astype(bool) == ok).all()
            assert (o[v][~ok] == np.float32(FILL)).all()
            assert (np.abs(o[v].astype(np.float64) - val)[ok] <= (2.0 ** -23 * mag)[ok]).all()
    k.ref(check)


CASES = []
# (rows, cols, grid, resampling, views, valid, coords): across every footprint in both directions, single rows and columns,
# each nullable output present and absent, and the most views
for s_ in [(1, 1, "geographic", "bilinear", 1, True, True), (3, 67, "utm", "nearest", 2, False, False),
           (70, 5, "geographic", "bicubic", 3, True, False), (9, 130, "utm", "bilinear", 3, False, True),
           (1, 257, "utm_south", "bicubic", 2, True, True), (131, 1, "geographic", "nearest", 1, True, True),
           (33, 65, "utm", "bicubic", 16, True, True), (17, 19, "geographic", "bilinear", 4, False, False)]:
    CASES.append(T._case(c_ortho, s_, ["rd_ortho_rpc"], short=False))


@pytest.fixture()
def lib():
    from resdepth_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("case", [pytest.param(c, id=c["id"]) for c in CASES])
def test_memory_contract(lib, case):
    T._full(lib, case)


# ---- the refusals of the side header: RD_ERR_ARG (1), a message, nothing written -------------------------------------------------
ROWS, COLS = 21, 30
GOOD = dict(dsm=1, views=1, out=1, valid=1, coords=1, rows=ROWS, cols=COLS, dx=1e-5, dy=-1e-5, crs=0, lon0=9.0, hoff=0.0, n_views=3,
            resampling=1)
BAD = {
    "null dsm": dict(dsm=0), "null views": dict(views=0), "null out": dict(out=0), "no rows": dict(rows=0), "negative cols": dict(cols=-3),
    "2^31 pixels": dict(rows=65536, cols=32768),                     # refused before anything is read
    "more than 2^31 pixels": dict(rows=2000000000, cols=2000000000),
    "no views": dict(n_views=0), "negative views": dict(n_views=-1), "17 views": dict(n_views=17),
    "dx 0": dict(dx=0.0), "dx NaN": dict(dx=NAN), "dx Inf": dict(dx=INF), "dy 0": dict(dy=0.0), "dy NaN": dict(dy=NAN),
    "dy -Inf": dict(dy=-INF), "crs 2": dict(crs=2), "crs -1": dict(crs=-1), "resampling 3": dict(resampling=3),
    "resampling -1": dict(resampling=-1), "lon0 NaN": dict(lon0=NAN), "lon0 Inf": dict(lon0=INF), "height_offset NaN": dict(hoff=NAN),
    "height_offset -Inf": dict(hoff=-INF),
}


def _refusal(lib, spec):
    from arena import Arena, nbytes_of
    a = dict(GOOD, **spec)
    n = ROWS * COLS
    r, c, pitch = IMAGES[0][:3]
    ar = Arena(T.DEV, [nbytes_of((n,), F32), nbytes_of((r * pitch,), U8), 3 * 776, nbytes_of((3 * n,), F32), 3 * n,
                       nbytes_of((6 * n,), F64)])
    dsm = ar.alloc((n,), F32, fill=torch.full((n,), 400.0), kind="input", name="dsm")
    img = ar.alloc((r * pitch,), U8, fill=torch.from_numpy(_image_values(0)).reshape(-1), kind="input", name="img")
    models = G._models(G.GRIDS["geographic"], ROWS, COLS, [(r, c)] * 3)
    from resdepth_amd import ortho
    desc = np.zeros(3, dtype=ortho._VIEW_DESC)
    for v in range(3):
        desc[v]["image"], desc[v]["pitch"], desc[v]["rows"], desc[v]["cols"], desc[v]["dtype"] = img.data_ptr(), pitch, r, c, 0
        desc[v]["image_nodata"] = NAN
        for name in R.SCALARS + R.VECTORS:
            desc[v][name] = models[v][name]
    views = ar.alloc((3 * 776,), U8, fill=torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()), kind="input", name="views")
    out = ar.alloc((3 * n,), F32, fill="sentinel", kind="output", name="out")
    valid = ar.alloc((3 * n,), U8, fill="sentinel", kind="output", name="valid")
    coords = ar.alloc((6 * n,), F64, fill="sentinel", kind="output", name="coords")
    p = lambda flag, t: t.data_ptr() if flag else None
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    snap = ar.snapshot()
    gt = G.GRIDS["geographic"]["gt"]
    rc = lib.rd_ortho_rpc(p(a["dsm"], dsm), a["rows"], a["cols"], gt[0], a["dx"], gt[3], a["dy"], a["crs"], a["lon0"], 0.0, NODATA,
                          a["hoff"], p(a["views"], views), a["n_views"], a["resampling"], FILL, p(a["out"], out), p(a["valid"], valid),
                          p(a["coords"], coords), stream)
    msg = lib.rd_last_error_string()
    torch.cuda.synchronize()
    assert ar.same_as(snap), "the refused call changed memory"
    ar.check()
    return rc, msg


@pytest.mark.parametrize("what,spec", [pytest.param(w, s, id=w.replace(" ", "_")) for w, s in BAD.items()])
def test_refusals_write_nothing(lib, what, spec):
    rc, msg = _refusal(lib, spec)
    assert rc == 1 and msg, (what, rc, msg)


@pytest.mark.parametrize("spec", [{}, dict(valid=0), dict(coords=0), dict(valid=0, coords=0), dict(crs=1), dict(resampling=2)],
                         ids=["all", "no_valid", "no_coords", "out_alone", "utm", "bicubic"])
def test_the_refusal_driver_accepts_what_is_right(lib, spec):
    """the same driver with nothing wrong: the call goes through and writes -- the refusals above are refusals of their one defect"""
    with pytest.raises(AssertionError, match="changed memory"):
        _refusal(lib, spec)


def ledger_check():
    """every function of the side header is bound, exported and covered"""
    from resdepth_amd import _lib
    text = open(os.path.join(ROOT, "include", "resdepth_hip_ortho.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    exported = set(re.findall(r"\b(rd_\w+)\s*\(", text))
    assert exported == set(_lib.SIGNATURES_ORTHO), exported ^ set(_lib.SIGNATURES_ORTHO)
    lib = _lib.load()
    for name in exported:
        assert hasattr(lib, name), name
    covered = {f for c in CASES for f in c["covers"]}
    assert covered == exported, covered ^ exported


def test_every_function_of_the_side_header_has_a_case():
    ledger_check()
