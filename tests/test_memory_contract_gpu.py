"""Where the kernels read and write: the memory contract of include/resdepth_hip.h on ragged shapes (-m gpu).

Every case calls the C ABI directly (not resdepth_amd.ops) with every pointer inside a guard-band arena (tests/arena.py) and
with ws_bytes / part_floats / the wpartial row count EXACTLY as the matching query returns them.  Per case:
  1. guards intact, inputs untouched (magnitude slots: only words 0 and 1 of each 128-byte line may change);
  2. no sentinel left in any output (packed weight buffers are opaque: they are judged through the convolutions that read them);
  3. outputs bit-identical across three runs: outputs + scratch pre-filled with the sentinel / with 0xFF / with zeros at other
     arena offsets (shifted by 256 bytes plus an odd multiple of 16 bytes; slots stay 128-byte aligned);
  4. outputs bit-identical to the resdepth_amd.ops wrapper on the same inputs, same arithmetic mode, same slots armed -- the path
     the other test files tie to fp64 references; entry points without a wrapper get a direct reference of their own;
  5. with one byte (float) less scratch than the query says: RD_ERR_WS / RD_ERR_ARG, a message, and an unchanged arena.
The ledger test parses the header: every exported function is in the case table or in EXEMPT (no device pointer written).
"""
import ctypes as C
import os
import re
import struct
import sys
import zlib

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from arena import Arena, ArenaError, nbytes_of  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32, F64, U8, I32, I64 = torch.float32, torch.float64, torch.uint8, torch.int32, torch.int64
SLOT_BYTES = 2048
NOSTREAM = {"rd_quant_next", "rd_quant_next_img"}


class _Stop(Exception):
    """the undersized-scratch call was made and judged: the rest of the case does not run"""


class _P:
    """placeholder for a tensor while a case is only being sized"""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = tuple(shape), dtype

    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n


def _shape(s):
    return (s,) if isinstance(s, int) else tuple(s)


def _rand(seed, *shape):
    """seeded uniform [0, 1) on the host: every run of a case sees the same inputs"""
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def _randint(seed, high, *shape):
    return torch.randint(0, high, shape, generator=torch.Generator().manual_seed(seed))


class _Recording:
    """the ctypes handle, remembering which entry points a case really reached"""

    def __init__(self, lib, called):
        self._lib, self._called = lib, called

    def __getattr__(self, name):
        self._called.add(name)
        return getattr(self._lib, name)


class K:
    """One pass over a case.  plan=True only records allocation sizes; otherwise allocations come from an Arena sized by the plan.
    fill: what outputs and scratch hold before the call; shifted: allocations start 256 + an odd multiple of 16 bytes later;
    short: the flagged scratch is one unit smaller than its query says and the flagged call must refuse it."""

    def __init__(self, lib, sizes=None, fill="sentinel", shifted=False, short=False, with_wrapper=False):
        from resdepth_amd import _lib
        self.called = set()
        self.lib, self._lib = _Recording(lib, self.called), _lib
        self.plan = sizes is None
        self.sizes = []
        self.fill, self.shifted, self.short, self.with_wrapper = fill, shifted, short, with_wrapper
        self.arena = None if self.plan else Arena(DEV, sizes)
        self.three = self.lib.rd_mfma_products() == 3 and not _lib.tune_get("mfma_f32")
        assert self.three == (_lib.products() == 3)
        self.split = not _lib.tune_get("mfma_f32")
        self.outs, self.limit, self.slots, self.initial = {}, {}, [], {}
        self.wrappers, self.refs, self.short_seen = [], [], False
        self.stream = None if self.plan else torch.cuda.current_stream().cuda_stream
        self._i = 0

    # ---- allocations -------------------------------------------------------------------------------------------------
    def _alloc(self, name, shape, dtype, fill, kind, slot=False):
        shape = _shape(shape)
        if self.plan:
            self.sizes.append(nbytes_of(shape, dtype))
            return _P(shape, dtype)
        shift = 0
        if self.shifted:
            shift = 384 if slot else 256 + 16 * (2 * (self._i % 4) + 1)
        self._i += 1
        return self.arena.alloc(shape, dtype, fill=fill, kind=kind, name=name, shift=shift)

    def _data(self, name, shape, dtype, fn, scale):
        if fn is not None:
            t = fn() if callable(fn) else fn
            return t.to(device=DEV, dtype=dtype).reshape(shape)
        g = torch.Generator(device=DEV).manual_seed(zlib.crc32(name.encode()))
        if dtype in (F32, F64):
            return (torch.randn(shape, generator=g, device=DEV, dtype=F32) * scale).to(dtype)
        return torch.randint(0, 2, shape, generator=g, device=DEV).to(dtype)

    def inp(self, name, shape, fn=None, dtype=F32, scale=1.0):
        """an input: seeded normal values (x scale), or fn() -> tensor (only evaluated when the case really runs)"""
        shape = _shape(shape)
        return self._alloc(name, shape, dtype, None if self.plan else self._data(name, shape, dtype, fn, scale), "input")

    def pos(self, name, shape):
        """positive values in [0.5, 1.5) (invstd, gamma, std)"""
        shape = _shape(shape)
        g = None if self.plan else torch.Generator(device=DEV).manual_seed(zlib.crc32(name.encode()))
        return self.inp(name, shape, None if self.plan else (lambda: torch.rand(shape, generator=g, device=DEV) + 0.5))

    def out(self, name, shape, dtype=F32, fill=None):
        t = self._alloc(name, shape, dtype, fill if fill is not None else self.fill, "output")
        self.outs[name] = t
        return t

    def inout(self, name, shape, fn=None, dtype=F32, scale=1.0):
        """updated in place: holds data before the call, compared like an output after it"""
        shape = _shape(shape)
        d = None if self.plan else self._data(name, shape, dtype, fn, scale)
        t = self._alloc(name, shape, dtype, d, "output")
        if not self.plan:
            self.initial[name] = d.clone()
        self.outs[name] = t
        return t

    def opaque(self, name, nbytes):
        """a packed weight buffer of exactly `nbytes`: guards only (which of its regions are written depends on the mode)"""
        return self._alloc(name, nbytes, U8, self.fill, "scratch")

    def packed(self, name, rows, taps, cin):
        return self.opaque(name, self.lib.rd_packed_weight_bytes(rows, taps, cin))

    def ws(self, name, nbytes, short=False):
        """scratch of exactly the queried size -> (tensor, ws_bytes to pass)"""
        nbytes = int(nbytes)
        if short:
            assert nbytes > 0, f"{name}: the query returned 0 bytes"
            self.short_seen = True
        t = self._alloc(name, max(nbytes, 16), U8, self.fill, "scratch")
        return t, (nbytes - 1 if (short and self.short) else nbytes)

    def part(self, name, nfloats, short=False):
        """BN-backward partial rows of exactly the queried float count -> (tensor, part_floats to pass)"""
        nfloats = int(nfloats)
        if short:
            assert nfloats > 0
            self.short_seen = True
        t = self.out(name, max(nfloats, 4))
        self.limit[name] = 0
        return t, (nfloats - 1 if (short and self.short) else nfloats)

    def slot(self, name):
        """a zeroed magnitude slot (the contract: zeroed by the caller, 128-byte aligned)"""
        t = self._alloc(name, SLOT_BYTES // 4, I32, "zero", "output", slot=True)
        if not self.plan:
            self.slots.append((name, t))
        self.outs[name] = t
        return t

    # ---- calls -------------------------------------------------------------------------------------------------------
    def call(self, fname, *args, refuses_short=False):
        if self.plan:
            return 0
        a = [x.data_ptr() if isinstance(x, torch.Tensor) else x for x in args]
        if fname not in NOSTREAM:
            a.append(self.stream)
        fn = getattr(self.lib, fname)
        if self.short and refuses_short:
            torch.cuda.synchronize()
            snap = self.arena.snapshot()
            rc = fn(*a)
            msg = self.lib.rd_last_error_string()
            torch.cuda.synchronize()
            assert rc in (1, 2), f"{fname}: undersized scratch accepted (rc {rc})"
            assert msg, f"{fname}: no error string"
            assert self.arena.same_as(snap), f"{fname}: the refused call changed memory"
            raise _Stop()
        rc = fn(*a)
        assert rc == 0, f"{fname} failed (rc {rc}): {self.lib.rd_last_error_string()}"
        return rc

    def tag(self, name, x):
        """rd_amax of an operand into a slot of its own (three-product mode only, like ops.amax_of)"""
        if not self.three:
            return None
        s = self.slot(name + "_amax")
        self.call("rd_amax", x, x.numel(), s)
        return s

    def quant(self, a=None, b=None, out=None, out2=None):
        if self.three and any(t is not None for t in (a, b, out, out2)):
            self.call("rd_quant_next", a, b, out, out2)

    def rows(self):
        return C.c_int(-1)

    def wrapper(self, fn):
        """fn() -> {output name: tensor the ops wrapper returned}; run once, compared bit for bit"""
        self.wrappers.append(fn)

    def ref(self, fn):
        """fn() asserts something about the outputs of entry points that have no wrapper"""
        self.refs.append(fn)

    def first(self, name):
        return None if self.plan else self.initial[name].clone()

    # ---- judgement ---------------------------------------------------------------------------------------------------
    def finish(self):
        """assertions 1 and 2 (+ 4 when asked) -> {output name: bytes}"""
        ar = self.arena
        ar.check()
        got = {}
        for name, t in self.outs.items():
            lim = self.limit.get(name)
            flat = t.reshape(-1) if lim is None else t.reshape(-1)[:lim]
            if name not in self.initial and not any(name == s for s, _ in self.slots):
                if lim is None:
                    assert ar.unwritten(t) == 0, f"output {name!r}: {ar.unwritten(t)} elements never written"
                elif lim:
                    hole = int((flat.view(I32) == 0x7FFBADED).sum()) if self.fill == "sentinel" else 0
                    assert hole == 0, f"output {name!r}: {hole} of the first {lim} elements never written"
            got[name] = flat.clone().view(U8) if flat.numel() else flat.clone()
        for name, s in self.slots:
            w = s.view(16, 32)
            assert int((w[:, 2:] != 0).sum()) == 0, f"slot {name!r}: words beyond 0 and 1 of a 128-byte line changed"
        if self.with_wrapper:
            for fn in self.wrappers:
                for name, t in fn().items():
                    lim = self.limit.get(name)
                    a = self.outs[name].reshape(-1)
                    b = t.reshape(-1)
                    if lim is not None:
                        a, b = a[:lim], b[:lim]
                    assert a.dtype == b.dtype and a.numel() == b.numel(), (name, a.dtype, b.dtype, a.numel(), b.numel())
                    assert torch.equal(a.view(U8), b.contiguous().view(U8)), f"{name}: C ABI result differs from the ops wrapper"
            for fn in self.refs:
                fn()
            torch.cuda.synchronize()
            ar.check()                      # the wrappers read the arena's inputs: they must not have written either
        return got


# ---- helpers shared by the cases --------------------------------------------------------------------------------------------
def _bn(k, name, c):
    """mean, invstd, gamma, beta of a BatchNorm with c channels"""
    return (k.inp(name + "_mean", c, scale=0.1), k.pos(name + "_invstd", c), k.pos(name + "_gamma", c),
            k.inp(name + "_beta", c, scale=0.1))


def _pack3(k, wt, cout, cin, dgrad=True):
    wf = k.packed("wf", cout, 9, cin)
    wd = k.packed("wd", cin, 9, cout) if dgrad else None
    sw = k.slot("w_amax") if k.three else None
    k.quant(out2=sw)
    k.call("rd_pack_conv3x3_weight", wt, wf, wd, cout, cin)
    return wf, wd, sw


def _packt(k, wt, cin, cout):
    wtf = k.packed("wtf", 4 * cout, 1, cin)
    wtd = k.packed("wtd", cin, 4, cout)
    sw = k.slot("w_amax") if k.three else None
    k.quant(out2=sw)
    k.call("rd_pack_convt2x2_weight", wt, wtf, wtd, cin, cout)
    return wtf, wtd, sw


def _ops():
    from resdepth_amd import ops
    return ops


def _lim_part(k, name, rows, c):
    if not k.plan:
        assert rows.value >= 0
        k.limit[name] = rows.value * 4 * c


# ---- the GEMM families ------------------------------------------------------------------------------------------------------
def c_conv3x3(k, n, h, w, cin, cout):
    lib, ops = k.lib, _ops()
    x, wt, dz = k.inp("x", (n, h, w, cin)), k.inp("w", (cout, cin, 3, 3), scale=0.1), k.inp("dz", (n, h, w, cout))
    wf, wd, sw = _pack3(k, wt, cout, cin)
    sx, sdz = k.tag("x", x), k.tag("dz", dz)
    z = k.out("z", (n, h, w, cout))
    k.quant(sx, sw)
    k.call("rd_conv3x3_fwd", x, wf, z, n, h, w, cin, cout)
    dx = k.out("dx", (n, h, w, cin))
    k.quant(sdz, sw)
    k.call("rd_conv3x3_bwd_data", dz, wd, dx, n, h, w, cin, cout)
    dw = k.out("dw", (cout, cin, 3, 3))
    ws, nb = k.ws("ws", lib.rd_conv3x3_bwd_weight_ws_bytes(n, h, w, cin, cout), short=True)
    k.quant(sdz, sx)
    k.call("rd_conv3x3_bwd_weight", x, dz, dw, n, h, w, cin, cout, ws, nb, refuses_short=True)

    def wrap():
        pf, pd = ops.pack_conv3x3_weight(wt)
        ops.amax_of(x), ops.amax_of(dz)
        return {"z": ops.conv3x3_fwd(x, pf), "dx": ops.conv3x3_bwd_data(dz, pd), "dw": ops.conv3x3_bwd_weight(x, dz)}
    k.wrapper(wrap)


def c_conv3x3_stats(k, n, h, w, cin, cout):
    lib, ops = k.lib, _ops()
    x, wt = k.inp("x", (n, h, w, cin)), k.inp("w", (cout, cin, 3, 3), scale=0.1)
    wf, _, sw = _pack3(k, wt, cout, cin, dgrad=False)
    sx = k.tag("x", x)
    z, sums = k.out("z", (n, h, w, cout)), k.out("sums", 2 * cout, F64)
    ws, nb = k.ws("ws", lib.rd_conv3x3_fwd_stats_ws_bytes(n, h, w, cin, cout), short=True)
    k.quant(sx, sw)
    k.call("rd_conv3x3_fwd_stats", x, wf, z, sums, n, h, w, cin, cout, ws, nb, refuses_short=True)

    def wrap():
        pf, _ = ops.pack_conv3x3_weight(wt, need_dgrad=False)
        ops.amax_of(x)
        zz, ss = ops.conv3x3_fwd_stats(x, pf)
        return {"z": zz, "sums": ss}
    k.wrapper(wrap)


def c_conv3x3_bn(k, n, h, w, cin, cout):
    lib, ops = k.lib, _ops()
    x, wt = k.inp("x", (n, h, w, cin)), k.inp("w", (cout, cin, 3, 3), scale=0.1)
    wf, _, sw = _pack3(k, wt, cout, cin, dgrad=False)
    sx = k.tag("x", x)
    z, mean, invstd = k.out("z", (n, h, w, cout)), k.out("mean", cout), k.out("invstd", cout)
    rm, rv = k.inout("rm", cout, scale=0.1), k.inout("rv", cout, fn=lambda: _rand(1, cout) + 0.5)
    nbt = k.inout("nbt", 1, fn=lambda: torch.tensor([7]), dtype=I64)
    ws, nb = k.ws("ws", lib.rd_conv3x3_fwd_stats_ws_bytes(n, h, w, cin, cout), short=True)
    k.quant(sx, sw)
    k.call("rd_conv3x3_fwd_bn", x, wf, z, float(n * h * w), 1e-5, 0.1, mean, invstd, rm, rv, nbt, n, h, w, cin, cout, ws, nb,
           refuses_short=True)

    def wrap():
        pf, _ = ops.pack_conv3x3_weight(wt, need_dgrad=False)
        ops.amax_of(x)
        a, b, c = k.first("rm"), k.first("rv"), k.first("nbt")
        zz, m, i = ops.conv3x3_fwd_bn(x, pf, a, b, c)
        return {"z": zz, "mean": m, "invstd": i, "rm": a, "rv": b, "nbt": c}
    k.wrapper(wrap)


def c_conv3x3_act(k, n, h, w, cin, cout):
    """inference: folded pack + convolution with shift, activation and (where the shape allows) the pooled output"""
    ops = _ops()
    pool = w % 16 == 0 and h % 8 == 0
    x, wt = k.inp("x", (n, h, w, cin)), k.inp("w", (cout, cin, 3, 3), scale=0.1)
    scale, shift = k.pos("row_scale", cout), k.inp("shift", cout, scale=0.1)
    wf = k.packed("wf", cout, 9, cin)
    sw = k.slot("w_amax") if k.three else None
    k.quant(out2=sw)
    k.call("rd_pack_conv3x3_weight_folded", wt, scale, wf, cout, cin)
    sx = k.tag("x", x)
    a = k.out("a", (n, h, w, cout))
    pooled = k.out("pooled", (n, h // 2, w // 2, cout)) if pool else None
    k.quant(sx, sw)
    k.call("rd_conv3x3_fwd_act", x, wf, shift, 0.01, a, pooled, n, h, w, cin, cout)

    def wrap():
        pf = ops.pack_conv3x3_weight_folded(wt, scale)
        ops.amax_of(x)
        aa, pp = ops.conv3x3_fwd_act(x, pf, shift, 0.01, pool=pool)
        return {"a": aa, "pooled": pp} if pool else {"a": aa}
    k.wrapper(wrap)


def c_conv3x3_dgrad_bnstats(k, n, h, w, cin, cout, mode=1):
    lib, ops = k.lib, _ops()
    dz, wt = k.inp("dz", (n, h, w, cout)), k.inp("w", (cout, cin, 3, 3), scale=0.1)
    bz = k.inp("bn_z", (n, h, w, cin))
    mean, invstd, gamma, beta = _bn(k, "bn", cin)
    _, wd, sw = _pack3(k, wt, cout, cin)
    sdz = k.tag("dz", dz)
    dx = k.out("dx", (n, h, w, cin))
    part, pf = k.part("part", lib.rd_bn_bwd_part_floats(n * h * w, cin), short=True)
    rows = k.rows()
    k.quant(sdz, sw)
    k.call("rd_conv3x3_bwd_data_bnstats", dz, wd, dx, n, h, w, cin, cout, bz, mean, invstd, gamma, beta, 0.01, None, mode, part, pf,
           C.byref(rows), refuses_short=True)
    _lim_part(k, "part", rows, cin)
    fin = not k.plan and rows.value > 0
    if k.plan or fin:
        sums, dg, db, de = k.out("sums", 4 * cin, F64), k.out("dgamma", cin), k.out("dbeta", cin), k.out("dextra", cin)
        k.call("rd_bn_bwd_stats_finalize", part, rows.value, None, 0, cin, sums, dg, db, de)
    if not k.plan:
        assert rows.value * 4 * cin <= lib.rd_bn_bwd_part_floats(n * h * w, cin), "rows_out exceeds rd_bn_bwd_part_floats"

    def wrap():
        _, pd = ops.pack_conv3x3_weight(wt)
        ops.amax_of(dz)
        hook = ops.BnHook(bz, mean, invstd, gamma, beta, 0.01, mode=mode)
        dxx, (pp, rr) = ops.conv3x3_bwd_data(dz, pd, bn=hook)
        assert rr == rows.value
        res = {"dx": dxx, "part": pp}
        if fin:
            g, b, e = (torch.empty(cin, device=DEV) for _ in range(3))
            res.update(sums=ops.bn_bwd_stats_finalize([(pp, rr)], cin, g, b, e), dgamma=g, dbeta=b, dextra=e)
        return res
    k.wrapper(wrap)


def c_convt(k, n, h, w, cin, cout):
    lib, ops = k.lib, _ops()
    x, wt, bias = k.inp("x", (n, h, w, cin)), k.inp("w", (cin, cout, 2, 2), scale=0.1), k.inp("bias", cout, scale=0.1)
    skip, dout = k.inp("skip", (n, 2 * h, 2 * w, cout)), k.inp("dout", (n, 2 * h, 2 * w, cout))
    wtf, wtd, sw = _packt(k, wt, cin, cout)
    sx, sdo = k.tag("x", x), k.tag("dout", dout)
    out = k.out("out", (n, 2 * h, 2 * w, cout))
    k.quant(sx, sw)
    k.call("rd_convt2x2_fwd", x, wtf, bias, skip, out, n, h, w, cin, cout)
    dx = k.out("dx", (n, h, w, cin))
    k.quant(sdo, sw)
    k.call("rd_convt2x2_bwd_data", dout, wtd, dx, n, h, w, cin, cout)
    dw = k.out("dw", (cin, cout, 2, 2))
    ws, nb = k.ws("ws", lib.rd_convt2x2_bwd_weight_ws_bytes(n, h, w, cin, cout), short=True)
    k.quant(sdo, sx)
    k.call("rd_convt2x2_bwd_weight", x, dout, dw, n, h, w, cin, cout, ws, nb, refuses_short=True)

    def wrap():
        pf, pd = ops.pack_convt2x2_weight(wt)
        ops.amax_of(x), ops.amax_of(dout)
        return {"out": ops.convt2x2_fwd(x, pf, bias, skip), "dx": ops.convt2x2_bwd_data(dout, pd),
                "dw": ops.convt2x2_bwd_weight(x, dout)}
    k.wrapper(wrap)


def c_convt_bn(k, n, h, w, cin, cout):
    """the lazy-skip forward and the data gradient with the BN-statistics epilogue"""
    lib, ops = k.lib, _ops()
    x, wt, bias = k.inp("x", (n, h, w, cin)), k.inp("w", (cin, cout, 2, 2), scale=0.1), k.inp("bias", cout, scale=0.1)
    zs, dout, bz = k.inp("z_skip", (n, 2 * h, 2 * w, cout)), k.inp("dout", (n, 2 * h, 2 * w, cout)), k.inp("bn_z", (n, h, w, cin))
    sk = _bn(k, "sk", cout)
    bn = _bn(k, "bn", cin)
    wtf, wtd, sw = _packt(k, wt, cin, cout)
    sx, sdo = k.tag("x", x), k.tag("dout", dout)
    out = k.out("out", (n, 2 * h, 2 * w, cout))
    k.quant(sx, sw)
    k.call("rd_convt2x2_fwd_bnskip", x, wtf, bias, zs, *sk, 0.01, None, out, n, h, w, cin, cout)
    dx = k.out("dx", (n, h, w, cin))
    part, pf = k.part("part", lib.rd_bn_bwd_part_floats(n * h * w, cin), short=True)
    rows = k.rows()
    k.quant(sdo, sw)
    k.call("rd_convt2x2_bwd_data_bnstats", dout, wtd, dx, n, h, w, cin, cout, bz, *bn, 0.0, None, part, pf, C.byref(rows),
           refuses_short=True)
    _lim_part(k, "part", rows, cin)
    if not k.plan:
        assert rows.value * 4 * cin <= lib.rd_bn_bwd_part_floats(n * h * w, cin), "rows_out exceeds rd_bn_bwd_part_floats"

    def wrap():
        pf_, pd = ops.pack_convt2x2_weight(wt)
        ops.amax_of(x), ops.amax_of(dout)
        o = ops.convt2x2_fwd_bnskip(x, pf_, bias, zs, *sk, 0.01)
        dxx, (pp, rr) = ops.convt2x2_bwd_data(dout, pd, bn=ops.BnHook(bz, *bn, 0.0))
        assert rr == rows.value
        return {"out": o, "dx": dxx, "part": pp}
    k.wrapper(wrap)


def c_conv1x1(k, n, h, w, cin, cout):
    lib, ops = k.lib, _ops()
    px = n * h * w
    x, wt, dy = k.inp("x", (n, h, w, cin)), k.inp("w", (cout, cin, 1, 1), scale=0.1), k.inp("dy", (n, h, w, cout))
    wf, wtr = k.packed("wf", cout, 1, cin), k.packed("wt", cin, 1, cout)
    sw = k.slot("w_amax") if k.three else None
    k.quant(out2=sw)
    k.call("rd_pack_conv1x1_weight", wt, wf, wtr, cout, cin)
    sx, sdy = k.tag("x", x), k.tag("dy", dy)
    out = k.out("out", (n, h, w, cout))
    k.quant(sx, sw)
    k.call("rd_conv1x1_fwd", x, wf, out, px, cin, cout)
    dx = k.out("dx", (n, h, w, cin))
    k.quant(sdy, sw)
    k.call("rd_conv1x1_bwd_data", dy, wtr, dx, px, cin, cout)
    dw = k.out("dw", (cout, cin, 1, 1))
    ws, nb = k.ws("ws", lib.rd_conv1x1_bwd_weight_ws_bytes(px, cin, cout), short=True)
    k.quant(sdy, sx)
    k.call("rd_conv1x1_bwd_weight", x, dy, dw, px, cin, cout, ws, nb, refuses_short=True)

    def wrap():
        pf, pt = ops.pack_conv1x1_weight(wt)
        ops.amax_of(x), ops.amax_of(dy)
        return {"out": ops.conv1x1_fwd(x, pf), "dx": ops.conv1x1_bwd_data(dy, pt), "dw": ops.conv1x1_bwd_weight(x, dy)}
    k.wrapper(wrap)


def c_pack_fused(k, shapes):
    """rd_pack_weights_fused over a table of (kind, cout, cin): each packed buffer then feeds one forward launch, which must equal
    the layer-by-layer pack (the header: "same results as rd_pack_conv3x3_weight / rd_pack_convt2x2_weight layer by layer")"""
    lib, ops = k.lib, _ops()
    rows, begin, tbegin, layers = [], 0, 0, []
    for i, (kind, cout, cin) in enumerate(shapes):
        wt = k.inp(f"w{i}", (cout, cin, 3, 3) if kind == 0 else (cin, cout, 2, 2), scale=0.1)
        dims = ((cout, 9, cin), (cin, 9, cout)) if kind == 0 else ((4 * cout, 1, cin), (cin, 4, cout))
        bf, bd = k.packed(f"f{i}", *dims[0]), k.packed(f"d{i}", *dims[1])
        sl = k.slot(f"s{i}") if k.three else None
        f32 = 1 if kind == 1 else 0
        tiles = lib.rd_pack_item_tiles(kind, cout, cin)
        at = (begin, tbegin)
        if tiles > 0:
            tbegin += tiles
        else:
            begin += lib.rd_pack_item_pieces(kind, cout, cin, f32)
        layers.append((kind, cout, cin, wt, bf, bd, sl))
        if not k.plan:
            sp = lambda b, d: b.data_ptr() + (d[0] * d[1] * d[2] * 4 + 15) // 16 * 16      # noqa: E731
            rows.append([wt.data_ptr(), sp(bf, dims[0]), sp(bd, dims[1]), kind, cout, cin, at[0], bf.data_ptr() if f32 else 0, at[1],
                         sl.data_ptr() if sl is not None else 0])
    items = k.inp("items", (len(shapes), 10), fn=lambda: torch.tensor(rows, dtype=I64), dtype=I64)
    k.call("rd_pack_weights_fused", items, len(shapes), begin, tbegin)
    n, h, w = 2, 8, 16
    for i, (kind, cout, cin, wt, bf, bd, sl) in enumerate(layers):
        x = k.inp(f"x{i}", (n, h, w, cin))
        sx = k.tag(f"x{i}", x)
        k.quant(sx, sl)
        if kind == 0:
            z = k.out(f"z{i}", (n, h, w, cout))
            k.call("rd_conv3x3_fwd", x, bf, z, n, h, w, cin, cout)
            g = k.inp(f"g{i}", (n, h, w, cout))
            sg = k.tag(f"g{i}", g)
            dx = k.out(f"dx{i}", (n, h, w, cin))
            k.quant(sg, sl)
            k.call("rd_conv3x3_bwd_data", g, bd, dx, n, h, w, cin, cout)
        else:
            z = k.out(f"z{i}", (n, 2 * h, 2 * w, cout))
            k.call("rd_convt2x2_fwd", x, bf, None, None, z, n, h, w, cin, cout)
            g = k.inp(f"g{i}", (n, 2 * h, 2 * w, cout))
            sg = k.tag(f"g{i}", g)
            dx = k.out(f"dx{i}", (n, h, w, cin))
            k.quant(sg, sl)
            k.call("rd_convt2x2_bwd_data", g, bd, dx, n, h, w, cin, cout)

        def wrap(kind=kind, wt=wt, x=x, g=g, i=i):
            ops.amax_of(x), ops.amax_of(g)
            if kind == 0:
                pf, pd = ops.pack_conv3x3_weight(wt)
                return {f"z{i}": ops.conv3x3_fwd(x, pf), f"dx{i}": ops.conv3x3_bwd_data(g, pd)}
            pf, pd = ops.pack_convt2x2_weight(wt)
            return {f"z{i}": ops.convt2x2_fwd(x, pf, None, None), f"dx{i}": ops.convt2x2_bwd_data(g, pd)}
        k.wrapper(wrap)


# ---- first / last convolution and the tail ----------------------------------------------------------------------------------
def c_first(k, n, h, w, cin, cout):
    lib, ops = k.lib, _ops()
    x, wt, dz = k.inp("x", (n, cin, h, w)), k.inp("w", (cout, cin, 3, 3), scale=0.1), k.inp("dz", (n, h, w, cout))
    z = k.out("z", (n, h, w, cout))
    k.call("rd_conv3x3_first_fwd", x, wt, z, n, h, w, cin, cout)
    dw = k.out("dw", (cout, cin, 3, 3))
    ws, nb = k.ws("ws", lib.rd_conv3x3_first_bwd_weight_ws_bytes(n, h, w, cin, cout), short=True)
    k.call("rd_conv3x3_first_bwd_weight", x, dz, dw, n, h, w, cin, cout, ws, nb, refuses_short=True)
    k.wrapper(lambda: {"z": ops.conv3x3_first_fwd(x, wt), "dw": ops.conv3x3_first_bwd_weight(x, dz)})


def c_first_stats(k, n, h, w, cin, cout):
    lib, ops = k.lib, _ops()
    x, wt = k.inp("x", (n, cin, h, w)), k.inp("w", (cout, cin, 3, 3), scale=0.1)
    z, sums = k.out("z", (n, h, w, cout)), k.out("sums", 2 * cout, F64)
    ws, nb = k.ws("ws", lib.rd_conv3x3_first_fwd_stats_ws_bytes(n, h, w, cin, cout), short=True)
    k.call("rd_conv3x3_first_fwd_stats", x, wt, z, sums, n, h, w, cin, cout, ws, nb, refuses_short=True)

    def wrap():
        zz, ss = ops.conv3x3_first_fwd_stats(x, wt)
        return {"z": zz, "sums": ss}
    k.wrapper(wrap)


def c_first_bn(k, n, h, w, cin, cout):
    lib, ops = k.lib, _ops()
    x, wt = k.inp("x", (n, cin, h, w)), k.inp("w", (cout, cin, 3, 3), scale=0.1)
    z, mean, invstd = k.out("z", (n, h, w, cout)), k.out("mean", cout), k.out("invstd", cout)
    rm, rv = k.inout("rm", cout, scale=0.1), k.inout("rv", cout, fn=lambda: _rand(1, cout) + 0.5)
    ws, nb = k.ws("ws", lib.rd_conv3x3_first_fwd_stats_ws_bytes(n, h, w, cin, cout), short=True)
    k.call("rd_conv3x3_first_fwd_bn", x, wt, z, float(n * h * w), 1e-5, 0.1, mean, invstd, rm, rv, None, n, h, w, cin, cout, ws, nb,
           refuses_short=True)

    def wrap():
        a, b = k.first("rm"), k.first("rv")
        zz, m, i = ops.conv3x3_first_fwd_bn(x, wt, a, b, None)
        return {"z": zz, "mean": m, "invstd": i, "rm": a, "rv": b}
    k.wrapper(wrap)


def c_first_act(k, n, h, w, cin, cout):
    """first convolution with BN + activation + pool in its epilogue, and the weight gradient with the BN backward on the fly"""
    lib, ops = k.lib, _ops()
    assert lib.rd_conv3x3_first_fwd_act_available(n, h, w, cin, cout) and lib.rd_conv3x3_first_bwd_weight_bn_available(n, h, w, cin, cout)
    x, wt = k.inp("x", (n, cin, h, w)), k.inp("w", (cout, cin, 3, 3), scale=0.1)
    bn = _bn(k, "bn", cout)
    a, pooled = k.out("a", (n, h, w, cout)), k.out("pooled", (n, h // 2, w // 2, cout))
    sp = k.slot("pooled_amax") if k.three else None
    k.quant(out2=sp)
    k.call("rd_conv3x3_first_fwd_act", x, wt, *bn, 0.01, None, a, pooled, n, h, w, cin, cout)
    z = k.inp("z", (n, h, w, cout))
    gf, gp = k.inp("g_full", (n, h, w, cout)), k.inp("g_pool", (n, h // 2, w // 2, cout))
    idx = k.inp("idx", (n, h // 2, w // 2, cout), fn=lambda: _randint(5, 4, n, h // 2, w // 2, cout), dtype=U8)
    sums = k.inp("sums", 4 * cout, dtype=F64)
    dw = k.out("dw", (cout, cin, 3, 3))
    ws, nb = k.ws("ws", lib.rd_conv3x3_first_bwd_weight_ws_bytes(n, h, w, cin, cout), short=True)
    k.call("rd_conv3x3_first_bwd_weight_bn", x, z, *bn, 0.01, None, gf, gp, idx, sums, float(n * h * w), 1, None, None, dw, n, h, w,
           cin, cout, ws, nb, refuses_short=True)

    def wrap():
        aa, pp = ops.conv3x3_first_fwd_act(x, wt, *bn, 0.01, pool=True)
        d = ops.conv3x3_first_bwd_weight_bn(x, z, *bn, 0.01, gf, gp, idx, sums, n * h * w, True)
        return {"a": aa, "pooled": pp, "dw": d}
    k.wrapper(wrap)


def c_last(k, n, h, w, c, xc):
    lib, ops = k.lib, _ops()
    s, wt, bias = k.inp("s", (n, h, w, c)), k.inp("w", (1, c, 3, 3), scale=0.1), k.inp("bias", 1)
    x0, dout, bz = k.inp("x_nchw", (n, xc, h, w)), k.inp("dout", (n, 1, h, w)), k.inp("bn_z", (n, h, w, c))
    bn = _bn(k, "bn", c)
    out = k.out("out", (n, 1, h, w))
    k.call("rd_conv3x3_last_fwd", s, wt, bias, x0, xc, out, n, h, w, c)
    ds = k.out("ds", (n, h, w, c))
    k.call("rd_conv3x3_last_bwd_data", dout, wt, ds, n, h, w, c)
    dw, db = k.out("dw", (1, c, 3, 3)), k.out("dbias", 1)
    ws, nb = k.ws("ws", lib.rd_conv3x3_last_bwd_weight_ws_bytes(n, h, w, c), short=True)
    k.call("rd_conv3x3_last_bwd_weight", s, dout, dw, db, n, h, w, c, ws, nb, refuses_short=True)
    ds2 = k.out("ds2", (n, h, w, c))
    part, pf = k.part("part", lib.rd_bn_bwd_part_floats(n * h * w, c))
    rows = k.rows()
    k.call("rd_conv3x3_last_bwd_data_bnstats", dout, wt, ds2, n, h, w, c, bz, *bn, 0.01, None, part, pf, C.byref(rows))
    _lim_part(k, "part", rows, c)
    if not k.plan:
        assert rows.value * 4 * c <= lib.rd_bn_bwd_part_floats(n * h * w, c), "rows_out exceeds rd_bn_bwd_part_floats"

    def wrap():
        d, b = ops.conv3x3_last_bwd_weight(s, dout)
        d2, (pp, rr) = ops.conv3x3_last_bwd_data(dout, wt, c, bn=ops.BnHook(bz, *bn, 0.01))
        assert rr == rows.value
        return {"out": ops.conv3x3_last_fwd(s, wt, bias, x0), "ds": ops.conv3x3_last_bwd_data(dout, wt, c), "dw": d, "dbias": b,
                "ds2": d2, "part": pp}
    k.wrapper(wrap)


def c_last_part_short(k, n, h, w, c):
    lib = k.lib
    wt, dout, bz = k.inp("w", (1, c, 3, 3), scale=0.1), k.inp("dout", (n, 1, h, w)), k.inp("bn_z", (n, h, w, c))
    bn = _bn(k, "bn", c)
    ds = k.out("ds", (n, h, w, c))
    part, pf = k.part("part", lib.rd_bn_bwd_part_floats(n * h * w, c), short=True)
    rows = k.rows()
    k.call("rd_conv3x3_last_bwd_data_bnstats", dout, wt, ds, n, h, w, c, bz, *bn, 0.01, None, part, pf, C.byref(rows),
           refuses_short=True)
    _lim_part(k, "part", rows, c)

    def wrap():
        d, (pp, rr) = _ops().conv3x3_last_bwd_data(dout, wt, c, bn=_ops().BnHook(bz, *bn, 0.01))
        assert rr == rows.value
        return {"ds": d, "part": pp}
    k.wrapper(wrap)


def c_tail(k, n, h, w, cin, c0):
    """every entry point of the composed tail; (n, h, w) is the full resolution, the up-convolution's input is (h/2, w/2)"""
    lib, ops = k.lib, _ops()
    assert lib.rd_tail_available(cin, c0)
    hc, wc = h // 2, w // 2
    wt, bt = k.inp("wt", (cin, c0, 2, 2), scale=0.1), k.inp("bias_t", c0, scale=0.1)
    wl, bl = k.inp("w_last", (1, c0, 3, 3), scale=0.1), k.inp("bias", 1)
    xcr, z0 = k.inp("x_coarse", (n, hc, wc, cin)), k.inp("z0", (n, h, w, c0))
    dout, x0 = k.inp("dout", (n, 1, h, w)), k.inp("x_nchw", (n, 3, h, w))
    b0 = _bn(k, "bn0", c0)
    b1 = _bn(k, "bn1", cin)
    M, V, VT, B9 = k.out("M", (cin, 4, 9)), k.out("V", (cin, 16)), k.out("VT", (16, cin, 1, 1)), k.out("B9", 9)
    k.call("rd_tail_compose", wt, bt, wl, M, V, VT, B9, cin, c0)
    t16 = k.out("t16", (n, hc, wc, 16))
    k.call("rd_tail_t16", xcr, None, None, None, None, 1.0, None, V, t16, n * hc * wc, cin)
    t16b = k.out("t16_bn", (n, hc, wc, 16))
    k.call("rd_tail_t16", xcr, *b1, 0.01, None, V, t16b, n * hc * wc, cin)
    out = k.out("out", (n, 1, h, w))
    k.call("rd_conv3x3_last_fwd_tail", z0, *b0, 0.01, None, t16, B9, wl, bl, x0, 3, out, n, h, w, c0)
    dprev = k.out("dprev", (n, hc, wc, cin))
    k.call("rd_convt_last_bwd_data", dout, V, dprev, n, hc, wc, cin, None, None, None, None, None, 0.0, None, None, 0, None)
    dprev2 = k.out("dprev_bn", (n, hc, wc, cin))
    part1, pf1 = k.part("part1", lib.rd_bn_bwd_part_floats(n * hc * wc, cin))
    rows1 = k.rows()
    k.call("rd_convt_last_bwd_data", dout, V, dprev2, n, hc, wc, cin, xcr, *b1, 0.01, None, part1, pf1, C.byref(rows1))
    _lim_part(k, "part1", rows1, cin)
    dwt, c16 = k.out("dwt", (cin, c0, 2, 2)), k.out("c16", (cin, 16), F64)
    ws, nb = k.ws("ws", lib.rd_convt_last_bwd_weight_ws_bytes(n, hc, wc, cin), short=True)
    k.call("rd_convt_last_bwd_weight", xcr, dout, wl, dwt, c16, n, hc, wc, cin, c0, ws, nb, refuses_short=True)
    dwt2 = k.out("dwt_bn", (cin, c0, 2, 2))
    ws2, nb2 = k.ws("ws2", lib.rd_convt_last_bwd_weight_ws_bytes(n, hc, wc, cin))
    k.call("rd_convt_last_bwd_weight_bn", xcr, *b1, 0.01, None, dout, wl, dwt2, None, n, hc, wc, cin, c0, ws2, nb2)
    # the head of the backward: wpartial has exactly rd_conv3x3_last_bwd_tail_blocks rows, `part` that many rows of 4 * C floats
    blocks = lib.rd_conv3x3_last_bwd_tail_blocks(n, h, w)
    wpart = k.out("wpartial", (blocks, 9 * c0 + 9), F64)
    part0, pf0 = k.part("part0", blocks * 4 * c0)
    rows0 = k.rows()
    k.call("rd_conv3x3_last_bwd_tail_fused", z0, *b0, 0.01, None, dout, wl, wpart, part0, pf0, C.byref(rows0), n, h, w, c0)
    _lim_part(k, "part0", rows0, c0)
    if not k.plan:
        assert rows0.value == blocks
    dw, db = k.out("dw", (1, c0, 3, 3)), k.out("dbias", 1)
    k.call("rd_tail_wl_finish", wpart, blocks, c16, wt, bt, dw, db, cin, c0)
    dw2, db2 = k.out("dw2", (1, c0, 3, 3)), k.out("dbias2", 1)
    ws3, nb3 = k.ws("ws3", lib.rd_conv3x3_last_bwd_weight_tail_ws_bytes(n, h, w, c0))
    k.call("rd_conv3x3_last_bwd_weight_tail", z0, *b0, 0.01, None, dout, c16, wt, bt, dw2, db2, n, h, w, cin, c0, ws3, nb3)

    def wrap():
        skip = dict(z=z0, mean=b0[0], invstd=b0[1], gamma=b0[2], beta=b0[3], slope=0.01, slope_dev=None)
        lazy = dict(z=xcr, mean=b1[0], invstd=b1[1], gamma=b1[2], beta=b1[3], slope=0.01, slope_dev=None)
        m, v, vt, b9 = ops.tail_compose(wt, wl, bt, forward=True)
        t = ops.tail_t16(xcr, v)
        d2, (pp1, rr1) = ops.convt_last_bwd_data(dout, v, bn=ops.BnHook(xcr, *b1, 0.01))
        cc = torch.empty(cin, 16, device=DEV, dtype=F64)
        dwt_ = ops.convt_last_bwd_weight(xcr, dout, wl, c16=cc)
        wp, (pp0, rr0) = ops.conv3x3_last_bwd_tail_fused(skip, dout, wl)
        assert rr1 == rows1.value and rr0 == rows0.value
        dw_, db_ = ops.tail_wl_finish(wp, cc, wt, bt)
        dw2_, db2_ = ops.conv3x3_last_bwd_weight_tail(skip, dout, cc, wt, bt)
        return {"M": m, "V": v, "VT": vt, "B9": b9, "t16": t, "t16_bn": ops.tail_t16(lazy, v),
                "out": ops.conv3x3_last_fwd_tail(skip, t, b9, wl, bl, x0), "dprev": ops.convt_last_bwd_data(dout, v), "dprev_bn": d2,
                "part1": pp1, "dwt": dwt_, "c16": cc, "dwt_bn": ops.convt_last_bwd_weight(lazy, dout, wl), "wpartial": wp,
                "part0": pp0, "dw": dw_, "dbias": db_, "dw2": dw2_, "dbias2": db2_}
    k.wrapper(wrap)


def c_tail_short(k, which, n, h, w, cin, c0):
    """the undersized-scratch refusals of the tail entry points that c_tail does not stop at"""
    lib = k.lib
    hc, wc = h // 2, w // 2
    wt, bt, wl = k.inp("wt", (cin, c0, 2, 2), scale=0.1), k.inp("bias_t", c0, scale=0.1), k.inp("w_last", (1, c0, 3, 3), scale=0.1)
    xcr, z0, dout = k.inp("x_coarse", (n, hc, wc, cin)), k.inp("z0", (n, h, w, c0)), k.inp("dout", (n, 1, h, w))
    V, c16 = k.inp("V", (cin, 16)), k.inp("c16", (cin, 16), dtype=F64)
    b0, b1 = _bn(k, "bn0", c0), _bn(k, "bn1", cin)
    rows = k.rows()
    ops = _ops()
    skip = dict(z=z0, mean=b0[0], invstd=b0[1], gamma=b0[2], beta=b0[3], slope=0.01, slope_dev=None)
    lazy = dict(z=xcr, mean=b1[0], invstd=b1[1], gamma=b1[2], beta=b1[3], slope=0.01, slope_dev=None)
    if which == "dgrad":
        dprev = k.out("dprev", (n, hc, wc, cin))
        part, pf = k.part("part", lib.rd_bn_bwd_part_floats(n * hc * wc, cin), short=True)
        k.call("rd_convt_last_bwd_data", dout, V, dprev, n, hc, wc, cin, xcr, *b1, 0.01, None, part, pf, C.byref(rows),
               refuses_short=True)
        _lim_part(k, "part", rows, cin)

        def wrap():
            d, (pp, rr) = ops.convt_last_bwd_data(dout, V, bn=ops.BnHook(xcr, *b1, 0.01))
            assert rr == rows.value
            return {"dprev": d, "part": pp}
    elif which == "wgrad_bn":
        dwt = k.out("dwt", (cin, c0, 2, 2))
        ws, nb = k.ws("ws", lib.rd_convt_last_bwd_weight_ws_bytes(n, hc, wc, cin), short=True)
        k.call("rd_convt_last_bwd_weight_bn", xcr, *b1, 0.01, None, dout, wl, dwt, None, n, hc, wc, cin, c0, ws, nb, refuses_short=True)

        def wrap():
            return {"dwt": ops.convt_last_bwd_weight(lazy, dout, wl)}
    elif which == "fused":
        blocks = lib.rd_conv3x3_last_bwd_tail_blocks(n, h, w)
        wpart = k.out("wpartial", (blocks, 9 * c0 + 9), F64)
        part, pf = k.part("part", blocks * 4 * c0, short=True)
        k.call("rd_conv3x3_last_bwd_tail_fused", z0, *b0, 0.01, None, dout, wl, wpart, part, pf, C.byref(rows), n, h, w, c0,
               refuses_short=True)
        _lim_part(k, "part", rows, c0)

        def wrap():
            wp, (pp, rr) = ops.conv3x3_last_bwd_tail_fused(skip, dout, wl)
            assert rr == rows.value
            return {"wpartial": wp, "part": pp}
    else:
        dw, db = k.out("dw", (1, c0, 3, 3)), k.out("dbias", 1)
        ws, nb = k.ws("ws", lib.rd_conv3x3_last_bwd_weight_tail_ws_bytes(n, h, w, c0), short=True)
        k.call("rd_conv3x3_last_bwd_weight_tail", z0, *b0, 0.01, None, dout, c16, wt, bt, dw, db, n, h, w, cin, c0, ws, nb,
               refuses_short=True)

        def wrap():
            d, b = ops.conv3x3_last_bwd_weight_tail(skip, dout, c16, wt, bt)
            return {"dw": d, "dbias": b}
    k.wrapper(wrap)


# ---- BatchNorm / activation / pooling, reductions, loss ---------------------------------------------------------------------
def c_bn_act(k, n, h, w, c, pool):
    lib, ops = k.lib, _ops()
    z = k.inp("z", (n, h, w, c))
    bn = _bn(k, "bn", c)
    a = k.out("a", (n, h, w, c))
    hp, wp = h // 2, w // 2
    pooled = idx = zpool = gp = None
    if pool:
        pooled, idx, zpool = k.out("pooled", (n, hp, wp, c)), k.out("idx", (n, hp, wp, c), U8), k.out("zpool", (n, hp, wp, c))
        gp = k.inp("g_pool", (n, hp, wp, c))
    gf = k.inp("g_full", (n, h, w, c))
    sa = k.slot("a_amax") if k.three and not pool else None
    sp = k.slot("pooled_amax") if k.three and pool else None
    k.quant(out=sa, out2=sp)
    k.call("rd_bn_act_pool_fwd", z, *bn, 0.01, None, a, pooled, idx, zpool, n, h, w, c)
    sums, dg, db, de = k.out("sums", 4 * c, F64), k.out("dgamma", c), k.out("dbeta", c), k.out("dextra", c)
    ws, nb = k.ws("ws", lib.rd_bn_act_bwd_ws_bytes(n, h, w, c), short=True)
    k.call("rd_bn_act_bwd_reduce", z, *bn, 0.01, None, gf, gp, idx, sums, dg, db, de, n, h, w, c, ws, nb, refuses_short=True)
    dz, dg2, db2 = k.out("dz", (n, h, w, c)), k.out("dgamma2", c), k.out("dbeta2", c)
    sdz = k.slot("dz_amax") if k.three else None
    k.quant(out=sdz)
    k.call("rd_bn_act_bwd_apply", z, *bn, 0.01, None, gf, gp, idx, sums, float(n * h * w), 1, dz, dg2, db2, n, h, w, c)

    def wrap():
        res = ops.bn_act_pool_fwd(z, *bn, 0.01, pool, want_zpool=pool)
        g, b, e = (torch.empty(c, device=DEV) for _ in range(3))
        g2, b2 = (torch.empty(c, device=DEV) for _ in range(2))
        ix = res[2]
        s = ops.bn_act_bwd_reduce(z, *bn, 0.01, gf, gp, ix, dgamma=g, dbeta=b, dextra=e)
        d = ops.bn_act_bwd_apply(z, *bn, 0.01, gf, gp, ix, s, n * h * w, True, dgamma=g2, dbeta=b2)
        r = {"a": res[0], "sums": s, "dgamma": g, "dbeta": b, "dextra": e, "dz": d, "dgamma2": g2, "dbeta2": b2}
        if pool:
            r.update(pooled=res[1], idx=res[2], zpool=res[3])
        return r
    k.wrapper(wrap)


def c_bn_finalize(k, rows_a, rows_b, c):
    """rd_bn_bwd_stats_finalize over the partial rows of one or two producers"""
    ops = _ops()
    pa = k.inp("part_a", (rows_a, 4, c))
    pb = k.inp("part_b", (rows_b, 4, c)) if rows_b else None
    sums, dg, db, de = k.out("sums", 4 * c, F64), k.out("dgamma", c), k.out("dbeta", c), k.out("dextra", c)
    k.call("rd_bn_bwd_stats_finalize", pa, rows_a, pb, rows_b, c, sums, dg, db, de)

    def wrap():
        g, b, e = (torch.empty(c, device=DEV) for _ in range(3))
        parts = [(pa, rows_a)] + ([(pb, rows_b)] if rows_b else [])
        return {"sums": ops.bn_bwd_stats_finalize(parts, c, g, b, e), "dgamma": g, "dbeta": b, "dextra": e}
    k.wrapper(wrap)


def c_bn_stats(k, n, h, w, c):
    lib, ops = k.lib, _ops()
    px = n * h * w
    z = k.inp("z", (n, h, w, c))
    sums = k.out("sums", 2 * c, F64)
    ws, nb = k.ws("ws", lib.rd_bn_stats_ws_bytes(px, c), short=True)
    k.call("rd_bn_stats_partial", z, sums, px, c, ws, nb, refuses_short=True)
    mean, invstd = k.out("mean", c), k.out("invstd", c)
    rm, rv = k.inout("rm", c, scale=0.1), k.inout("rv", c, fn=lambda: _rand(1, c) + 0.5)
    nbt = k.inout("nbt", 1, fn=lambda: torch.tensor([3]), dtype=I64)
    k.call("rd_bn_stats_finalize", sums, float(px), 1e-5, 0.1, mean, invstd, rm, rv, nbt, c)
    m2, i2 = k.out("mean_eval", c), k.out("invstd_eval", c)
    k.call("rd_bn_eval_stats", rm, rv, 1e-5, m2, i2, c)
    cs = k.out("chsum", c)
    ws2, nb2 = k.ws("ws2", lib.rd_channel_sum_ws_bytes(px, c))
    k.call("rd_channel_sum", z, cs, px, c, ws2, nb2)

    def wrap():
        s = ops.bn_stats_partial(z)
        a, b, t = k.first("rm"), k.first("rv"), k.first("nbt")
        m, i = ops.bn_stats_finalize(s, px, a, b, t)
        me, ie = ops.bn_eval_stats(a, b)
        return {"sums": s, "mean": m, "invstd": i, "rm": a, "rv": b, "nbt": t, "mean_eval": me, "invstd_eval": ie,
                "chsum": ops.channel_sum(z)}
    k.wrapper(wrap)


def c_channel_sum_short(k, n, h, w, c):
    px = n * h * w
    z, cs = k.inp("z", (n, h, w, c)), k.out("chsum", c)
    ws, nb = k.ws("ws", k.lib.rd_channel_sum_ws_bytes(px, c), short=True)
    k.call("rd_channel_sum", z, cs, px, c, ws, nb, refuses_short=True)
    k.wrapper(lambda: {"chsum": _ops().channel_sum(z)})


def c_masked_l1(k, n, h, w):
    lib, ops = k.lib, _ops()
    yp, y = k.inp("yp", (n, 1, h, w)), k.inp("y", (n, 1, h, w))
    mask = k.inp("mask", (n, 1, h, w), dtype=U8)
    mean, std = k.inp("mean", n), k.pos("std", n)
    gout = k.inp("gout", 1, fn=lambda: torch.tensor([0.75]))
    sums = k.out("sums", 2, F64)
    ws, nb = k.ws("ws", lib.rd_masked_l1_ws_bytes(n * h * w), short=True)
    k.call("rd_masked_l1_partial", yp, y, mask, mean, std, sums, n, h * w, ws, nb, refuses_short=True)
    loss, dyp = k.out("loss", 1), k.out("dyp", (n, 1, h, w))
    k.call("rd_masked_l1_finish", yp, y, mask, mean, std, sums, float(n * h * w), gout, loss, dyp, n, h * w)

    def wrap():
        s = ops.masked_l1_partial(yp, y, mask, mean, std)
        lo, d = ops.masked_l1_finish(yp, y, mask, mean, std, s, n * h * w, gout=gout)
        return {"sums": s, "loss": lo, "dyp": d}
    k.wrapper(wrap)


def c_upsample(k, n, h, w, c):
    ops = _ops()
    t, bias, skip, g = k.inp("t", (n, h, w, c)), k.inp("bias", c), k.inp("skip", (n, 2 * h, 2 * w, c)), k.inp("g", (n, 2 * h, 2 * w, c))
    out, dt = k.out("out", (n, 2 * h, 2 * w, c)), k.out("dt", (n, h, w, c))
    k.call("rd_upsample2x_add_fwd", t, bias, skip, out, n, h, w, c)
    k.call("rd_upsample2x_bwd", g, dt, n, h, w, c)
    k.wrapper(lambda: {"out": ops.upsample2x_add_fwd(t, bias, skip), "dt": ops.upsample2x_bwd(g)})


def c_layout(k, n, c, h, w):
    ops = _ops()
    a, b = k.inp("nchw", (n, c, h, w)), k.inp("nhwc", (n, h, w, c))
    o1, o2 = k.out("to_nhwc", (n, h, w, c)), k.out("to_nchw", (n, c, h, w))
    k.call("rd_nchw_to_nhwc", a, o1, n, c, h, w)
    k.call("rd_nhwc_to_nchw", b, o2, n, c, h, w)
    k.wrapper(lambda: {"to_nhwc": ops.nchw_to_nhwc(a), "to_nchw": ops.nhwc_to_nchw(b)})


# ---- optimizers, rd_zero, rd_copy_segments, rd_amax -------------------------------------------------------------------------
def c_optim(k, numel):
    ops = _ops()
    g = k.inp("g", numel)
    sc = [1.0 - 0.9, 0.999, 1.0 - 0.999, 1e-8, 1e-5, 2e-4, 0.9, 0.5]
    scal = k.inp("scalars", 8, fn=lambda: torch.tensor(sc))
    st = {}
    for tagname in ("adam", "adamdev", "sgd", "sgd0"):
        st[tagname] = (k.inout(f"p_{tagname}", numel), k.inout(f"m_{tagname}", numel, scale=0.1),
                       k.inout(f"v_{tagname}", numel, fn=lambda: _rand(2, numel) * 0.1))
    p, m, v = st["adam"]
    k.call("rd_adam_step", p, g, m, v, numel, 0.9, 0.999, 1e-8, 1e-5, 2e-4, 0.9, 0.5)
    p, m, v = st["adamdev"]
    k.call("rd_adam_step_dev", p, g, m, v, numel, scal)
    p, m, _ = st["sgd"]
    k.call("rd_sgd_step", p, g, m, numel, 0.01, 1e-4, 0.9, 0.1, 1, 0, 0.5)
    p0 = st["sgd0"][0]
    k.call("rd_sgd_step", p0, g, None, numel, 0.01, 1e-4, 0.0, 0.0, 0, 0, 1.0)

    def wrap():
        f = {n_: k.first(n_) for n_ in k.initial}
        ops.adam_step(f["p_adam"], g, f["m_adam"], f["v_adam"], 0.9, 0.999, 1e-8, 1e-5, 2e-4, 0.9, 0.5)
        ops.adam_step_dev(f["p_adamdev"], g, f["m_adamdev"], f["v_adamdev"], scal)
        ops.sgd_step(f["p_sgd"], g, f["m_sgd"], 0.01, 1e-4, 0.9, 0.1, True, False, 0.5)
        ops.sgd_step(f["p_sgd0"], g, None, 0.01, 1e-4)
        return f
    k.wrapper(wrap)


def c_zero_copy(k, n16):
    """rd_zero / rd_copy_segments on ranges of whole 16-byte units, rd_amax on a length that is not a multiple of anything"""
    nb = 16 * n16
    srcs = [k.inp(f"src{i}", (n16 + i) * 4) for i in range(3)]
    dsts = [k.out(f"dst{i}", (n16 + i) * 4) for i in range(3)]
    zed = k.out("zeroed", nb // 4)
    x = k.inp("x", 4 * n16 + 3)
    slot = k.slot("x_amax")
    k.call("rd_zero", zed, nb)
    if not k.plan:
        k.call("rd_copy_segments", (C.c_void_p * 3)(*[d.data_ptr() for d in dsts]), (C.c_void_p * 3)(*[s.data_ptr() for s in srcs]),
               (C.c_size_t * 3)(*[16 * (n16 + i) for i in range(3)]), 3)
        k.call("rd_amax", x, x.numel(), slot)

    def ref():
        assert int(zed.view(I32).abs().sum()) == 0
        for s, d in zip(srcs, dsts):
            assert torch.equal(s, d)
        top = slot.view(16, 32)[:, 0].max().view(1).view(F32)
        assert float(top) == float(x.abs().max())
    k.ref(ref)


# ---- tiled inference, sample assembly, raster statistics --------------------------------------------------------------------
def c_blend(k, n, tile, stride, rows, cols):
    ops = _ops()
    pred, mean, std = k.inp("pred", (n, 1, tile, tile)), k.inp("mean", n), k.pos("std", n)
    per_row = (cols - tile) // stride + 1
    pos_l = [[(i // per_row) * stride, (i % per_row) * stride] for i in range(n)]
    assert all(p[0] + tile <= rows for p in pos_l)
    pos = k.inp("pos", (n, 2), fn=lambda: torch.tensor(pos_l), dtype=I32)
    reg = k.inp("reg", (n, 4), fn=lambda: torch.tensor([[0, 0, rows - 1, cols - 1]] * n), dtype=I32)
    raster = k.inout("raster", (rows, cols), dtype=F64)
    k.call("rd_blend_accumulate", pred, mean, std, pos, reg, n, tile, stride, raster, rows, cols)
    k.wrapper(lambda: {"raster": ops.blend_accumulate(pred, mean, std, pos, reg, tile, stride, k.first("raster"))})


def c_patches(k, n, tile, height, width, views):
    """rd_patch_sums + rd_assemble_patches on a raster with odd row and column counts"""
    planes = 2 * views
    dsm_in = k.inp("dsm_in", (height, width), scale=10.0)
    dsm_gt = k.inp("dsm_gt", (height, width), fn=lambda: _with_nodata(height, width, 11))
    ortho = k.inp("ortho", (planes, height, width), fn=lambda: _rand(3, planes, height, width) * 255)
    pos_l = [[(3 * i) % (height - tile + 1), (5 * i + 1) % (width - tile + 1)] for i in range(n - 1)] + [[height - tile, width - tile]]
    pos = k.inp("pos", (n, 2), fn=lambda: torch.tensor(pos_l), dtype=I32)
    pair = k.inp("pair", (n, views), fn=lambda: torch.tensor([[(i + j) % planes for j in range(views)] for i in range(n)]), dtype=I32)
    zero = k.inp("plane0", n, fn=lambda: torch.zeros(n), dtype=I32)
    aug = k.inp("aug", n, fn=lambda: torch.arange(n) % 16, dtype=I32)
    sums, osums = k.out("sums", (n, 2), F64), k.out("osums", (n, 2), F64)
    k.call("rd_patch_sums", dsm_in, height * width, zero, 1, pos, n, tile, width, -9999.0, 1, sums)
    k.call("rd_patch_sums", ortho, height * width, pair, views, pos, n, tile, width, 0.0, 0, osums)
    dmean = k.inp("dsm_mean", n, fn=lambda: torch.linspace(-1, 1, n))
    omean = k.inp("ortho_mean", n, fn=lambda: torch.linspace(100, 120, n))
    inp_, tgt, msk = k.out("input", (n, 1 + views, tile, tile)), k.out("target", (n, 1, tile, tile)), k.out("mask", (n, 1, tile, tile), U8)
    k.call("rd_assemble_patches", dsm_in, dsm_gt, ortho, height * width, pair, views, pos, aug, dmean, 2.5, omean, 60.0, -9999.0, n, tile,
           width, inp_, tgt, msk)

    def ref():
        for i, (y, x) in enumerate(pos_l):
            p = dsm_in[y:y + tile, x:x + tile].double()
            assert abs(float(sums[i, 0]) - float(p.sum())) <= 1e-10 * float(p.abs().sum()) and int(sums[i, 1]) == tile * tile
        # sample 0 has aug = 0 (no rotation, no flip): its planes are the normalised patches, rounded as torch's sub_ / div_
        y, x = pos_l[0]
        assert torch.equal(inp_[0, 0].cpu(), (dsm_in[y:y + tile, x:x + tile].cpu() - dmean[0].cpu()) / 2.5)
        g = dsm_gt[y:y + tile, x:x + tile]
        assert torch.equal(msk[0, 0].bool(), (g != 0) & (g != -9999.0))
    k.ref(ref)


def _with_nodata(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(h, w, generator=g) * 10
    t[torch.rand(h, w, generator=g) < 0.1] = -9999.0
    t[torch.rand(h, w, generator=g) < 0.05] = 0.0
    return t


def c_grid_tiles(k, n, tile, height, width, views, mode):
    lib = k.lib
    planes, n_pairs = views + 1, 2
    dsm_in = k.inp("dsm_in", (height, width), fn=lambda: _with_nodata(height, width, 5))
    dsm_gt = k.inp("dsm_gt", (height, width), fn=lambda: _with_nodata(height, width, 6))
    ortho = k.inp("ortho", (planes, height, width), fn=lambda: _rand(3, planes, height, width) * 255)
    smp = [[(7 * i) % (height - tile + 1), (3 * i) % (width - tile + 1), 1, 1, tile - 2, tile - 2, i % n_pairs, 0] for i in range(n - 1)]
    smp.append([height - tile, width - tile, 0, 0, tile - 1, tile - 1, 1, 0])
    samples = k.inp("samples", (n, 8), fn=lambda: torch.tensor(smp), dtype=I32)
    pairs = k.inp("pair_planes", (n_pairs, views), fn=lambda: torch.tensor([[(p + j) % planes for j in range(views)] for p in range(n_pairs)]),
                  dtype=I32)
    inp_, tgt = k.out("input", (n, 1 + views, tile, tile)), k.out("target", (n, 1, tile, tile))
    msk, dmo = k.out("mask", (n, 1, tile, tile), U8), k.out("dsm_mean_out", n)
    ws, nb = k.ws("ws", lib.rd_assemble_grid_tiles_ws_bytes(n, tile), short=(mode == 2))
    k.call("rd_assemble_grid_tiles", dsm_in, dsm_gt, ortho, planes, height, width, samples, pairs, n_pairs, views, 1, n, tile, -9999.0,
           mode, 1.5, 2.5, mode, 110.0, 60.0, inp_, tgt, msk, dmo, ws, nb, refuses_short=(mode == 2))

    def ref():
        y, x = smp[-1][0], smp[-1][1]
        g = dsm_gt[y:y + tile, x:x + tile]
        assert torch.equal(msk[-1, 0].bool(), (g != 0) & (g != -9999.0))
        if mode == 1:
            assert torch.equal(inp_[-1, 0].cpu(), (dsm_in[y:y + tile, x:x + tile].cpu() - 1.5) / 2.5)
    k.ref(ref)


def c_train_patches(k, n, tile, views):
    dims = [(37, 45), (51, 33)]
    ras, table = [], []
    for r, (hh, ww) in enumerate(dims):
        ras.append((k.inp(f"dsm_in{r}", (hh, ww), fn=lambda hh=hh, ww=ww, r=r: _with_nodata(hh, ww, 20 + r)),
                    k.inp(f"dsm_gt{r}", (hh, ww), fn=lambda hh=hh, ww=ww, r=r: _with_nodata(hh, ww, 30 + r)),
                    k.inp(f"ortho{r}", (3, hh, ww), fn=lambda hh=hh, ww=ww, r=r: _rand(40 + r, 3, hh, ww) * 255)))
    if not k.plan:
        for r, (hh, ww) in enumerate(dims):
            a, b, c = ras[r]
            table.append(struct.pack("<QQQiiiffiffii", a.data_ptr(), b.data_ptr(), c.data_ptr(), hh, ww, 3, -9999.0, 2.5, r + 1, 110.0,
                                     60.0, 0, 0))
    desc = k.inp("rasters", 64 * len(dims), fn=lambda: torch.frombuffer(bytearray(b"".join(table)), dtype=U8), dtype=U8)
    cols = []
    for i in range(n):
        r = i % 2
        hh, ww = dims[r]
        last = i >= n - 2
        cols.append([r, hh - tile if last else (5 * i) % (hh - tile + 1), ww - tile if last else (3 * i) % (ww - tile + 1), i % 16, i % 3,
                     struct.unpack("<i", struct.pack("<f", 0.5))[0], 0, 0] + [(i + j) % 3 for j in range(views)])
    samples = k.inp("samples", ((8 + views) * n,), fn=lambda: torch.tensor(cols).t().contiguous().reshape(-1), dtype=I32)
    inp_, tgt = k.out("input", (n, 1 + views, tile, tile)), k.out("target", (n, 1, tile, tile))
    msk, dmo = k.out("mask", (n, 1, tile, tile), U8), k.out("dsm_mean_out", n)
    sums = k.opaque("sums", n * 4 * 8)                  # "device scratch of n * 4 doubles"
    k.call("rd_assemble_train_patches", desc, len(dims), samples, n, views, 1, tile, inp_, tgt, msk, dmo, sums)

    def ref():
        assert float(dmo[0]) == 0.0 and float(dmo[1]) == 0.5         # DSM modes 0 and 1
        # sample 0: raster 0 at (0, 0), aug 0 (no rotation, no flip) -- its mask is the target's validity, as in c_patches
        g = ras[0][1][:tile, :tile]
        assert torch.equal(msk[0, 0].bool(), (g != 0) & (g != -9999.0))
        # sample 1: raster 1 at (5, 3), aug 1 = rot90(k = 1), DSM mode 1 (mean 0.5): torch.rot90 of the normalised patch
        g1 = ras[1][1][5:5 + tile, 3:3 + tile]
        assert torch.equal(msk[1, 0].bool().cpu(), torch.rot90((g1 != 0) & (g1 != -9999.0), 1).cpu())
    k.ref(ref)


def c_moments(k, n, tile, height, width):
    lib = k.lib
    plane = k.inp("plane", (height, width), fn=lambda: _with_nodata(height, width, 9))
    pos_l = [[(3 * i) % (height - tile + 1), (7 * i) % (width - tile + 1)] for i in range(n - 1)] + [[height - tile, width - tile]]
    pos = k.inp("pos", (n, 2), fn=lambda: torch.tensor(pos_l), dtype=I32)
    out = k.out("out", (n, 3), F64)
    ws, nb = k.ws("ws", lib.rd_patch_moments_ws_bytes(n, tile), short=True)
    k.call("rd_patch_moments", plane, height, width, pos, n, tile, -9999.0, 1, out, ws, nb, refuses_short=True)
    stack = k.inp("stack", (3, height, width), fn=lambda: _rand(4, 3, height, width) * 255)
    rects = (C.c_int * 8)(0, height, 0, width // 2, height // 3, height, width // 2, width)
    pidx = (C.c_int * 2)(2, 0)
    out2 = k.out("region", 3, F64)
    ws2, nb2 = k.ws("ws2", lib.rd_region_moments_ws_bytes(height, width, 2, rects, 2))
    k.call("rd_region_moments", stack, height * width, 3, height, width, pidx, 2, rects, 2, out2, ws2, nb2)

    def ref():
        for i, (y, x) in enumerate(pos_l):
            p = plane[y:y + tile, x:x + tile].double()
            p = p[p != -9999.0]
            assert int(out[i, 0]) == p.numel()
            if p.numel():
                assert abs(float(out[i, 1]) - float(p.mean())) <= 1e-9 * float(p.abs().max())
        px = torch.cat([stack[pl, rects[4 * j]:rects[4 * j + 1], rects[4 * j + 2]:rects[4 * j + 3]].reshape(-1) for pl in (2, 0)
                        for j in range(2)]).double()
        assert int(out2[0]) == px.numel() and abs(float(out2[1]) - float(px.mean())) <= 1e-9 * 255
    k.ref(ref)


def c_region_short(k, height, width):
    stack = k.inp("stack", (3, height, width), fn=lambda: _rand(4, 3, height, width) * 255)
    rects = (C.c_int * 4)(1, height, 0, width - 1)
    pidx = (C.c_int * 1)(1)
    out = k.out("region", 3, F64)
    ws, nb = k.ws("ws", k.lib.rd_region_moments_ws_bytes(height, width, 1, rects, 1), short=True)
    k.call("rd_region_moments", stack, height * width, 3, height, width, pidx, 1, rects, 1, out, ws, nb, refuses_short=True)


def c_eval(k, rows, cols):
    """dilation, classification and both statistics entry points on a raster with odd row and column counts"""
    lib = k.lib
    n = rows * cols
    pred = k.inp("pred", (rows, cols), fn=lambda: _with_nodata(rows, cols, 1), dtype=F64)
    init = k.inp("init", (rows, cols), fn=lambda: _with_nodata(rows, cols, 2))
    gt = k.inp("gt", (rows, cols), fn=lambda: _with_nodata(rows, cols, 3))
    bits = {nm: k.inp(nm, (rows, cols), dtype=U8) for nm in ("gt_mask", "bmask", "bnodata", "water", "forest")}
    dil = k.out("dilated", (rows, cols), U8)
    k.call("rd_dilate_mask", bits["bmask"], dil, rows, cols, 3)
    rb, ra, cls = k.out("r_before", (rows, cols), F64), k.out("r_after", (rows, cols), F64), k.out("cls", (rows, cols), U8)
    rects = (C.c_int * 8)(0, rows // 2 + 1, 0, cols, rows // 2, rows, 1, cols - 1)
    k.call("rd_eval_classify", pred, init, 0, gt, 0, bits["gt_mask"], dil, bits["bnodata"], bits["water"], bits["forest"], rects, 2,
           rows, cols, -9999.0, rb, ra, cls)
    st = k.out("stats", 8, F64)
    ws, nb = k.ws("ws", lib.rd_residual_stats_ws_bytes(n), short=True)
    k.call("rd_residual_stats", pred, gt, bits["gt_mask"], n, -9999.0, 5.0, st, ws, nb, refuses_short=True)
    ns = 5
    sets = k.out("sets", (ns, 8), F64)
    ws2, nb2 = k.ws("ws2", lib.rd_residual_stats_sets_ws_bytes(n, ns))
    k.call("rd_residual_stats_sets", rb, ra, cls, n, (C.c_int * ns)(0, 1, 1, 0, 1), (C.c_int * ns)(1, 2, 2 | 4, 1 | 8, 2 | 32),
           (C.c_double * ns)(-1.0, -1.0, 5.0, 0.0, 5.0), ns, sets, ws2, nb2)

    def ref():
        import torch.nn.functional as Fn
        m = (bits["bmask"] != 0).float()[None, None]
        want = torch.zeros_like(m)
        for dy in range(-3, 4):                         # the L1 ball of radius 3
            for dx in range(-3 + abs(dy), 4 - abs(dy)):
                want = torch.maximum(want, torch.roll(Fn.pad(m, (3, 3, 3, 3)), (dy, dx), (2, 3))[..., 3:-3, 3:-3])
        assert torch.equal(dil != 0, want[0, 0] != 0)
        ok = (pred != -9999.0) & (gt.double() != -9999.0) & (bits["gt_mask"] != 0)
        r = (pred - gt.double())[ok]
        r = r[r.abs() <= 5.0]
        assert int(st[0]) == r.numel()
        if r.numel():
            assert abs(float(st[3]) - float(r.abs().mean())) <= 1e-12 * 5.0
            assert float(st[1]) == float(r.max()) and float(st[2]) == float(r.min())
        assert int(cls.max()) < 64
    k.ref(ref)


def c_sets_short(k, rows, cols):
    n, ns = rows * cols, 2
    rb = k.inp("r_before", (rows, cols), dtype=F64)
    cls = k.inp("cls", (rows, cols), fn=lambda: _randint(6, 64, rows, cols), dtype=U8)
    sets = k.out("sets", (ns, 8), F64)
    ws, nb = k.ws("ws", k.lib.rd_residual_stats_sets_ws_bytes(n, ns), short=True)
    k.call("rd_residual_stats_sets", rb, None, cls, n, (C.c_int * ns)(0, 0), (C.c_int * ns)(1, 2), (C.c_double * ns)(-1.0, 3.0), ns, sets,
           ws, nb, refuses_short=True)


# ---- the table --------------------------------------------------------------------------------------------------------------
CONV_SHAPES = [(1, 4, 4, 4, 4), (2, 8, 16, 8, 24), (3, 12, 20, 8, 24), (16, 64, 64, 24, 132), (2, 32, 32, 32, 132), (1, 6, 48, 32, 128),
               (2, 16, 32, 160, 32), (33, 8, 8, 64, 256), (1, 8, 8, 64, 64), (5, 8, 8, 128, 192), (2, 48, 80, 64, 128)]
CONVT_SHAPES = [(1, 2, 2, 4, 4), (2, 6, 10, 8, 12), (1, 5, 8, 32, 64), (1, 65, 70, 64, 128), (1, 67, 68, 128, 64), (5, 30, 32, 192, 64)]
SMALL_CONV = [(1, 4, 4, 4, 4), (3, 12, 20, 8, 24), (2, 32, 32, 32, 132), (33, 8, 8, 64, 256), (2, 16, 32, 64, 64)]
TAIL_ALL = ["rd_tail_compose", "rd_tail_t16", "rd_conv3x3_last_fwd_tail", "rd_convt_last_bwd_data", "rd_convt_last_bwd_weight",
            "rd_convt_last_bwd_weight_bn", "rd_conv3x3_last_bwd_tail_fused", "rd_tail_wl_finish", "rd_conv3x3_last_bwd_weight_tail"]


def _case(fn, args, covers, gemm=False, split_only=False, short=True):
    return dict(fn=fn, args=args, covers=covers, gemm=gemm, split_only=split_only, short=short,
                id=f"{fn.__name__[2:]}-" + re.sub(r"[^0-9A-Za-z]+", "_", "x".join(str(a) for a in args)).strip("_"))


CASES = []
for s_ in CONV_SHAPES:
    CASES.append(_case(c_conv3x3, s_, ["rd_pack_conv3x3_weight", "rd_conv3x3_fwd", "rd_conv3x3_bwd_data", "rd_conv3x3_bwd_weight",
                                        "rd_mfma_products", "rd_packed_weight_bytes"], gemm=True))
for s_ in SMALL_CONV:
    CASES.append(_case(c_conv3x3_stats, s_, ["rd_conv3x3_fwd_stats"], gemm=True))
    CASES.append(_case(c_conv3x3_bn, s_, ["rd_conv3x3_fwd_bn"], gemm=True))
    CASES.append(_case(c_conv3x3_act, s_, ["rd_pack_conv3x3_weight_folded", "rd_conv3x3_fwd_act"], gemm=True, split_only=True, short=False))
    CASES.append(_case(c_conv3x3_dgrad_bnstats, s_, ["rd_conv3x3_bwd_data_bnstats", "rd_bn_bwd_part_floats"],
                       gemm=True))
CASES.append(_case(c_conv3x3_dgrad_bnstats, (2, 16, 32, 64, 64, 2), ["rd_conv3x3_bwd_data_bnstats"], gemm=True))
for s_ in CONVT_SHAPES:
    CASES.append(_case(c_convt, s_, ["rd_pack_convt2x2_weight", "rd_convt2x2_fwd", "rd_convt2x2_bwd_data", "rd_convt2x2_bwd_weight"], gemm=True))
for s_ in [(1, 2, 2, 4, 4), (2, 6, 10, 8, 12), (1, 5, 8, 32, 64), (2, 16, 16, 64, 64)]:
    CASES.append(_case(c_convt_bn, s_, ["rd_convt2x2_fwd_bnskip", "rd_convt2x2_bwd_data_bnstats"], gemm=True))
for s_ in [(2, 6, 10, 8, 12), (1, 5, 8, 32, 64), (3, 7, 9, 64, 16), (1, 1, 1, 4, 4)]:
    CASES.append(_case(c_conv1x1, s_, ["rd_pack_conv1x1_weight", "rd_conv1x1_fwd", "rd_conv1x1_bwd_data", "rd_conv1x1_bwd_weight"], gemm=True))
CASES.append(_case(c_pack_fused, ([(0, 24, 8), (0, 64, 32), (1, 12, 8), (1, 32, 64), (0, 132, 32)],), ["rd_pack_weights_fused"], gemm=True,
                   split_only=True, short=False))
for s_ in [(1, 16, 16, 1, 4), (3, 8, 64, 2, 64), (2, 9, 13, 5, 12)]:
    CASES.append(_case(c_first, s_, ["rd_conv3x3_first_fwd", "rd_conv3x3_first_bwd_weight"]))
    CASES.append(_case(c_first_stats, s_, ["rd_conv3x3_first_fwd_stats"]))
    CASES.append(_case(c_first_bn, s_, ["rd_conv3x3_first_fwd_bn"]))
for s_ in [(2, 16, 32, 1, 32), (3, 32, 96, 3, 64)]:
    CASES.append(_case(c_first_act, s_, ["rd_conv3x3_first_fwd_act", "rd_conv3x3_first_bwd_weight_bn"]))
for s_ in [(1, 16, 16, 4, 1), (2, 9, 13, 12, 3), (2, 32, 32, 16, 3), (1, 36, 20, 64, 2), (3, 4, 4, 16, 1)]:
    CASES.append(_case(c_last, s_, ["rd_conv3x3_last_fwd", "rd_conv3x3_last_bwd_data", "rd_conv3x3_last_bwd_weight",
                                    "rd_conv3x3_last_bwd_data_bnstats"]))
CASES.append(_case(c_last_part_short, (1, 36, 20, 64), ["rd_conv3x3_last_bwd_data_bnstats"]))
for s_ in [(2, 32, 32, 16, 16), (1, 36, 20, 32, 16), (3, 4, 4, 16, 16), (2, 16, 16, 256, 64)]:
    CASES.append(_case(c_tail, s_, TAIL_ALL))
for w_, f_ in (("dgrad", "rd_convt_last_bwd_data"), ("wgrad_bn", "rd_convt_last_bwd_weight_bn"),
               ("fused", "rd_conv3x3_last_bwd_tail_fused"), ("wl_tail", "rd_conv3x3_last_bwd_weight_tail")):
    CASES.append(_case(c_tail_short, (w_, 1, 36, 20, 32, 16), [f_]))
for s_ in [(1, 0, 4), (7, 3, 12), (40, 33, 132)]:
    CASES.append(_case(c_bn_finalize, s_, ["rd_bn_bwd_stats_finalize"], short=False))
for s_ in [(3, 8, 8, 8, True), (1, 5, 7, 12, False), (2, 16, 32, 64, True), (2, 6, 10, 132, True), (1, 1, 1, 4, False)]:
    CASES.append(_case(c_bn_act, s_, ["rd_bn_act_pool_fwd", "rd_bn_act_bwd_reduce", "rd_bn_act_bwd_apply"]))
for s_ in [(1, 1, 2, 4), (3, 5, 7, 12), (2, 32, 32, 132)]:
    CASES.append(_case(c_bn_stats, s_, ["rd_bn_stats_partial", "rd_bn_stats_finalize", "rd_bn_eval_stats", "rd_channel_sum"]))
CASES.append(_case(c_channel_sum_short, (3, 5, 7, 12), ["rd_channel_sum"]))
for s_ in [(1, 1, 1), (3, 17, 23), (2, 64, 64)]:
    CASES.append(_case(c_masked_l1, s_, ["rd_masked_l1_partial", "rd_masked_l1_finish"]))
for s_ in [(1, 1, 1, 4), (3, 4, 16, 12), (1, 2, 1, 8), (2, 5, 7, 132)]:
    CASES.append(_case(c_upsample, s_, ["rd_upsample2x_add_fwd", "rd_upsample2x_bwd"], short=False))
for s_ in [(1, 1, 1, 1), (2, 3, 5, 7), (3, 64, 9, 11)]:
    CASES.append(_case(c_layout, s_, ["rd_nchw_to_nhwc", "rd_nhwc_to_nchw"], short=False))
for s_ in [(1,), (1023,), (70001,)]:
    CASES.append(_case(c_optim, s_, ["rd_adam_step", "rd_adam_step_dev", "rd_sgd_step"], short=False))
for s_ in [(1,), (4099,)]:
    CASES.append(_case(c_zero_copy, s_, ["rd_zero", "rd_copy_segments", "rd_amax"], short=False))
for s_ in [(3, 16, 8, 33, 41), (70, 8, 4, 45, 37)]:
    CASES.append(_case(c_blend, s_, ["rd_blend_accumulate"], short=False))
for s_ in [(5, 8, 37, 45, 2), (3, 12, 13, 29, 1)]:
    CASES.append(_case(c_patches, s_, ["rd_patch_sums", "rd_assemble_patches"], short=False))
for s_ in [(4, 8, 37, 45, 2, 2), (3, 16, 33, 19, 1, 1), (2, 8, 9, 11, 2, 0)]:
    CASES.append(_case(c_grid_tiles, s_, ["rd_assemble_grid_tiles"], short=(s_[5] == 2)))
for s_ in [(6, 8, 2), (5, 12, 1)]:
    CASES.append(_case(c_train_patches, s_, ["rd_assemble_train_patches"], short=False))
for s_ in [(5, 8, 37, 45), (3, 20, 21, 23)]:
    CASES.append(_case(c_moments, s_, ["rd_patch_moments", "rd_region_moments"]))
CASES.append(_case(c_region_short, (37, 45), ["rd_region_moments"]))
for s_ in [(37, 45), (5, 3)]:
    CASES.append(_case(c_eval, s_, ["rd_dilate_mask", "rd_eval_classify", "rd_residual_stats", "rd_residual_stats_sets"]))
CASES.append(_case(c_sets_short, (37, 45), ["rd_residual_stats_sets"]))

MODES = {"default": {}, "products6": {"mfma_products": 6}, "f32": {"mfma_f32": 1}}
# functions that take no device pointer they write through (the ledger test refuses anything else here)
EXEMPT = {
    "rd_version": "returns a number",
    "rd_last_error_string": "returns a host string",
    "rd_quant_next": "host-side registration of slots; the slots are written by the NEXT call, which the table covers",
    "rd_quant_next_img": "host-side registration of slots, as rd_quant_next",
    "rd_pack_item_pieces": "size query",
    "rd_pack_item_tiles": "size query",
    "rd_set_splitk_workspace": "registration; the launches that use it are in test_split_k_scratch_stays_inside_its_registration",
    "rd_host_register": "host memory", "rd_host_unregister": "host memory", "rd_copy_to_host_async": "writes host memory",
    "rd_conv3x3_last_bwd_tail_blocks": "size query",
    "rd_conv3x3_first_fwd_act_available": "shape query", "rd_conv3x3_first_bwd_weight_bn_available": "shape query",
    "rd_tail_available": "shape query",
}
EXEMPT_PATTERNS = [r"rd_tune_\w+", r"rd_prof_\w+", r"rd_plan_\w+", r"rd_\w+_ws_bytes"]
ALLOWED_EXEMPT = [r"rd_version", r"rd_tune_\w+", r"rd_prof_\w+", r"rd_plan_\w+", r"rd_last_error_string",
                  r"rd_quant_next\w*", r"rd_\w+_ws_bytes", r"rd_\w+_available", r"rd_\w+_blocks", r"rd_pack_item_\w+",
                  r"rd_host_register", r"rd_host_unregister",
                  r"rd_copy_to_host_async", r"rd_set_splitk_workspace"]


# ---- fixtures and drivers ---------------------------------------------------------------------------------------------------
@pytest.fixture()
def lib():
    from resdepth_amd import _lib
    handle = _lib.load()
    names = ["mfma_products", "mfma_f32", "last_blocks", "rows_blocks", "tn_blocks", "tn_tile", "wg_strip", "wg_blocks",
             "wg_minblocks", "convt_patch", "edge_conv"]
    before = {n_: _lib.tune_get(n_) for n_ in names}
    yield handle
    for n_, v in before.items():
        _lib.tune_set(n_, v)


def _set_mode(mode):
    from resdepth_amd import _lib
    for name, v in MODES[mode].items():
        _lib.tune_set(name, v)


def _run_case(lib, case, **kw):
    sizing = K(lib)
    case["fn"](sizing, *case["args"])
    k = K(lib, sizes=sizing.sizes, **kw)
    try:
        case["fn"](k, *case["args"])
    except _Stop:
        k.arena.check()
        return k, None
    return k, k.finish()


def _full(lib, case):
    k, a = _run_case(lib, case, fill="sentinel", with_wrapper=True)
    stale = set(case["covers"]) - k.called
    assert not stale, f"{case['id']} lists entry points it never calls: {sorted(stale)}"
    _, b = _run_case(lib, case, fill="ff")
    _, c = _run_case(lib, case, fill="zero", shifted=True)
    for name in a:
        assert torch.equal(a[name], b[name]), f"{name}: result depends on what the output / scratch held before (0xFF fill)"
        assert torch.equal(a[name], c[name]), f"{name}: result depends on prior contents or on the allocation's offset (zero fill, shifted)"


def _params():
    out = []
    for case in CASES:
        for mode in (MODES if case["gemm"] else ["default"]):
            if case["split_only"] and mode == "f32":
                continue
            out.append(pytest.param(case, mode, id=f"{case['id']}-{mode}"))
    return out


@pytest.mark.parametrize("case,mode", _params())
def test_memory_contract(lib, case, mode):
    _set_mode(mode)
    _full(lib, case)


@pytest.mark.parametrize("case", [pytest.param(c, id=c["id"]) for c in CASES if c["short"]])
def test_undersized_scratch_is_refused_and_nothing_is_written(lib, case):
    k, res = _run_case(lib, case, fill="sentinel", short=True)
    assert k.short_seen and res is None, "the case never reached its undersized call"


KNOB_CASES = [
    ("last_blocks", (64, 300), _case(c_last, (2, 32, 32, 16, 3), [])),
    ("last_blocks", (64, 300), _case(c_last, (2, 9, 13, 12, 3), [])),
    ("rows_blocks", (7, 1024), _case(c_bn_stats, (2, 32, 32, 132), [])),
    ("rows_blocks", (7, 1024), _case(c_bn_act, (2, 16, 32, 64, True), [])),
    ("tn_blocks", (16, 2048), _case(c_conv3x3, (2, 32, 32, 32, 132), [])),
    ("tn_blocks", (16, 2048), _case(c_conv1x1, (3, 7, 9, 64, 16), [])),
    ("tn_blocks", (16, 2048), _case(c_convt, (1, 65, 70, 64, 128), [])),
    ("tn_blocks", (16, 2048), _case(c_conv3x3, (3, 12, 20, 8, 24), [])),
    ("tn_tile", (64064, 128128), _case(c_conv3x3, (3, 12, 20, 8, 24), [])),
    ("tn_tile", (64064, 128128), _case(c_conv3x3, (2, 32, 32, 32, 132), [])),
    ("tn_tile", (64064, 128128), _case(c_conv1x1, (3, 7, 9, 64, 16), [])),
    ("tn_tile", (64064, 128128), _case(c_convt, (1, 65, 70, 64, 128), [])),
    ("wg_minblocks", (1, 100000), _case(c_conv3x3, (2, 48, 80, 64, 128), [])),
    ("wg_blocks", (16, 4096), _case(c_conv3x3, (2, 48, 80, 64, 128), [])),
    ("wg_strip", (0, -1), _case(c_conv3x3, (2, 48, 80, 64, 128), [])),
    ("wg_strip", (0, 4, -1), _case(c_conv3x3, (33, 8, 8, 64, 256), [])),
    ("convt_patch", (0, -1), _case(c_convt, (5, 30, 32, 192, 64), [])),
    ("edge_conv", (0, -1), _case(c_first, (3, 8, 64, 2, 64), [])),
    ("edge_conv", (0, -1), _case(c_first_stats, (3, 8, 64, 2, 64), [])),
    ("edge_conv", (0, -1), _case(c_last, (2, 32, 32, 16, 3), [])),
]


@pytest.mark.parametrize("knob,values,case", [pytest.param(a, b, c, id=f"{a}-{c['id']}") for a, b, c in KNOB_CASES])
def test_scratch_queries_that_depend_on_a_knob(lib, knob, values, case):
    """query and call under the same knob value, at two values: the query must follow the knob the launch reads"""
    from resdepth_amd import _lib
    for v in values:
        _lib.tune_set(knob, v)
        _full(lib, case)
        k, res = _run_case(lib, case, fill="sentinel", short=True)
        assert k.short_seen and res is None


def test_tail_head_statistics_rows_are_not_what_the_generic_query_counts(lib):
    """rd_conv3x3_last_bwd_tail_fused writes one row per 16 x 32 image tile: for images smaller than 64 pixels that is more than
    rd_bn_bwd_part_floats(pixels, C) holds, so `part` is sized by rd_conv3x3_last_bwd_tail_blocks (the header says so)."""
    n, h, w, c = 3, 4, 4, 16
    assert lib.rd_conv3x3_last_bwd_tail_blocks(n, h, w) * 4 * c > lib.rd_bn_bwd_part_floats(n * h * w, c)


@pytest.mark.parametrize("n,cin,cout", [(33, 128, 192), (16, 256, 64), (2, 512, 512)])
def test_split_k_scratch_stays_inside_its_registration(lib, n, cin, cout):
    from resdepth_amd import _lib, ops
    nbytes = _lib.SPLITK_BYTES
    sizing = K(lib)
    c_conv3x3(sizing, n, 8, 8, cin, cout)
    ar = Arena(DEV, sizing.sizes + [nbytes])
    sk = ar.alloc(nbytes, U8, kind="scratch", name="splitk")
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.rd_set_splitk_workspace(sk.data_ptr(), nbytes, stream), "set_splitk_workspace")
    try:
        torch.cuda.synchronize()
        tickets = sk[:64 << 10]                      # the first 64 KB of the registration
        assert int(tickets.sum()) == 0, "the registration leaves the tickets zero"
        g = torch.Generator(device=DEV).manual_seed(3)
        x = ar.alloc((n, 8, 8, cin), F32, fill=torch.randn(n, 8, 8, cin, generator=g, device=DEV), name="x")
        dz = ar.alloc((n, 8, 8, cout), F32, fill=torch.randn(n, 8, 8, cout, generator=g, device=DEV), name="dz")
        wt = torch.randn(cout, cin, 3, 3, generator=g, device=DEV) * 0.1
        wf, wd = ops.pack_conv3x3_weight(wt)
        z, dx = ar.alloc((n, 8, 8, cout), F32, name="z"), ar.alloc((n, 8, 8, cin), F32, name="dx")
        for _ in range(2):
            _lib.check(lib.rd_conv3x3_fwd(x.data_ptr(), wf.data_ptr(), z.data_ptr(), n, 8, 8, cin, cout, stream), "fwd")
            ar.check()
            assert int(tickets.sum()) == 0, "forward: tickets not left zero"
            _lib.check(lib.rd_conv3x3_bwd_data(dz.data_ptr(), wd.data_ptr(), dx.data_ptr(), n, 8, 8, cin, cout, stream), "dgrad")
            ar.check()
            assert int(tickets.sum()) == 0, "data gradient: tickets not left zero"
        assert ar.unwritten(z) == 0 and ar.unwritten(dx) == 0
        with_ws = (z.clone(), dx.clone())
    finally:
        _lib.check(lib.rd_set_splitk_workspace(None, 0, stream), "set_splitk_workspace")
    # "the same bits with or without a registration"
    assert torch.equal(ops.conv3x3_fwd(x, wf), with_ws[0]) and torch.equal(ops.conv3x3_bwd_data(dz, wd), with_ws[1])


def test_planted_overrun_on_the_device_is_reported():
    ar = Arena(DEV, [4096, 4096])
    a = ar.alloc(1000, F32, fill=torch.arange(1000.0), name="a")
    out = ar.alloc(1000, F32, name="out")
    out.copy_(a)
    ar.check()
    rec = ar.find("out")
    ar.raw[rec.start:rec.end + 4].view(F32)[-1:].fill_(1.0)          # one element past the end, inside the arena
    with pytest.raises(ArenaError) as e:
        ar.check()
    assert (e.value.name, e.value.side, e.value.offset) == ("out", "after", 0)


def _exported():
    text = open(os.path.join(ROOT, "include", "resdepth_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rd_\w+)\s*\(", text)))


def test_every_exported_function_has_a_case_or_a_reason():
    ledger_check()


def ledger_check():
    """the ledger (no GPU work; tests/test_arena_cpu.py runs it in the CPU suite too): a new entry point cannot arrive without a
    memory-contract case; test_memory_contract holds every case to the entry points its `covers` list names"""
    from resdepth_amd import _lib
    exported = _exported()
    assert set(exported) == set(_lib.SIGNATURES), set(exported) ^ set(_lib.SIGNATURES)
    covered = {f for c in CASES for f in c["covers"]}
    assert covered <= set(exported), covered - set(exported)
    for f in EXEMPT:
        assert f in exported, f"EXEMPT names {f}, which the header does not export"
        assert f not in covered, f"{f} is both covered and exempt"
    for name in EXEMPT:
        assert any(re.fullmatch(a, name) for a in ALLOWED_EXEMPT), \
            f"{name} may not be exempt: only functions that write through no device pointer"
    for pat in EXEMPT_PATTERNS:
        assert pat in ALLOWED_EXEMPT, f"{pat} may not be exempt"
    missing = [f for f in exported if f not in covered and f not in EXEMPT and not any(re.fullmatch(p, f) for p in EXEMPT_PATTERNS)]
    assert not missing, f"exported functions without a memory-contract case or an exemption: {missing}"
