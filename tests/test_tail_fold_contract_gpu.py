"""The memory contract of include/resdepth_hip.h for the two entry points of include/resdepth_hip_tail.h: the guard-band cases
that tests/test_memory_contract_gpu.py runs for every entry point of the main header (its driver and judgement are used as they
are) on ragged tiles for each of the three channel counts, and the ledger over the side header: an entry point cannot arrive
there without a case here.  Neither entry point takes scratch, so there is no undersized-scratch case.

This module leans on that file's helpers (_case, _full, _bn, _ops and the Case methods inp / out / slot / quant / call / wrapper),
as tests/test_optim_contract_gpu.py does; test_the_borrowed_helpers_are_there names what is used."""
import os
import re

import pytest

import test_memory_contract_gpu as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_borrowed_helpers_are_there():
    for name in ("_case", "_full", "_bn", "_ops", "U8"):
        assert hasattr(T, name), name
    for name in ("inp", "out", "slot", "quant", "call", "wrapper"):
        assert hasattr(T.K, name), name


def c_tail_fold(k, n, h, w, c0):
    """level 0's pool pass with the skip term, then the rest of the tail from it; (n, h, w) is the full resolution.  The slot of
    the pooled tensor is zeroed by the caller and compared like an output."""
    ops = T._ops()
    hc, wc = h // 2, w // 2
    z0, b0 = k.inp("z0", (n, h, w, c0)), T._bn(k, "bn0", c0)
    wl, bl = k.inp("w_last", (1, c0, 3, 3), scale=0.1), k.inp("bias", 1)
    t16, b9, x0 = k.inp("t16", (n, hc, wc, 16)), k.inp("b9", 9, scale=0.1), k.inp("x_nchw", (n, 3, h, w))
    pooled, idx, zpool = k.out("pooled", (n, hc, wc, c0)), k.out("idx", (n, hc, wc, c0), T.U8), k.out("zpool", (n, hc, wc, c0))
    skip9 = k.out("skip9", (n, h, w))
    sp = k.slot("pooled_amax") if k.three else None
    k.quant(out2=sp)
    k.call("rd_bn_act_pool_fwd_tailskip", z0, *b0, 0.01, None, wl, pooled, idx, zpool, skip9, n, h, w, c0)
    out = k.out("out", (n, 1, h, w))
    k.call("rd_conv3x3_last_fwd_tail_pre", skip9, t16, b9, bl, x0, 3, out, n, h, w)

    def wrap():
        p, i, zp, s9 = ops.bn_act_pool_fwd_tailskip(z0, *b0, 0.01, wl, want_zpool=True)
        return {"pooled": p, "idx": i, "zpool": zp, "skip9": s9, "out": ops.conv3x3_last_fwd_tail_pre(s9, t16, b9, bl, x0)}
    k.wrapper(wrap)


ALL = ["rd_bn_act_pool_fwd_tailskip", "rd_conv3x3_last_fwd_tail_pre"]
# ragged 16 x 32 tiles in both directions for each lane count (C0 = 64 / 32 / 16), and the smallest image there is
CASES = [T._case(c_tail_fold, s_, ALL, short=False) for s_ in [(2, 34, 66, 64), (1, 18, 34, 32), (3, 20, 36, 16), (1, 2, 2, 16)]]


@pytest.fixture()
def lib():
    from resdepth_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("case", [pytest.param(c, id=c["id"]) for c in CASES])
def test_memory_contract(lib, case):
    T._full(lib, case)


def test_bad_shapes_are_refused_and_nothing_is_written(lib):
    """an odd height, a channel count outside {16, 32, 64}: RD_ERR_ARG, a message, no launch"""
    import torch
    dev = "cuda:0"
    z = torch.zeros(1, 6, 6, 64, device=dev)
    v = torch.ones(64, device=dev)
    outs = [torch.full((1, 3, 3, 64), 7.0, device=dev), torch.full((1, 3, 3, 64), 7, device=dev, dtype=torch.uint8),
            torch.full((1, 6, 6), 7.0, device=dev)]
    wl = torch.zeros(1, 64, 3, 3, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()                                                                         # noqa: E731
    for h, w, c in ((5, 6, 64), (6, 6, 24), (6, 5, 64)):
        rc = lib.rd_bn_act_pool_fwd_tailskip(p(z), p(v), p(v), p(v), p(v), 0.0, None, p(wl), p(outs[0]), p(outs[1]), None,
                                             p(outs[2]), 1, h, w, c, s)
        assert rc != 0 and lib.rd_last_error_string()
    rc = lib.rd_conv3x3_last_fwd_tail_pre(p(outs[2]), p(z), p(v), None, None, 0, p(outs[2]), 1, 5, 6, s)
    assert rc != 0 and lib.rd_last_error_string()
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in outs)


def test_every_function_of_the_side_header_has_a_case():
    from resdepth_amd import _lib
    text = open(os.path.join(ROOT, "include", "resdepth_hip_tail.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    exported = set(re.findall(r"\b(rd_\w+)\s*\(", text))
    assert exported == set(_lib.SIGNATURES_TAIL)
    covered = {f for c in CASES for f in c["covers"]}
    assert covered == exported, covered ^ exported
