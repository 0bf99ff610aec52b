"""The two forms of the statistics-set engine of rd_stats.hip at the C ABI: rd_residual_stats_sets over one of two sources and
rd_residual_stats_pooled over one plane of a strided buffer share the moments accumulator, the radix select and the launch
schedule, so on the same values they give the same BITS in all eight columns (both add in the same order), NaNs of an empty
set included.

Sizes: one moments block (256 values) and one more; one histogram round (512 threads x 8 values) and one more; one value past
the 1024-block grid cap of the moments kernel, so its grid-stride second round runs."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SIZES = [1, 255, 257, 4095, 4097, 1024 * 4096 + 1]
SETS = [(1, -1.0), (1 | 8, 1.0), (2, -1.0)]            # (need bits, threshold or none)
PAD = 3                                                # the planes lie n + 3 doubles apart


def _source(rng, n):
    """seeded Laplace draw, a tenth of it duplicates, with +0.0, -0.0 and one repeated negative value planted"""
    a = rng.laplace(size=n)
    dup = rng.randint(0, n, size=n // 10)
    a[dup] = a[rng.randint(0, n, size=n // 10)]
    for k, v in enumerate((0.0, -0.0, -1.25, -1.25, -1.25)):
        if k < n:
            a[(k * 37) % n] = v
    return a


def _call_sets(lib, L, a, b, cls, src):
    n, ns = cls.numel(), len(SETS)
    out = torch.empty((ns, 8), dtype=torch.float64, device=cls.device)
    ws = torch.empty(lib.rd_residual_stats_sets_ws_bytes(n, ns), dtype=torch.uint8, device=cls.device)
    L.check(lib.rd_residual_stats_sets(L.ptr(a), L.ptr(b), L.ptr(cls), n, (C.c_int * ns)(*[src] * ns),
                                       (C.c_int * ns)(*[s[0] for s in SETS]), (C.c_double * ns)(*[s[1] for s in SETS]), ns,
                                       L.ptr(out), ws.data_ptr(), ws.numel(), L.stream_ptr()), "residual_stats_sets")
    return out.cpu().numpy().view(np.int64)


def _call_pooled(lib, L, planes, n, p, cls, valid):
    ns = len(SETS)
    out = torch.empty((ns, 8), dtype=torch.float64, device=cls.device)
    ws = torch.empty(lib.rd_residual_stats_pooled_ws_bytes(n, ns), dtype=torch.uint8, device=cls.device)
    L.check(lib.rd_residual_stats_pooled(L.ptr(planes), n + PAD, 2, p, p + 1, L.ptr(cls), L.ptr(valid), n,
                                         (C.c_int * ns)(*[s[0] for s in SETS]), (C.c_double * ns)(*[s[1] for s in SETS]), ns,
                                         L.ptr(out), ws.data_ptr(), ws.numel(), L.stream_ptr()), "residual_stats_pooled")
    return out.cpu().numpy().view(np.int64)


@pytest.mark.parametrize("n", SIZES)
def test_sets_and_pooled_forms_give_the_same_bits(n):
    from resdepth_amd import _lib as L
    lib = L.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.RandomState(n % 9973)
    a, b = _source(rng, n), _source(rng, n)
    buf = np.full(2 * n + PAD, 1e300)                  # the padding between the planes must never be read
    buf[:n], buf[n + PAD:] = a, b
    cls = torch.from_numpy(rng.randint(0, 16, size=n).astype(np.uint8)).to(dev)
    ta, tb, planes = (torch.from_numpy(x).to(dev) for x in (a, b, buf))
    ones = torch.full((n,), -1, dtype=torch.int16, device=dev)                       # 0xFFFF: every plane valid
    with torch.cuda.device(dev):
        for p in (0, 1):
            sets = _call_sets(lib, L, ta, tb, cls, p)
            pooled = _call_pooled(lib, L, planes, n, p, cls, None)
            assert sets.shape == (len(SETS), 8)
            np.testing.assert_array_equal(sets, pooled, err_msg=f"source {p} against plane {p}")
            np.testing.assert_array_equal(_call_pooled(lib, L, planes, n, p, cls, ones), pooled,
                                          err_msg=f"plane {p}: an all-ones validity word against none")
    got = sets.view(np.float64)
    assert got[0, 0] == float(((cls.cpu().numpy() & 1) == 1).sum())                  # the calls did count something
