"""rd_grad_norm on the GPU (-m gpu): against fp64 numpy, bit-identical between an aligned and a misaligned buffer and between two
runs, non-finite elements counted and left out of the sum."""
import os
import re

import numpy as np
import pytest
import torch

import optim_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_D = {k: int(v) for k, v in re.findall(r"#define\s+(RD_\w+)\s+(\d+)", open(os.path.join(ROOT, "include", "resdepth_hip_optim.h")).read())}
VEC = _D["RD_GNORM_VEC"]
SHARE = _D["RD_GNORM_BLOCK"] * VEC                  # elements of one block
WRAP = _D["RD_GNORM_MAX_BLOCKS"] * SHARE            # span of the capped grid
# as tests/test_optim_contract_gpu.py; past 4 * WRAP the loop that keeps four chunks in flight runs
SIZES = [1, 3, 255, 256, 257, VEC - 1, VEC, VEC + 1, SHARE + 1, WRAP + 1, 4 * WRAP + 1, 9 * WRAP + 3]


def _randn(n, seed, scale=1.0):
    return (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale).numpy()


def _misaligned(a):
    """the same values in a device buffer that starts one float past a 16-byte boundary"""
    t = torch.empty(a.size + 1, device=DEV, dtype=torch.float32)
    assert t.data_ptr() % 16 == 0
    t[1:].copy_(torch.from_numpy(a))
    return t[1:]


@pytest.mark.parametrize("bad", [False, True], ids=["finite", "nonfinite"])
@pytest.mark.parametrize("n", SIZES)
def test_grad_norm_against_fp64(n, bad):
    from resdepth_amd import ops
    g = _randn(n, n, 3.0)
    if bad and n >= 3:
        g[0] = np.inf                         # counted, and left out of the sum
        g[n - 1] = np.nan
    want_sum, want_bad = optim_ref.grad_stats(g)
    assert want_bad == (2 if bad and n >= 3 else 0)
    ga = torch.from_numpy(g).to(DEV)
    assert ga.data_ptr() % 16 == 0
    a = ops.grad_norm(ga).cpu().numpy()
    b = ops.grad_norm(_misaligned(g)).cpu().numpy()
    c = ops.grad_norm(ga).cpu().numpy()
    # n <= 2^26 exact fp64 squares: worst-case relative summation error n * 2^-53 < 8e-9
    np.testing.assert_allclose(a[0], want_sum, rtol=1e-8)
    assert a[1] == want_bad
    assert a.tobytes() == b.tobytes(), "the float4 and the element-wise form differ"
    assert a.tobytes() == c.tobytes(), "two runs differ"
    # the norm on the device, no read-back in between: within one fp32 ulp of fl32(sqrt(sum))
    norm = ops.grad_norm(ga)[0].sqrt().float()
    want = np.float32(np.sqrt(want_sum))
    assert norm.is_cuda and abs(float(norm) - float(want)) <= float(np.spacing(want))


def test_a_scratch_of_the_callers_own_and_the_refusals():
    from resdepth_amd import _lib, ops
    lib = _lib.load()
    n = SHARE + 1
    g = torch.from_numpy(_randn(n, 5)).to(DEV)
    ws = torch.empty(lib.rd_grad_norm_ws_bytes(n), device=DEV, dtype=torch.uint8)
    stats = torch.zeros(2, device=DEV, dtype=torch.float64)
    assert ops.grad_norm(g, stats, ws) is stats
    assert torch.equal(stats, ops.grad_norm(g))
    with pytest.raises(RuntimeError, match="workspace too small"):
        ops.grad_norm(g, stats, ws[:-1])
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.grad_norm(torch.zeros(4))
