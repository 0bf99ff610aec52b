"""The gradient statistics of include/resdepth_hip_optim.h without a GPU: the oracle of tests/optim_ref.py against torch's own
clip_grad_norm_, and the side header against _lib.SIGNATURES_OPTIM and the library."""
import os
import re

import numpy as np
import torch

import optim_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_oracle_is_torchs_total_norm():
    for seed, n in ((0, 1), (1, 257), (2, 70001)):
        g = (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 3.0)
        p = torch.nn.Parameter(torch.zeros(n))
        p.grad = g.clone()
        total = float(torch.nn.utils.clip_grad_norm_([p], 1e30))       # fp32 reduction inside torch: 1e-6 is its own error
        s, bad = optim_ref.grad_stats(g.numpy())
        assert bad == 0
        np.testing.assert_allclose(np.sqrt(s), total, rtol=1e-6)
    g = g.numpy().copy()
    g[0], g[-1] = np.inf, np.nan
    s2, bad = optim_ref.grad_stats(g)
    assert bad == 2 and np.isfinite(s2) and s2 < s


def _side_header():
    text = open(os.path.join(ROOT, "include", "resdepth_hip_optim.h")).read()
    return text, re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def test_side_header_signatures_constants_and_version():
    from resdepth_amd import _lib
    main = open(os.path.join(ROOT, "include", "resdepth_hip.h")).read()
    assert '#include "resdepth_hip_optim.h"' in main
    assert "rd_grad_norm" not in re.sub(r'#include "resdepth_hip_optim.h".*', "", main)
    _, code = _side_header()
    exported = set(re.findall(r"\b(rd_\w+)\s*\(", code))
    assert exported == set(_lib.SIGNATURES_OPTIM) == {"rd_grad_norm_ws_bytes", "rd_grad_norm"}
    defines = {k: int(v) for k, v in re.findall(r"#define\s+(RD_\w+)\s+(\d+)", code)}
    assert (defines["RD_GNORM_BLOCK"], defines["RD_GNORM_VEC"], defines["RD_GNORM_MAX_BLOCKS"]) == \
        (_lib.GNORM_BLOCK, _lib.GNORM_VEC, _lib.GNORM_MAX_BLOCKS)
    lib = _lib.load()
    assert lib.rd_version() >= 115
    # the scratch query is host arithmetic: one {sum, count} pair of fp64 per block, the grid a function of numel alone, capped
    per_block = _lib.GNORM_BLOCK * _lib.GNORM_VEC
    assert lib.rd_grad_norm_ws_bytes(0) == 0 and lib.rd_grad_norm_ws_bytes(-5) == 0
    assert lib.rd_grad_norm_ws_bytes(1) == lib.rd_grad_norm_ws_bytes(per_block) == 16
    assert lib.rd_grad_norm_ws_bytes(per_block + 1) == 32
    assert lib.rd_grad_norm_ws_bytes(per_block * _lib.GNORM_MAX_BLOCKS + 1) == lib.rd_grad_norm_ws_bytes(1 << 40) == \
        16 * _lib.GNORM_MAX_BLOCKS


def test_the_new_unit_is_built_and_launches_through_rd_launch():
    csrc = os.path.join(ROOT, "resdepth_amd", "csrc")
    build = open(os.path.join(csrc, "build.sh")).read()
    units = re.search(r'^UNITS="([^"]*)"$', build, re.M).group(1).split()
    assert "rd_optim" in units and "resdepth_hip_optim.h" in build
    src = open(os.path.join(csrc, "rd_optim.hip")).read()
    assert "RD_LAUNCH(" in src and "hipLaunchKernelGGL" not in src and "<<<" not in src and "atomicAdd" not in src
