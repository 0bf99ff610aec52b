"""The optimizer oracles of tests/optim_ref.py without a GPU: the gradient statistics against torch's own clip_grad_norm_, the
Adam and SGD steps against torch.optim.Adam / torch.optim.SGD in fp64 (per-parameter step counts included), the error bound of
tests/test_optim_steps_gpu.py on an fp32 emulation of the kernels, and the side header against _lib.SIGNATURES_OPTIM and the
library."""
import os
import re

import numpy as np
import pytest
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


# ---- the step oracles against torch in fp64 ------------------------------------------------------------------------------------
STEPS = 6
LATE = 3          # the second parameter has no gradient for this many steps


def _fp64_problem(seed):
    g = torch.Generator().manual_seed(seed)
    shapes = [(5, 7), (33,)]
    ps = [torch.nn.Parameter(torch.randn(s, generator=g, dtype=torch.float64)) for s in shapes]
    grads = [[torch.randn(s, generator=g, dtype=torch.float64) * 3.0 for s in shapes] for _ in range(STEPS)]
    return ps, grads


@pytest.mark.parametrize("kw", [dict(lr=1e-3), dict(lr=2e-4, weight_decay=1e-5), dict(lr=1e-2, betas=(0.0, 0.99), weight_decay=1e-2),
                                dict(lr=1e-3, eps=1e-3, weight_decay=1e-2)])
def test_the_adam_oracle_is_torch_adam_in_fp64_with_one_step_count_per_parameter(kw):
    ps, grads = _fp64_problem(3)
    opt = torch.optim.Adam(ps, foreach=False, **kw)
    mine = [dict(p=p.detach().numpy().copy(), m=np.zeros(p.shape), v=np.zeros(p.shape), t=0) for p in ps]
    gs = 0.25           # torch has no grad_scale: it steps on the scaled gradient, the oracle scales the raw one
    for it in range(STEPS):
        before = ps[1].detach().clone()
        for i, (p, st) in enumerate(zip(ps, mine)):
            if i == 1 and it < LATE:
                p.grad = None
                continue
            p.grad = grads[it][i] * gs
            st["t"] += 1
            sc = optim_ref.adam_scalars(kw["lr"], kw.get("betas", (0.9, 0.999)), kw.get("eps", 1e-8), kw.get("weight_decay", 0.0),
                                        st["t"], gs, rounded=False)
            st["p"], st["m"], st["v"] = optim_ref.adam_step(st["p"], grads[it][i].numpy(), st["m"], st["v"], sc)
        opt.step()
        for p, st in zip(ps, mine):
            np.testing.assert_allclose(st["p"], p.detach().numpy(), rtol=1e-12, atol=1e-12, err_msg=f"step {it + 1}")
            if p in opt.state:
                assert float(opt.state[p]["step"]) == st["t"]
                np.testing.assert_allclose(st["m"], opt.state[p]["exp_avg"].numpy(), rtol=1e-12, atol=1e-12)
                np.testing.assert_allclose(st["v"], opt.state[p]["exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-14)
        if it == LATE and not kw.get("weight_decay") and kw.get("eps", 1e-8) < 1e-6:
            # the counts are 4 and 1: the late parameter's first step has the bias corrections of step 1, so it moves by lr
            assert [st["t"] for st in mine] == [LATE + 1, 1]
            np.testing.assert_allclose((ps[1].detach() - before).abs().numpy(), kw["lr"], rtol=1e-6)


@pytest.mark.parametrize("momentum,dampening,nesterov", [(0.0, 0.0, False), (0.9, 0.0, False), (0.8, 0.1, False), (0.9, 0.0, True)])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_the_sgd_oracle_is_torch_sgd_in_fp64(momentum, dampening, nesterov, wd):
    ps, grads = _fp64_problem(4)
    opt = torch.optim.SGD(ps, lr=0.05, momentum=momentum, dampening=dampening, nesterov=nesterov, weight_decay=wd, foreach=False)
    mine = [dict(p=p.detach().numpy().copy(), b=None) for p in ps]
    gs = 1.0 / 3.0
    sc = optim_ref.sgd_scalars(0.05, wd, momentum, dampening, gs, rounded=False)
    for it in range(STEPS):
        for i, (p, st) in enumerate(zip(ps, mine)):
            if i == 1 and it < LATE:
                p.grad = None
                continue
            p.grad = grads[it][i] * gs
            first = st["b"] is None               # torch: the buffer of a parameter's first step is clone(grad), whenever that is
            st["p"], st["b"] = optim_ref.sgd_step(st["p"], grads[it][i].numpy(), st["b"], sc, nesterov, first)
        opt.step()
        for p, st in zip(ps, mine):
            np.testing.assert_allclose(st["p"], p.detach().numpy(), rtol=1e-12, atol=1e-12, err_msg=f"step {it + 1}")
            if momentum and opt.state[p].get("momentum_buffer") is not None:
                np.testing.assert_allclose(st["b"], opt.state[p]["momentum_buffer"].numpy(), rtol=1e-12, atol=1e-12)


# ---- the bound of tests/test_optim_steps_gpu.py on the reference alone ---------------------------------------------------------
SMALL_SIZES = (1, 3, 255, 256, 257, 1023)


def _ratio(got, want, bound):
    assert np.isfinite(got).all() and np.isfinite(want).all() and np.isfinite(bound).all()
    err = np.abs(np.asarray(got).astype(np.float64) - want)
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))))


@pytest.mark.parametrize("n", SMALL_SIZES)
def test_an_fp32_emulation_of_the_adam_kernel_stays_inside_the_bound(n):
    for hp in optim_ref.ADAM_SETS:
        p, g, m, v, _ = optim_ref.step_inputs(n, hp["grad_scale"])
        sc = optim_ref.adam_set_scalars(hp)
        with np.errstate(under="raise", over="raise"):        # the input ranges keep every fp32 intermediate normal
            got = optim_ref.adam_step_f32(p, g, m, v, sc)
        want, bound = optim_ref.adam_bounds(p, g, m, v, sc)
        for name, a, b, c in zip("pmv", got, want, bound):
            assert _ratio(a, b, c) <= 1.0, (hp["name"], name, _ratio(a, b, c))


@pytest.mark.parametrize("n", SMALL_SIZES)
def test_an_fp32_emulation_of_the_sgd_kernel_stays_inside_the_bound(n):
    for hp in optim_ref.SGD_SETS:
        p, g, _, _, buf = optim_ref.step_inputs(n, hp["grad_scale"])
        sc = optim_ref.sgd_set_scalars(hp)
        with np.errstate(under="raise", over="raise"):
            got = optim_ref.sgd_step_f32(p, g, buf, sc, hp["nesterov"], hp["first"])
        want, bound = optim_ref.sgd_bounds(p, g, buf, sc, hp["nesterov"], hp["first"])
        assert _ratio(got[0], want[0], bound[0]) <= 1.0, (hp["name"], "p")
        if hp["momentum"]:
            assert _ratio(got[1], want[1], bound[1]) <= 1.0, (hp["name"], "buf")


def test_the_emulation_stays_inside_the_bound_on_the_optimizer_tests_inputs():
    """The FusedAdam / FusedSGD tests of tests/test_optim_steps_gpu.py draw their start values (seeds 11-13, 21-22, 31) and their
    gradients (seeds 41-43 and 110-162) from the same generator, at these sizes."""
    adam = optim_ref.adam_scalars(1e-3, (0.9, 0.999), 1e-8, 1e-2, 3, 1.0 / 3.0)
    sgd = optim_ref.sgd_scalars(0.05, 1e-2, 0.9, 0.0, 1.0)
    for n in (35, 300, 24, 40, 54, 288):
        for sp in (11, 12, 13, 21, 22, 31):
            p, _, m, v, buf = optim_ref.step_inputs(n, seed=sp)
            for sg in list(range(41, 44)) + list(range(110, 163)):
                g = optim_ref.step_inputs(n, seed=sg)[1]
                with np.errstate(under="raise", over="raise"):
                    got, got_s = optim_ref.adam_step_f32(p, g, m, v, adam), optim_ref.sgd_step_f32(p, g, buf, sgd)
                want, bound = optim_ref.adam_bounds(p, g, m, v, adam)
                assert max(_ratio(a, b, c) for a, b, c in zip(got, want, bound)) <= 1.0, (n, sp, sg)
                want, bound = optim_ref.sgd_bounds(p, g, buf, sgd)
                assert max(_ratio(a, b, c) for a, b, c in zip(got_s, want, bound)) <= 1.0, (n, sp, sg)


def test_the_inputs_are_what_the_gpu_tests_say_they_are():
    for gs in (1.0, 1.0 / 3.0, 1.0 / 1024.0):
        p, g, m, v, buf = optim_ref.step_inputs(1023, gs)
        gg = np.abs(g.astype(np.float64) * float(np.float32(gs)))
        nz = gg[gg > 0]
        assert 0 < (gg == 0).sum() <= 0.03 * gg.size and nz.min() >= 0.99e-12 and nz.max() <= 1.01e6
        assert np.log10(nz.max() / nz.min()) > 15 and (g > 0).any() and (g < 0).any()
        assert (v == 0).any() and v.min() >= 0 and v[v > 0].min() >= 0.99e-24 and v.max() <= 1.01e12
        assert (np.abs(m.astype(np.float64)) <= 1.0001 * np.sqrt(v.astype(np.float64))).all()
        assert np.abs(p).max() <= 10 and (p == 0).any() and (buf == 0).any()


def test_the_bound_is_no_looser_than_the_bars_of_test_adam_known_answers():
    """p rtol 2e-6 (atol 1e-8), exp_avg rtol 1e-5 (atol 1e-8), exp_avg_sq rtol 2e-6 (atol 1e-12) on that test's own vectors.
    The bound is relative to the sum of the terms' magnitudes, those bars to the result: for p and exp_avg_sq the bound is the
    smaller one at every element.  For exp_avg it is 3 ulp = 3.6e-7 of |m| + (1-b1)|g| against 1e-5 of the result, 28 times
    smaller wherever the two terms do not cancel; twelve of the 257 golden elements cancel by more than that (the worst by 4000:
    m = -0.1434, g = 1.2908, result 3.5e-5), and at nine of them four roundings can exceed a bar relative to the result, so
    no bound that counts them can sit below it."""
    g4 = dict(np.load(os.path.join(ROOT, "tests", "golden", "g4_ops.npz"), allow_pickle=False))
    z = np.zeros(257, np.float32)
    kw = dict(lr=2e-4, betas=(0.9, 0.999), eps=1e-8, wd=1e-5)
    (p1, m1, v1), (bp, bm, bv) = optim_ref.adam_bounds(g4["adam/p0"], g4["adam/g"][0], z, z, optim_ref.adam_scalars(t=1, **kw))
    assert (bp <= 2e-6 * np.abs(p1) + 1e-8).all()
    (p2, m2, v2), (bp, bm, bv) = optim_ref.adam_bounds(p1.astype(np.float32), g4["adam/g"][1], m1.astype(np.float32),
                                                         v1.astype(np.float32), optim_ref.adam_scalars(t=1000, **kw))
    np.testing.assert_allclose(p2, g4["adam/p1000"], rtol=2e-6, atol=1e-8)        # the same step as the golden one
    assert (bp <= 2e-6 * np.abs(p2) + 1e-8).all() and (bv <= 2e-6 * np.abs(v2) + 1e-12).all()
    s_m = np.abs(m1) + 0.1 * np.abs(g4["adam/g"][1].astype(np.float64))
    assert (bm <= 3.6e-7 * 1.001 * (s_m + 1e-5 * 0.1 * np.abs(p1))).all()
    plain = np.abs(m2) >= s_m / 27.0
    assert plain.sum() == 257 - 12 and (bm[plain] <= 1e-5 * np.abs(m2[plain]) + 1e-8).all()
