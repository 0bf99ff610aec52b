"""Oracles of the optimizer launches, written from their definitions in fp64 numpy.

grad_stats           rd_grad_norm (include/resdepth_hip_optim.h)
adam_step, sgd_step  rd_adam_step / rd_adam_step_dev / rd_sgd_step: torch.optim.Adam and torch.optim.SGD on one tensor (coupled
                     weight decay, grad_scale applied to the raw gradient before the decay term), on the fp32 tensors and the fp32
                     scalars the kernel receives -- only the kernel's own arithmetic differs from them
adam_bounds, sgd_bounds, adam_step_f32, sgd_step_f32, step_inputs, ADAM_SETS, SGD_SETS
                     the error bound of tests/test_optim_steps_gpu.py (its docstring derives it), an fp32 emulation of the kernels in
                     their operation order (the bound is checked on the reference alone, tests/test_optim_cpu.py), and the inputs
                     and hyper-parameter sets both files share
"""
import functools
import math

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24            # half an ulp of fp32, relative: one correctly rounded operation
ULP = 2.0 ** -23          # one ulp of fp32, relative (an upper bound of ulp(x) / |x|)


def grad_stats(g):
    """(sum of squares of the finite elements in fp64, number of non-finite elements) of the RAW gradient"""
    g = np.asarray(g, np.float32)
    fin = np.isfinite(g)
    return float((g[fin].astype(np.float64) ** 2).sum()), float((~fin).sum())


# ---- the scalars as the launches receive them ------------------------------------------------------------------------------
def adam_scalars(lr, betas, eps, wd, t, grad_scale=1.0, rounded=True):
    """{1-b1, b2, 1-b2, eps, wd, lr/bc1, sqrt(bc2), grad_scale} as fp64; rounded: every value through fp32, as rd_adam_step's host
    code ((float)(1.0 - beta1), float arguments) and FusedAdam.advance() (a float64 array cast to float32) round them."""
    b1, b2 = betas
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    s = np.array([1.0 - b1, b2, 1.0 - b2, eps, wd, lr / bc1, math.sqrt(bc2), grad_scale], F64)
    return s.astype(F32).astype(F64) if rounded else s


def sgd_scalars(lr, wd, momentum, dampening, grad_scale=1.0, rounded=True):
    """{lr, wd, momentum, 1-dampening, grad_scale} as fp64; rounded: through fp32 as rd_sgd_step takes them, 1-dampening
    subtracted in fp32 (`1.f - dampening` of its host code)."""
    if not rounded:
        return np.array([lr, wd, momentum, 1.0 - dampening, grad_scale], F64)
    return np.array([F32(lr), F32(wd), F32(momentum), F32(1.0) - F32(dampening), F32(grad_scale)], F32).astype(F64)


# ---- the oracles ----------------------------------------------------------------------------------------------------------------
def adam_step(p, g, m, v, scalars):
    """torch.optim.Adam's update of one tensor -> (p, exp_avg, exp_avg_sq) in fp64."""
    p, g, m, v = (np.asarray(a).astype(F64) for a in (p, g, m, v))
    w1, b2, w2, eps, wd, step_size, bc2_sqrt, gs = (float(s) for s in scalars)
    ge = g * gs + wd * p
    m = (1.0 - w1) * m + w1 * ge
    v = b2 * v + w2 * ge * ge
    return p - step_size * m / (np.sqrt(v) / bc2_sqrt + eps), m, v


def sgd_step(p, g, buf, scalars, nesterov=False, first=False):
    """torch.optim.SGD's update of one tensor -> (p, momentum_buffer or None) in fp64.  first: the buffer starts as the
    gradient (torch's clone(grad))."""
    p, g = np.asarray(p).astype(F64), np.asarray(g).astype(F64)
    lr, wd, mom, damp1, gs = (float(s) for s in scalars)
    ge = g * gs + wd * p
    if mom == 0.0:
        return p - lr * ge, None
    b = ge if first else mom * np.asarray(buf).astype(F64) + damp1 * ge
    return p - lr * (ge + mom * b if nesterov else b), b


# ---- the bound (derivation: tests/test_optim_steps_gpu.py) --------------------------------------------------------------------
def adam_bounds(p, g, m, v, scalars):
    """-> (oracle (p, m, v), bounds (p, m, v)): the largest |kernel - oracle| the kernel's roundings can cause, plus one ulp."""
    p0, g0, m0, v0 = (np.asarray(a).astype(F64) for a in (p, g, m, v))
    w1, b2, w2, eps, wd, step_size, bc2_sqrt, gs = (float(s) for s in scalars)
    pn, mn, vn = adam_step(p0, g0, m0, v0, scalars)
    G = np.abs(g0 * gs) + np.abs(wd * p0)
    s_m = np.abs(m0) + w1 * G
    s_v = b2 * np.abs(v0) + w2 * G * G
    e_m, e_v = 4 * U * s_m, 6 * U * s_v                      # counted roundings, without the margin
    # the denominator between its extremes: sqrtf one ulp, the division and the addition half an ulp each
    d = np.sqrt(vn) / bc2_sqrt + eps
    d_lo = (np.sqrt(np.maximum(vn - e_v, 0.0)) / bc2_sqrt + eps) * (1 - 4 * U)
    d_hi = (np.sqrt(vn + e_v) / bc2_sqrt + eps) * (1 + 4 * U)
    with np.errstate(divide="ignore", invalid="ignore"):
        q_max = (np.abs(mn) + e_m) / d_lo
        e_q = e_m / d_lo + np.abs(mn) * np.maximum(1 / d_lo - 1 / d, 1 / d - 1 / d_hi) + U * q_max     # + the division m / denom
    e_upd = step_size * e_q
    b_p = e_upd + ULP * step_size * q_max + (U + ULP) * (np.abs(pn) + e_upd)
    return (pn, mn, vn), (b_p, e_m + ULP * s_m, e_v + ULP * s_v)


def sgd_bounds(p, g, buf, scalars, nesterov=False, first=False):
    """-> (oracle (p, buf), bounds (p, buf))"""
    p0, g0 = np.asarray(p).astype(F64), np.asarray(g).astype(F64)
    lr, wd, mom, damp1, gs = (float(s) for s in scalars)
    pn, bn = sgd_step(p0, g0, buf, scalars, nesterov, first)
    G = np.abs(g0 * gs) + np.abs(wd * p0)
    if mom == 0.0:
        e_d, s_d, b_b = 2 * U * G, G, None
    else:
        s_b = G if first else mom * np.abs(np.asarray(buf).astype(F64)) + damp1 * G
        e_b = 2 * U * G if first else 3 * U * s_b
        b_b = e_b + ULP * s_b
        if nesterov:
            e_d, s_d = mom * e_b + 2 * U * G + U * (mom * s_b + G), mom * s_b + G
        else:
            e_d, s_d = e_b, s_b
    e_upd = lr * e_d
    return (pn, bn), (e_upd + ULP * lr * s_d + (U + ULP) * (np.abs(pn) + e_upd), b_b)


# ---- fp32 emulation in the kernels' operation order (csrc/rd_elementwise.hip as built with -ffp-contract=on) ---------------------
def _fma(a, b, c):
    """fmaf: the product of two fp32 is exact in fp64; the sum is rounded to fp64 and then to fp32"""
    return (np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64) + np.asarray(c, F32).astype(F64)).astype(F32)


def adam_step_f32(p, g, m, v, scalars):
    p, g, m, v = (np.asarray(a, F32) for a in (p, g, m, v))
    w1, b2, w2, eps, wd, step_size, bc2_sqrt, gs = (F32(s) for s in scalars)
    ge = _fma(wd, p, g * gs)
    m = _fma(w1, ge - m, m)
    v = _fma(w2 * ge, ge, v * b2)
    denom = np.sqrt(v) / bc2_sqrt + eps
    return _fma(-step_size, m / denom, p), m, v


def sgd_step_f32(p, g, buf, scalars, nesterov=False, first=False):
    p, g = np.asarray(p, F32), np.asarray(g, F32)
    lr, wd, mom, damp1, gs = (F32(s) for s in scalars)
    ge = _fma(wd, p, g * gs)
    if mom == 0:
        return _fma(-lr, ge, p), None
    b = ge if first else _fma(damp1, ge, np.asarray(buf, F32) * mom)
    return _fma(-lr, _fma(mom, b, ge) if nesterov else b, p), b


# ---- inputs and hyper-parameter sets shared by the CPU and the GPU tests ------------------------------------------------------------
def _log_uniform(rng, n, lo, hi):
    return np.exp(rng.uniform(math.log(lo), math.log(hi), n))


@functools.lru_cache(maxsize=4)
def _raw_inputs(n, seed):
    rng = np.random.default_rng([seed, n])
    gg = _log_uniform(rng, n, 1e-12, 1e6) * rng.choice([-1.0, 1.0], n)              # g * grad_scale
    gg[rng.random(n) < 0.01] = 0.0
    v = np.where(rng.random(n) < 0.25, 0.0, _log_uniform(rng, n, 1e-24, 1e12))
    m = np.sqrt(v) * _log_uniform(rng, n, 1e-3, 1.0) * rng.choice([-1.0, 1.0], n)    # |m| <= sqrt(v): a mean against a mean square
    p = rng.uniform(-10.0, 10.0, n)
    p[rng.random(n) < 0.02] = 0.0
    buf = np.where(rng.random(n) < 0.05, 0.0, _log_uniform(rng, n, 1e-12, 1e6) * rng.choice([-1.0, 1.0], n))
    return tuple(a.astype(F32) for a in (p, gg, m, v, buf))


def step_inputs(n, grad_scale=1.0, seed=0):
    """fp32 (p, g, m, v, buf) of n elements, magnitudes over many binades: |g * grad_scale| log-uniform in [1e-12, 1e6] with both
    signs and about 1 % exact zeros; v zero (a quarter) or log-uniform in [1e-24, 1e12]; |m| in [1e-3, 1] * sqrt(v); p uniform in
    [-10, 10] with exact zeros; the SGD buffer like g.  No fp32 intermediate of either kernel underflows or overflows on them."""
    p, gg, m, v, buf = _raw_inputs(int(n), int(seed))
    g = (gg.astype(F64) / float(F32(grad_scale))).astype(F32)
    return p.copy(), g, m.copy(), v.copy(), buf.copy()


def _adam(name, t, gs=1.0, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=0.0):
    return dict(name=name, lr=lr, betas=betas, eps=eps, wd=wd, t=t, grad_scale=gs)


ADAM_SETS = [_adam("defaults-t1", 1), _adam("defaults-t1000", 1000), _adam("beta1-0-wd-gs.5", 7, 0.5, betas=(0.0, 0.999), wd=1e-2),
             _adam("eps1e-3-wd-gs1/3", 3, 1.0 / 3.0, eps=1e-3, wd=1e-2), _adam("t1000-gs1/1024", 1000, 1.0 / 1024.0),
             _adam("project-gs1/3", 2, 1.0 / 3.0, lr=2e-4, wd=1e-5)]
ADAM_SETS_LARGE = [ADAM_SETS[1], ADAM_SETS[2]]


def _sgd(momentum, dampening, nesterov, first, wd, gs, lr=0.05):
    return dict(name=f"mom{momentum}-damp{dampening}-nest{int(nesterov)}-first{int(first)}-wd{wd}-gs{gs:.3g}", lr=lr, wd=wd,
                momentum=momentum, dampening=dampening, nesterov=nesterov, first=first, grad_scale=gs)


SGD_SETS = [_sgd(0.0, 0.0, False, False, 0.0, 1.0), _sgd(0.0, 0.0, False, False, 1e-2, 1.0 / 3.0),
            _sgd(0.9, 0.0, False, True, 1e-2, 1.0), _sgd(0.9, 0.0, False, False, 0.0, 1.0 / 3.0),
            _sgd(0.9, 0.1, False, False, 1e-2, 1.0 / 3.0), _sgd(0.9, 0.1, False, True, 1e-2, 1.0),
            _sgd(0.9, 0.0, True, False, 1e-2, 1.0 / 3.0), _sgd(0.9, 0.0, True, True, 0.0, 1.0)]
SGD_SETS_LARGE = [SGD_SETS[4], SGD_SETS[6]]


def adam_set_scalars(hp, rounded=True):
    return adam_scalars(hp["lr"], hp["betas"], hp["eps"], hp["wd"], hp["t"], hp["grad_scale"], rounded)


def sgd_set_scalars(hp, rounded=True):
    return sgd_scalars(hp["lr"], hp["wd"], hp["momentum"], hp["dampening"], hp["grad_scale"], rounded)
