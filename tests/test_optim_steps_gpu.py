"""rd_adam_step, rd_adam_step_dev and rd_sgd_step element by element against the fp64 oracles of tests/optim_ref.py, and FusedAdam /
FusedSGD step by step through the same oracles.  No model, no convolution, no loss, no backward.

The bound
---------
Every fp32 operation of the kernels as built (csrc/rd_elementwise.hip with -ffp-contract=on: `a * b + c` inside one expression is one
fmaf) is correctly rounded: a relative error of at most u = 2^-24, half an ulp.  The oracle works on the same fp32 tensors and the
same fp32 scalars, so it differs from the kernel by those roundings alone.  Errors are carried as ABSOLUTE errors against the sum of
the magnitudes of the terms, never against the result, so a result that cancels needs no allowance.  G = |g*gs| + |wd*p|.

  ge = fmaf(wd, p, g * gs)            two roundings, each of at most u*G                                          |d ge| <= 2u G
  m' = fmaf(w1, ge - m, m)            ge - m: u(G + |m|); the fmaf: u(|m| + w1(G + |m|)); w1 <= 1
                                      |d m'| <= w1(3u G + u|m|) + u|m| + u w1(G + |m|) <= 4u S_m,  S_m = |m| + w1 G
  v' = fmaf(w2 * ge, ge, v * b2)      ge enters twice (|d ge^2| <= 4u G^2), w2 * ge, v * b2 and the fmaf one rounding each
                                      |d v'| <= 6u S_v,  S_v = b2 |v| + w2 G^2
  denom = sqrtf(v') / bc2_sqrt + eps  sqrtf: 1 ulp = 2u (HIP's table of single-precision math functions); the division: u (hipcc
                                      rounds fp32 division correctly unless told otherwise, and build.sh does not); the sum: u.
                                      All terms are positive, so denom lies between (sqrt(max(v' -+ 6u S_v, 0)) / bc2_sqrt + eps)
                                      (1 -+ 4u): an interval, not a first-order term, because v' itself may have cancelled
  q = m' / denom                      |d q| <= 4u S_m / denom_lo + |m'| max(1/denom_lo - 1/denom, 1/denom - 1/denom_hi) + u q_max
  p' = fmaf(-step_size, q, p)         |d p'| <= step_size |d q| + u |p'|

  SGD:  ge as above (2u G);  buf' = fmaf(1-damp, ge, buf * mom): |d buf'| <= 3u S_b, S_b = mom |buf| + (1-damp) G (first step:
  buf' = ge);  nesterov d = fmaf(mom, buf', ge): mom |d buf'| + 2u G + u(mom S_b + G);  p' = fmaf(-lr, d, p): lr |d d| + u |p'|.

Margin: one ulp (2u) of the same sums: 2u S_m, 2u S_v, 2u S_b, and for p one ulp of the update's magnitude sum plus one ulp of p'.
So m' is bounded by 3 ulp of S_m (3.6e-7), v' by 4 ulp of S_v (4.8e-7), the SGD buffer by 2.5 ulp of S_b, and p' by 1.5 ulp(p')
plus the update's error: below the bars of test_adam_known_answers (m 1e-5, v 2e-6, p 2e-6) wherever its operands do not cancel
(tests/test_optim_cpu.py checks that on that test's own vectors, and checks the bound itself on an fp32 emulation of the kernels).
optim_ref.adam_bounds / sgd_bounds are these formulas.  Every element of every tensor is compared; none is left out.

Inputs (optim_ref.step_inputs): a fixed seed, |g*gs| log-uniform over [1e-12, 1e6] with both signs and 1 % exact zeros, v zero or
log-uniform over [1e-24, 1e12], |m| <= sqrt(v), p in [-10, 10] with zeros: no fp32 intermediate underflows or overflows
(tests/test_optim_cpu.py runs the emulation with underflow and overflow trapped).
"""
import copy
import math

import numpy as np
import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu

# rd_adam_step, rd_adam_step_dev and rd_sgd_step (csrc/rd_elementwise.hip) launch `grid_cap((numel + 255) / 256, 8192)` blocks of
# `dim3(256)` threads: elements from WRAP on are served by a second (third, ...) trip of the kernels' grid-stride loops
WRAP = 8192 * 256
SMALL = (1, 3, 255, 256, 257, 1023)
LARGE = (WRAP + 1, 2 * WRAP + 3)
PAD = 4                   # floats in front of and behind every test tensor: 16 bytes, so shift 0 is 16-byte aligned and shift 1 is not
SENTINEL = -7.5

ADAM_CASES = [(n, None) for n in SMALL] + [(n, k) for n in LARGE for k in range(len(R.ADAM_SETS_LARGE))]
SGD_CASES = [(n, None) for n in SMALL] + [(n, k) for n in LARGE for k in range(len(R.SGD_SETS_LARGE))]


def _id(case):
    n, k = case
    return str(n) if k is None else f"{n}-set{k}"


def dev():
    return "cuda:0"


def _sets(case, small, large):
    return small if case[1] is None else [large[case[1]]]


def _put(a, shift):
    """a (fp32 numpy) in device memory `shift` floats past a 16-byte boundary, sentinels on both sides -> (buffer, view)"""
    n = a.size
    buf = torch.full((n + 2 * PAD + 1,), SENTINEL, device=dev(), dtype=torch.float32)
    view = buf[PAD + shift:PAD + shift + n]
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4 * shift
    return buf, view


def _get(pair, n, shift):
    """the tensor back on the host; nothing outside it was written"""
    buf = pair[0].cpu().numpy()
    assert (buf[:PAD + shift] == SENTINEL).all() and (buf[PAD + shift + n:] == SENTINEL).all(), "write outside the tensor"
    return buf[PAD + shift:PAD + shift + n]


def _ratio(got, want, bound, what):
    """max |got - want| / bound over EVERY element (0 where the two agree exactly)"""
    got = got.astype(np.float64)
    assert np.isfinite(got).all() and np.isfinite(want).all() and np.isfinite(bound).all(), what
    err = np.abs(got - want)
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))))


def run_adam(form, p, g, m, v, hp, shift=0):
    """one launch of rd_adam_step ("host") or rd_adam_step_dev ("dev") on copies of the fp32 arrays -> (p, m, v) fp32 numpy"""
    from resdepth_amd import ops
    n = p.size
    P, G, M, V = (_put(a, shift) for a in (p, g, m, v))
    b1, b2 = hp["betas"]
    if form == "host":          # the arguments FusedAdam._step_group passes
        ops.adam_step(P[1], G[1], M[1], V[1], b1, b2, hp["eps"], hp["wd"], hp["lr"] / (1.0 - b1 ** hp["t"]),
                      math.sqrt(1.0 - b2 ** hp["t"]), hp["grad_scale"])
    else:                       # the block FusedAdam.advance() writes
        block = torch.from_numpy(R.adam_set_scalars(hp).astype(np.float32)).to(dev())
        ops.adam_step_dev(P[1], G[1], M[1], V[1], block)
    torch.cuda.synchronize()
    assert np.array_equal(_get(G, n, shift).view(np.int32), g.view(np.int32)), "the gradient was written"
    return tuple(_get(x, n, shift) for x in (P, M, V))


def run_sgd(p, g, buf, hp, shift=0):
    from resdepth_amd import ops
    n = p.size
    P, G = _put(p, shift), _put(g, shift)
    B = _put(buf, shift) if hp["momentum"] else None
    ops.sgd_step(P[1], G[1], B[1] if B else None, hp["lr"], hp["wd"], hp["momentum"], hp["dampening"], hp["nesterov"], hp["first"],
                 hp["grad_scale"])
    torch.cuda.synchronize()
    assert np.array_equal(_get(G, n, shift).view(np.int32), g.view(np.int32)), "the gradient was written"
    return _get(P, n, shift), (_get(B, n, shift) if B else None)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


# ---- the three entry points against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ADAM_CASES, ids=_id)
def test_adam_entry_points_against_the_oracle(case):
    n = case[0]
    worst = {"host": 0.0, "dev": 0.0}
    for hp in _sets(case, R.ADAM_SETS, R.ADAM_SETS_LARGE):
        p, g, m, v, _ = R.step_inputs(n, hp["grad_scale"])
        want, bound = R.adam_bounds(p, g, m, v, R.adam_set_scalars(hp))
        for shift in (0, 1):
            for form in ("host", "dev"):
                got = run_adam(form, p, g, m, v, hp, shift)
                rs = [_ratio(a, b, c, (hp["name"], form, name)) for name, a, b, c in zip("pmv", got, want, bound)]
                worst[form] = max(worst[form], *rs)
                print(f"[ratio] adam_{form} n={n} shift={shift} {hp['name']}: p {rs[0]:.3f} m {rs[1]:.3f} v {rs[2]:.3f}")
                assert max(rs) <= 1.0, (hp["name"], form, shift, dict(zip("pmv", rs)))
    print(f"[worst] rd_adam_step n={n}: {worst['host']:.3f}   rd_adam_step_dev n={n}: {worst['dev']:.3f}")


@pytest.mark.parametrize("case", SGD_CASES, ids=_id)
def test_sgd_entry_point_against_the_oracle(case):
    n = case[0]
    worst = 0.0
    for hp in _sets(case, R.SGD_SETS, R.SGD_SETS_LARGE):
        p, g, _, _, buf = R.step_inputs(n, hp["grad_scale"])
        want, bound = R.sgd_bounds(p, g, buf, R.sgd_set_scalars(hp), hp["nesterov"], hp["first"])
        for shift in (0, 1):
            got = run_sgd(p, g, buf, hp, shift)
            rs = [_ratio(got[0], want[0], bound[0], (hp["name"], "p"))]
            if hp["momentum"]:
                rs.append(_ratio(got[1], want[1], bound[1], (hp["name"], "buf")))
            worst = max(worst, *rs)
            print(f"[ratio] sgd n={n} shift={shift} {hp['name']}: " + " ".join(f"{r:.3f}" for r in rs))
            assert max(rs) <= 1.0, (hp["name"], shift, rs)
    print(f"[worst] rd_sgd_step n={n}: {worst:.3f}")


@pytest.mark.parametrize("case", ADAM_CASES, ids=_id)
def test_the_two_adam_forms_are_bit_identical(case):
    """rd_adam_step_dev with the block FusedAdam.advance() builds == rd_adam_step with the arguments FusedAdam.step() passes"""
    n = case[0]
    for hp in _sets(case, R.ADAM_SETS, R.ADAM_SETS_LARGE):
        p, g, m, v, _ = R.step_inputs(n, hp["grad_scale"])
        for shift in (0, 1):
            host, device = run_adam("host", p, g, m, v, hp, shift), run_adam("dev", p, g, m, v, hp, shift)
            for name, a, b in zip("pmv", host, device):
                assert _same_bits(a, b), (hp["name"], shift, name, int((a.view(np.int32) != b.view(np.int32)).sum()))
            assert not _same_bits(host[0], p) or n < 4        # and the step did something


# ---- exact lanes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 1023])
def test_zero_gradient_and_zero_moments_leave_every_bit_alone(n):
    p = R.step_inputs(n)[0]
    p[0], p[-1] = -0.0, 0.0
    z = np.zeros(n, np.float32)
    for hp in R.ADAM_SETS:
        hp = dict(hp, wd=0.0)
        for form in ("host", "dev"):
            got = run_adam(form, p, z, z, z, hp, shift=n % 2)
            assert _same_bits(got[0], p) and _same_bits(got[1], z) and _same_bits(got[2], z), (hp["name"], form)
    for hp in R.SGD_SETS:
        hp = dict(hp, wd=0.0)
        got = run_sgd(p, z, z, hp, shift=n % 2)
        assert _same_bits(got[0], p) and (got[1] is None or _same_bits(got[1], z)), hp["name"]


def test_a_non_finite_gradient_element_stays_in_its_own_lane():
    n = 1023
    bad = {0: np.nan, 255: np.inf, 256: -np.inf, 700: np.nan, 1022: np.inf}
    idx = np.array(sorted(bad))
    others = np.setdiff1d(np.arange(n), idx)
    for hp in (R.ADAM_SETS[1], R.ADAM_SETS[3]):
        p, g, m, v, _ = R.step_inputs(n, hp["grad_scale"])
        gb = g.copy()
        for i, x in bad.items():
            gb[i] = x
        for form in ("host", "dev"):
            clean, dirty = run_adam(form, p, g, m, v, hp, 1), run_adam(form, p, gb, m, v, hp, 1)
            for name, a, b in zip("pmv", clean, dirty):
                assert np.isfinite(a).all() and _same_bits(a[others], b[others]), (hp["name"], form, name)
                assert not np.isfinite(b[idx]).any(), (hp["name"], form, name, b[idx])
    for hp in (R.SGD_SETS[1], R.SGD_SETS[4], R.SGD_SETS[6], R.SGD_SETS[5]):
        p, g, _, _, buf = R.step_inputs(n, hp["grad_scale"])
        gb = g.copy()
        for i, x in bad.items():
            gb[i] = x
        clean, dirty = run_sgd(p, g, buf, hp, 1), run_sgd(p, gb, buf, hp, 1)
        for a, b in zip(clean, dirty):
            if a is not None:
                assert np.isfinite(a).all() and _same_bits(a[others], b[others]), hp["name"]
                assert not np.isfinite(b[idx]).any(), (hp["name"], b[idx])


# ---- FusedAdam / FusedSGD step by step ---------------------------------------------------------------------------------------------------
SHAPES = [(7, 5), (300,), (3, 4, 2)]


def _numel(s):
    return int(np.prod(s))


def _np(t):
    """a device tensor's elements in logical order, on the host"""
    return t.detach().cpu().numpy().reshape(-1).copy()


def _tiled(shapes, order, values=None):
    """one flat device buffer tiled by tensors of `shapes`, laid out in `order` -> (buffer, views in the order of `shapes`)"""
    buf = torch.zeros(sum(_numel(s) for s in shapes), device=dev())
    views, off = [None] * len(shapes), 0
    for i in order:
        n = _numel(shapes[i])
        views[i] = buf[off:off + n].view(shapes[i])
        if values is not None:
            views[i].copy_(torch.from_numpy(values[i]).view(shapes[i]))
        off += n
    return buf, views


def _separate(shapes, values=None):
    return [torch.zeros(s, device=dev()) if values is None else torch.from_numpy(values[i]).view(s).to(dev()).clone()
            for i, s in enumerate(shapes)]


def _start_values(shapes, seed=11):
    return [R.step_inputs(_numel(s), seed=seed + i)[0] for i, s in enumerate(shapes)]


def _step_grads(shapes, it):
    return [R.step_inputs(_numel(s), seed=100 + 10 * it + i)[1] for i, s in enumerate(shapes)]


def _snapshot_adam(opt):
    snap = {}
    for group in opt.param_groups:
        for p in group["params"]:
            st, z = opt.state.get(p, {}), np.zeros(p.numel(), np.float32)
            snap[p] = dict(p=_np(p.data), m=_np(st["exp_avg"]) if "exp_avg" in st else z, v=_np(st["exp_avg_sq"]) if "exp_avg_sq" in st
                           else z, t=float(st["step"]) if "step" in st else 0.0)
    return snap


def _verify_adam(opt, snap, label):
    """every parameter with a gradient took the oracle's step with ITS OWN count; every other one kept its bits"""
    worst = 0.0
    for gi, group in enumerate(opt.param_groups):
        for pi, p in enumerate(group["params"]):
            s, st = snap[p], opt.state.get(p, {})
            what = (label, gi, pi)
            if p.grad is None:
                assert _same_bits(_np(p.data), s["p"]) and float(st.get("step", 0.0)) == s["t"], what
                continue
            sc = R.adam_scalars(group["lr"], group["betas"], group["eps"], group["weight_decay"], s["t"] + 1, opt.grad_scale)
            want, bound = R.adam_bounds(s["p"], _np(p.grad), s["m"], s["v"], sc)
            assert float(st["step"]) == s["t"] + 1, what
            for name, got, w, b in zip("pmv", (_np(p.data), _np(st["exp_avg"]), _np(st["exp_avg_sq"])), want, bound):
                r = _ratio(got, w, b, what + (name,))
                worst = max(worst, r)
                assert r <= 1.0, what + (name, r)
    return worst


def _make_adam(case):
    """-> (FusedAdam, its parameters, a torch.optim.Adam on CPU copies, its parameters, set_grads(list of fp32 numpy))"""
    from resdepth_amd import FusedAdam
    vals = _start_values(SHAPES)
    if case == "flat":                       # the buffer holds C, A, B; the optimizer sees A, B, C
        _, views = _tiled(SHAPES, (2, 0, 1), vals)
        _, gviews = _tiled(SHAPES, (2, 0, 1))
    elif case == "per_tensor":
        views, gviews = _separate(SHAPES, vals), _separate(SHAPES)
    else:                                    # two groups: A and B tile one buffer, C stands alone
        _, ab = _tiled(SHAPES[:2], (1, 0), vals[:2])
        _, gab = _tiled(SHAPES[:2], (1, 0))
        views, gviews = ab + _separate(SHAPES[2:], vals[2:]), gab + _separate(SHAPES[2:])
    ps = [torch.nn.Parameter(v) for v in views]
    cps = [torch.nn.Parameter(torch.from_numpy(v.copy()).view(s)) for v, s in zip(vals, SHAPES)]
    if case == "two_groups":
        def groups(q):
            return [dict(params=q[:2], lr=1e-3, weight_decay=0.0), dict(params=q[2:], lr=5e-3, weight_decay=1e-2)]
        opt, ref = FusedAdam(groups(ps)), torch.optim.Adam(groups(cps), foreach=False)
    else:
        opt, ref = FusedAdam(ps, lr=1e-3, weight_decay=1e-2), torch.optim.Adam(cps, lr=1e-3, weight_decay=1e-2, foreach=False)

    def set_grads(grads, gs):
        for p, gv, c, g, s in zip(ps, gviews, cps, grads, SHAPES):
            gv.copy_(torch.from_numpy(g).view(s))
            p.grad = gv
            c.grad = (torch.from_numpy(g) * float(np.float32(gs))).view(s)     # torch has no grad_scale: the kernel's first product
    return opt, ps, ref, cps, set_grads


@pytest.mark.parametrize("case", ["flat", "per_tensor", "two_groups"])
def test_fused_adam_six_steps_each_against_the_oracle(case):
    opt, ps, ref, cps, set_grads = _make_adam(case)
    worst = 0.0
    for it in range(1, 7):
        if it == 3:
            for o in (opt, ref):
                for k, group in enumerate(o.param_groups):
                    group["lr"] = (3e-4, 2e-3)[k]
        if it == 4:
            opt.grad_scale = 1.0 / 3.0
        if it == 5:             # the moments and counts of a torch.optim.Adam that ran the same steps on the CPU
            opt.load_state_dict(copy.deepcopy(ref.state_dict()))      # a copy: the CPU step counters would be shared
            assert not opt._flat_state
            for p, c in zip(ps, cps):
                assert opt.state[p]["exp_avg"].is_cuda and torch.equal(opt.state[p]["exp_avg"].cpu(), ref.state[c]["exp_avg"])
                assert float(opt.state[p]["step"]) == 4.0
        set_grads(_step_grads(SHAPES, it), opt.grad_scale)
        snap = _snapshot_adam(opt)
        opt.step()
        ref.step()
        torch.cuda.synchronize()
        worst = max(worst, _verify_adam(opt, snap, f"{case} step {it}"))
        # which path ran: the flat one keeps its moments in _flat_state, one entry per group
        assert sorted(opt._flat_state) == {"flat": [0], "per_tensor": [], "two_groups": [0, 1]}[case], (case, it)
    print(f"[worst] FusedAdam {case}: {worst:.3f}")


def test_captured_step_plumbing_called_eagerly_matches_step():
    """capture_prepare / advance / capture_step without a graph, beside a twin that calls step(): the same bits after every step"""
    from resdepth_amd import FusedAdam
    vals = _start_values(SHAPES)
    twins = []
    for _ in range(2):
        buf, views = _tiled(SHAPES, (2, 0, 1), vals)
        gbuf, gviews = _tiled(SHAPES, (2, 0, 1))
        ps = [torch.nn.Parameter(v) for v in views]
        twins.append(dict(buf=buf, gviews=gviews, ps=ps, opt=FusedAdam(ps, lr=1e-3, weight_decay=1e-2)))
    a, b = twins

    def set_grads(it):
        for t in twins:
            for p, gv, g, s in zip(t["ps"], t["gviews"], _step_grads(SHAPES, it), SHAPES):
                gv.copy_(torch.from_numpy(g).view(s))
                p.grad = gv

    set_grads(1)
    assert a["opt"].capture_prepare() is False            # no moments yet
    a["opt"].step()
    b["opt"].step()
    assert a["opt"].capture_prepare() is True
    for it in range(2, 6):
        if it == 3:
            a["opt"].param_groups[0]["lr"] = b["opt"].param_groups[0]["lr"] = 3e-4
        if it == 4:
            a["opt"].grad_scale = b["opt"].grad_scale = 1.0 / 3.0
        set_grads(it)
        before = a["buf"].clone()
        a["opt"].advance()
        a["opt"].capture_step()
        b["opt"].step()
        torch.cuda.synchronize()
        assert not torch.equal(a["buf"], before)
        assert torch.equal(a["buf"].view(torch.int32), b["buf"].view(torch.int32)), it
        for k in (1, 2):
            assert torch.equal(a["opt"]._flat_state[0][k].view(torch.int32), b["opt"]._flat_state[0][k].view(torch.int32)), (it, k)
        sa, sb = a["opt"].state_dict()["state"], b["opt"].state_dict()["state"]
        assert [float(sa[i]["step"]) for i in range(3)] == [float(sb[i]["step"]) for i in range(3)] == [float(it)] * 3


@pytest.mark.parametrize("layout", ["flat", "separate"])
def test_a_parameter_without_gradient_keeps_its_own_step_count(layout):
    """torch.optim.Adam counts steps per parameter: the second parameter has no gradient for three steps, so its first step is
    bias-corrected as step 1 while the first parameter is at step 4."""
    from resdepth_amd import FusedAdam
    shapes = [(8, 5), (24,)]
    vals = _start_values(shapes, seed=21)
    if layout == "flat":
        _, views = _tiled(shapes, (1, 0), vals)
        _, gviews = _tiled(shapes, (1, 0))
    else:
        views, gviews = _separate(shapes, vals), _separate(shapes)
    ps = [torch.nn.Parameter(v) for v in views]
    opt = FusedAdam(ps, lr=1e-3)
    for it in range(1, 6):
        for i, (p, gv, g) in enumerate(zip(ps, gviews, _step_grads(shapes, it))):
            gv.copy_(torch.from_numpy(g).view(shapes[i]))
            p.grad = None if i == 1 and it <= 3 else gv
        snap = _snapshot_adam(opt)
        opt.step()
        torch.cuda.synchronize()
        _verify_adam(opt, snap, f"{layout} step {it}")
        counts = [float(opt.state[p]["step"]) if p in opt.state and "step" in opt.state[p] else 0.0 for p in ps]
        assert counts == [float(it), float(max(it - 3, 0))]
        if it >= 4:
            assert opt.capture_prepare() is False, "one scalar block cannot serve two step counts"
            assert bool(opt._flat_state) == (layout == "flat")       # the moments are flat; the launches were per tensor


def _permuted(kind, values=None):
    """a dense, non-contiguous device tensor: a transposed 2-D view or a channels_last 4-D weight"""
    shape = (9, 6) if kind == "transposed" else (8, 4, 3, 3)
    t = torch.zeros(shape) if values is None else torch.from_numpy(values).view(shape)
    t = t.to(dev())
    t = t.t().contiguous().t() if kind == "transposed" else t.contiguous(memory_format=torch.channels_last)
    assert not t.is_contiguous() and t.shape == shape
    return t


@pytest.mark.parametrize("grad_layout", ["contiguous", "same_strides"])
@pytest.mark.parametrize("kind", ["transposed", "channels_last"])
def test_fused_adam_on_a_permuted_parameter(kind, grad_layout):
    from resdepth_amd import FusedAdam
    n = 54 if kind == "transposed" else 288
    p = torch.nn.Parameter(_permuted(kind, R.step_inputs(n, seed=31)[0]))
    assert not p.data.is_contiguous()
    opt = FusedAdam([p], lr=1e-3, weight_decay=1e-2)
    for it in range(1, 4):
        g = R.step_inputs(n, seed=40 + it)[1]
        p.grad = _permuted(kind, g) if grad_layout == "same_strides" else torch.from_numpy(g).view(p.shape).to(dev())
        snap = _snapshot_adam(opt)
        opt.step()
        torch.cuda.synchronize()
        _verify_adam(opt, snap, f"{kind} {grad_layout} step {it}")
        assert not p.data.is_contiguous() and not opt._flat_state


@pytest.mark.parametrize("grad_layout", ["contiguous", "same_strides"])
@pytest.mark.parametrize("kind", ["transposed", "channels_last"])
def test_fused_sgd_on_a_permuted_parameter(kind, grad_layout):
    from resdepth_amd import FusedSGD
    n = 54 if kind == "transposed" else 288
    p = torch.nn.Parameter(_permuted(kind, R.step_inputs(n, seed=31)[0]))
    kw = dict(lr=0.05, momentum=0.9, weight_decay=1e-2)
    opt = FusedSGD([p], **kw)
    sc = R.sgd_scalars(kw["lr"], kw["weight_decay"], kw["momentum"], 0.0, 1.0)
    for it in range(1, 4):
        g = R.step_inputs(n, seed=40 + it)[1]
        p.grad = _permuted(kind, g) if grad_layout == "same_strides" else torch.from_numpy(g).view(p.shape).to(dev())
        p0 = _np(p.data)
        b0 = _np(opt.state[p]["momentum_buffer"]) if it > 1 else None
        opt.step()
        torch.cuda.synchronize()
        want, bound = R.sgd_bounds(p0, g, b0, sc, False, first=it == 1)
        what = (kind, grad_layout, it)
        assert _ratio(_np(p.data), want[0], bound[0], what) <= 1.0, what + ("p",)
        assert _ratio(_np(opt.state[p]["momentum_buffer"]), want[1], bound[1], what) <= 1.0, what + ("buf",)
        assert not p.data.is_contiguous()
