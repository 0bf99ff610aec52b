"""CPU checks of tests/level0_ref.py: every fp64 restatement against torch's own double-precision op (a different code path:
F.conv2d, F.conv_transpose2d, F.batch_norm, F.max_pool2d and autograd), and the premise of the exact-integer matrix of
test_level0_matrix_gpu.py -- the reference's largest magnitude sum stays below 2^23 for every case, so integer inputs make
every partial sum of any fp32 summation order exact."""
import pytest
import torch
import torch.nn.functional as F

import level0_ref as R

D = torch.float64


def _eq(a, b, tol=1e-12):
    scale = float(b.abs().max()) + 1e-300
    assert float((a - b).abs().max()) <= tol * scale


@pytest.mark.parametrize("n,h,w,cin,cout", [(2, 7, 9, 3, 8), (1, 2, 2, 1, 4), (3, 17, 33, 4, 12)])
def test_first_convolution_restatement(n, h, w, cin, cout):
    g = torch.Generator().manual_seed(h)
    x = torch.randn(n, cin, h, w, generator=g, dtype=D)
    wt = torch.randn(cout, cin, 3, 3, generator=g, dtype=D, requires_grad=True)
    dz = torch.randn(n, h, w, cout, generator=g, dtype=D)
    y = F.conv2d(x, wt, None, 1, 1)
    y.backward(dz.permute(0, 3, 1, 2))
    z, zmag = R.first_fwd(x, wt)
    _eq(z, y.detach().permute(0, 2, 3, 1))
    _eq(zmag, F.conv2d(x.abs(), wt.detach().abs(), None, 1, 1).permute(0, 2, 3, 1))
    dw, dwmag = R.first_wgrad(x, dz)
    _eq(dw, wt.grad)
    assert bool((dwmag >= dw.abs() - 1e-9).all())


@pytest.mark.parametrize("n,h,w,c,xc,bias", [(2, 7, 9, 8, 3, True), (1, 2, 2, 4, 1, False), (3, 17, 33, 20, 2, True)])
def test_last_convolution_restatement(n, h, w, c, xc, bias):
    g = torch.Generator().manual_seed(c)
    s = torch.randn(n, c, h, w, generator=g, dtype=D, requires_grad=True)
    wt = torch.randn(1, c, 3, 3, generator=g, dtype=D, requires_grad=True)
    b = torch.randn(1, generator=g, dtype=D, requires_grad=True) if bias else None
    x = torch.randn(n, xc, h, w, generator=g, dtype=D)
    dout = torch.randn(n, 1, h, w, generator=g, dtype=D)
    y = x[:, 0:1] + F.conv2d(s, wt, b, 1, 1)
    y.backward(dout)
    s_nhwc = s.detach().permute(0, 2, 3, 1)
    out, mag = R.last_fwd(s_nhwc, wt, b, x)
    _eq(out, y.detach())
    assert bool((mag >= out.abs() - 1e-9).all())
    _eq(R.last_dgrad(dout, wt)[0], s.grad.permute(0, 2, 3, 1))
    dw, db, _, dbmag = R.last_wgrad(s_nhwc, dout)
    _eq(dw, wt.grad)
    if bias:
        _eq(db, b.grad)
    _eq(dbmag, dout.abs().sum().reshape(1))


@pytest.mark.parametrize("slope,training,pool", [(0.0, True, True), (0.01, True, True), (0.25, False, True), (0.01, True, False)])
def test_bn_activation_pool_restatement(slope, training, pool):
    n, h, w, c = 3, 6, 10, 8
    g = torch.Generator().manual_seed(5)
    zt = (torch.randn(n, c, h, w, generator=g, dtype=D) * 1.7 + 0.6).requires_grad_(True)
    # ties: a quarter of the windows hold one repeated value
    with torch.no_grad():
        zt[:, :2] = torch.round(zt[:, :2])
    gam = (torch.rand(c, generator=g, dtype=D) + 0.5).requires_grad_(True)
    bet = (torch.randn(c, generator=g, dtype=D) * 0.3).requires_grad_(True)
    sl = torch.tensor([slope], dtype=D, requires_grad=True)
    rm, rv = torch.randn(c, generator=g, dtype=D), torch.rand(c, generator=g, dtype=D) + 0.5
    rm0, rv0 = rm.clone(), rv.clone()
    z = zt.detach().permute(0, 2, 3, 1).contiguous()
    mean, var, invstd = R.bn_stats(z)
    if training:
        y = F.batch_norm(zt, rm, rv, gam, bet, True, 0.1, 1e-5)
        nrm, nrv = R.bn_running_update(rm0, rv0, mean, var, n * h * w)
        _eq(nrm, rm)
        _eq(nrv, rv)
    else:
        mean, invstd = rm0, 1.0 / torch.sqrt(rv0 + 1e-5)
        y = F.batch_norm(zt, rm, rv, gam, bet, False, 0.1, 1e-5)
    a = F.prelu(y, sl)
    g_full = torch.randn(n, c, h, w, generator=g, dtype=D)
    obj = (a * g_full).sum()
    g_pool = idx = None
    ra, rp, ridx = R.bn_act_pool_fwd(z, mean, invstd, gam, bet, slope, pool)
    _eq(ra, a.detach().permute(0, 2, 3, 1))
    if pool:
        p, ti = F.max_pool2d(a, 2, 2, return_indices=True)
        g_pool = torch.randn(p.shape, generator=g, dtype=D)
        obj = obj + (p * g_pool).sum()
        _eq(rp, p.detach().permute(0, 2, 3, 1))
        pos = ((ti // w) % 2) * 2 + (ti % w) % 2
        assert torch.equal(ridx.long(), pos.permute(0, 2, 3, 1))
        g_pool, idx = g_pool.permute(0, 2, 3, 1).contiguous(), ridx
    obj.backward()
    b = R.bn_act_bwd(z, mean, invstd, gam, bet, slope, g_full.permute(0, 2, 3, 1), g_pool, idx, n * h * w, training)
    _eq(b["dz"], zt.grad.permute(0, 2, 3, 1), 1e-11)
    _eq(b["dgamma"], gam.grad, 1e-11)
    _eq(b["dbeta"], bet.grad, 1e-11)
    _eq(b["dslope"].sum().reshape(1), sl.grad, 1e-11)
    _eq(b["sum_g_full"], g_full.sum((0, 2, 3)), 1e-11)
    # the composite: first weight gradient of that dz, with the last convolution's data gradient as g_full
    x = torch.randn(n, 2, h, w, generator=g, dtype=D)
    wl = torch.randn(1, c, 3, 3, generator=g, dtype=D)
    dout = torch.randn(n, 1, h, w, generator=g, dtype=D)
    dw, bb = R.first_wgrad_of_block_backward(x, z, mean, invstd, gam, bet, slope, None, g_pool, idx, n * h * w, training, dout, wl)
    gl = F.conv_transpose2d(dout, wl, padding=1).permute(0, 2, 3, 1)
    b2 = R.bn_act_bwd(z, mean, invstd, gam, bet, slope, gl, g_pool, idx, n * h * w, training)
    _eq(bb["dz"], b2["dz"], 1e-11)
    w0 = torch.zeros(c, 2, 3, 3, dtype=D, requires_grad=True)
    (F.conv2d(x, w0, None, 1, 1) * b2["dz"].permute(0, 3, 1, 2)).sum().backward()
    _eq(dw, w0.grad, 1e-11)


def test_tail_restatement():
    n, hc, wc, cin, c0 = 2, 5, 3, 8, 4
    g = torch.Generator().manual_seed(9)
    xc = torch.randn(n, cin, hc, wc, generator=g, dtype=D, requires_grad=True)
    wt = torch.randn(cin, c0, 2, 2, generator=g, dtype=D, requires_grad=True)
    bt = torch.randn(c0, generator=g, dtype=D)
    a0 = torch.randn(n, c0, 2 * hc, 2 * wc, generator=g, dtype=D)
    wl = torch.randn(1, c0, 3, 3, generator=g, dtype=D, requires_grad=True)
    bl = torch.randn(1, generator=g, dtype=D, requires_grad=True)
    x = torch.randn(n, 3, 2 * hc, 2 * wc, generator=g, dtype=D)
    dout = torch.randn(n, 1, 2 * hc, 2 * wc, generator=g, dtype=D)
    s = F.conv_transpose2d(xc, wt, bt, stride=2) + a0
    out = x[:, 0:1] + F.conv2d(s, wl, bl, padding=1)
    out.backward(dout)
    xc_nhwc = xc.detach().permute(0, 2, 3, 1)
    rout, rs = R.tail_forward(xc_nhwc, wt, bt, a0.permute(0, 2, 3, 1), wl, bl, x)
    _eq(rout, out.detach())
    b = R.tail_backward(xc_nhwc, rs, wt, wl, dout)
    _eq(b["dxc"], xc.grad.permute(0, 2, 3, 1))
    _eq(b["dwt"], wt.grad)
    _eq(b["dw_last"], wl.grad)
    _eq(b["db_last"], bl.grad)


def _int_cases():
    first = [(n, h, w, cin, cout) for (cin, cout) in R.FIRST_PAIRS + R.GENERIC_FIRST_PAIRS for (n, h, w) in R.SPATIAL]
    first += [(n, h, w, 3, 32) for (n, h, w) in R.LOOP_SHAPES]
    last = [(n, h, w, c) for c in R.LAST_WIDTHS for (n, h, w) in R.SPATIAL] + [(n, h, w, 32) for (n, h, w) in R.LOOP_SHAPES]
    return first, last


def test_exact_integer_matrix_premise_holds_for_the_reference():
    """Non-vacuity of part A: the largest sum |a||b| of any output element of any case is below 2^23, so with integer inputs
    every product and partial sum is an integer that fp32 holds exactly, whatever the order."""
    first, last = _int_cases()
    worst = 0.0
    for n, h, w, cin, cout in first:
        worst = max(worst, R.int_first_case(n, h, w, cin, cout)["max_mag"])
    for n, h, w, c in last:
        worst = max(worst, R.int_last_case(n, h, w, c, 3, True)["max_mag"])
    assert 0 < worst < 2 ** 23, worst
    for n, h, w in R.LOOP_SHAPES:
        assert R.tiles(n, h, w) > R.MAX_BLOCKS and R.tiles(n, h, w) % R.MAX_BLOCKS != 0, (n, h, w)
