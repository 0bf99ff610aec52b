"""Level 0 (first convolution, last convolution, composed tail) pinned to fp64, instantiation by instantiation and element by
element (-m gpu).  References: tests/level0_ref.py (float64 restatements, checked on the CPU by test_level0_ref_cpu.py).

Three techniques:

A. exact-integer matrix -- inputs are integers in [-3, 3] stored as fp32, so every product and partial sum is an integer far
   below 2^24 and ANY summation order (vector ALU, DPP, exact-f32 MFMA, fp64 second stages) is exact: the bar is torch.equal
   with the fp64 reference.  One dropped, duplicated or misrouted term fails it.  Premise asserted per case (< 2^23).
B. element-wise bound on real data -- |got - ref64| <= (n + 2) 2^-24 sum|a||b| per element, n = number of terms: the standard
   bound of any fp32 summation order.  Weight-gradient shapes keep N H W <= 2048 so that one missing typical term exceeds it.
C. fused forms against the fp64 composite -- no closed bound exists, so the bar is measured on the inputs at hand, never
   from the code under test: the same composite runs in fp32 on the CPU, e32 = max over a channel's elements of
   |fp32 - fp64| / max|fp64| of that channel, and the kernel's error, normalised the same way, may be at most
   4 e32 + 2^-23 (4: another association order and fp32 per-tile partials where torch has one long or pairwise fp32 sum).
   "Channel" = the output-channel axis of the result (Cout of a weight gradient, C of an activation gradient, Cin of the
   up-convolution's gradients; a 1-channel result is one channel; for the four reduced BatchNorm sums each QUANTITY is a
   channel -- a per-channel sum has one element, and normalising a cancelling sum by itself bounds nothing in either
   arithmetic).  RD_LEVEL0_RATIOS=<file> makes the tests write the worst ratio per family there (profiles/level0_matrix.json).

Kernel templates and the rows that launch them (edge_conv knob in brackets; "A/B/C" = the parts above).  Every instantiation
reachable through the C ABI has a row.

rd_edge_conv.hip
  conv_first_fwd_seg_kernel<CIN 1-4, CQ 8/16/32>        A test_first_convolution_exact [default, vector]; B test_first_convolution_bound,
                                                         test_first_convolution_statistics_epilogues [default]
  conv_first_fwd_mfma_kernel<CIN 1-4, NB 1/2, MODE 0>   A/B the same tests [matrix = 127], Cout 32 / 64 (Cout 128 has no instantiation:
                                                         the knob leaves it on the segment kernel)
  conv_first_fwd_mfma_kernel<CIN 1-4, NB 1/2, MODE 1>   C test_first_convolution_with_activation_epilogue [matrix]
  conv_first_fwd_act_seg_kernel<CIN 1-4, CQ 8/16/32>    C test_first_convolution_with_activation_epilogue [default]
  conv_first_wgrad_seg_kernel<CIN 1-4, CQ, false>       A test_first_convolution_exact [default, vector], test_block_loops_exact;
                                                         B test_first_convolution_bound
  conv_first_wgrad_seg_kernel<CIN 1-3, CQ, true>        C test_fused_first_weight_gradient [vector = 63] (CIN 4 is refused by the C ABI)
  conv_first_wgrad_mfma_kernel<CIN 1-3, NB 1/2, GF t/f> C test_fused_first_weight_gradient [matrix = default]: g_full given (GF true),
                                                         g_full None and LastConvGrad (GF false); block loop in
                                                         test_fused_first_weight_gradient_block_loop_and_ties
  conv_last_fwd_dpp_kernel<LP 2/4/8>                    A test_last_convolution_exact; B test_last_convolution_bound (C 16 / 32 / 64)
  conv_last_dgrad_tile_kernel<false>                    A/B the same (runtime C)
  conv_last_dgrad_tile_kernel<true>                     C test_tail_against_the_uncomposed_layers (statistics hook; rows 0 = no epilogue
                                                         for that shape, the documented contract, on the 1100-image case)
  conv_last_wgrad_tile_kernel                           A test_last_convolution_exact, test_block_loops_exact; B test_last_convolution_bound
  tail_compose_kernel, convt_last_dgrad_kernel<false>,  C test_tail_against_the_uncomposed_layers (Cin 16 .. 256)
  tail_t16_kernel<CPL 4/8/16/32/64>, tail_corr_kernel,
  tail_wgrad_finish_kernel, conv_last_fwd_tail_kernel<LP 2/4/8>, tail_wl_finish_kernel
  conv_last_bwd_tail_fused_kernel                       C the same [head vector = 255]
  conv_last_bwd_tail_mfma_kernel<NB 1/2>                C the same [head matrix = 255 | 256], C0 32 / 64
  convt_last_dgrad_kernel<true>, conv_last_wgrad_tail_kernel, bn_act_pool_tailskip_kernel<LP 2/4/8>, conv_last_fwd_pre_kernel
                                                         C the same test (hook of the coarse block, rd_conv3x3_last_bwd_weight_tail,
                                                         rd_bn_act_pool_fwd_tailskip -> rd_conv3x3_last_fwd_tail_pre); the arg-max bytes
                                                         of the tailskip kernel stay with tests/test_tail_fold_gpu.py
rd_elementwise.hip (generic level-0 kernels)
  conv_first_kernel<CI 1-6, WGRAD false/true>           A test_first_convolution_exact [generic = 0] for CI 1-4, GENERIC_FIRST_PAIRS for
                                                         (5, 64), (3, 48), (6, 32); its 512-block loop in test_block_loops_exact [generic]
  conv_last_fwd_kernel, conv_last_dgrad_kernel,         A test_last_convolution_exact: C = 20 [default] and C 16 / 32 / 64 [generic = 0];
  conv_last_wgrad_kernel                                 B test_last_convolution_bound likewise
  bn_act_bwd_kernel<POOL, APPLY>                        C test_bn_backward_at_level0_widths (all four instantiations)
  bn_reduce_finalize*, partial_reduce_f32_kernel        B test_first_convolution_statistics_epilogues
None of these generic kernels goes through the split GEMM bodies (they are direct fp32 fmaf kernels), so no row runs under
mfma_f32 = 1 / mfma_products: those knobs do not change what is launched here.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import level0_ref as R
from test_ops_gpu import dev, nchw

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F32, F64 = torch.float32, torch.float64
EDGE = {"default": -1, "vector": 63, "matrix": 63 | 64, "generic": 0}
# kernel class each knob value selects for the first convolution (Cout in {32, 64, 128}, Cin <= 4):
#   default / vector: conv_first_fwd_seg + conv_first_wgrad_seg<.., false>;  matrix: conv_first_fwd_mfma (Cout <= 64) + the segment
#   weight gradient;  generic: conv_first_kernel<CI>.  Last convolution: default = tile kernels for C in {16, 32, 64}, generic for 20.


@pytest.fixture(params=list(EDGE))
def route(request):
    """knob edge_conv for the plain first / last convolution kernels, restored afterwards"""
    from resdepth_amd import _lib
    _lib.load()
    _lib.tune_set("edge_conv", EDGE[request.param])
    yield request.param
    _lib.tune_set("edge_conv", -1)


@pytest.fixture(params=["default", "generic"])
def last_route(request):
    from resdepth_amd import _lib
    _lib.load()
    _lib.tune_set("edge_conv", EDGE[request.param])
    yield request.param
    _lib.tune_set("edge_conv", -1)


@pytest.fixture(params=["default", "matrix"])
def act_route(request):
    from resdepth_amd import _lib
    _lib.load()
    _lib.tune_set("edge_conv", EDGE[request.param])
    yield request.param
    _lib.tune_set("edge_conv", -1)


@pytest.fixture(params=["vector", "matrix"])
def wgrad_pipe(request):
    """the fused first weight gradient on the vector ALU (edge_conv without bit 128) or on the exact-f32 matrix pipe (default)"""
    from resdepth_amd import _lib
    _lib.load()
    _lib.tune_set("edge_conv", -1 if request.param == "matrix" else 63)
    yield request.param
    _lib.tune_set("edge_conv", -1)


@pytest.fixture(params=["vector", "matrix"])
def head_pipe(request):
    """rd_conv3x3_last_bwd_tail_fused on the vector ALU or on the matrix pipe (opt-in bit 256)"""
    from resdepth_amd import _lib
    _lib.load()
    _lib.tune_set("edge_conv", 255 if request.param == "vector" else 255 | 256)
    yield request.param
    _lib.tune_set("edge_conv", -1)


def D(t):
    return None if t is None else t.to(dev())


def exact(got, ref64, name):
    want = ref64.to(F32)
    assert torch.equal(want.double(), ref64), name                      # the reference itself is an fp32 integer
    got = got.cpu()
    if not torch.equal(got, want):
        bad = (got != want)
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements differ, first at "
                             f"{tuple(int(i) for i in bad.nonzero()[0])}: {float(got[bad][0])} != {float(want[bad][0])}")


def within(got, ref64, bnd, name):
    err = (got.cpu().double() - ref64).abs()
    bad = err > bnd
    if bool(bad.any()):
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements beyond the bound; worst error / bound "
                             f"{float((err / (bnd + 1e-300))[bad].max()):.3g}")


def ulp32(t64):
    return torch.from_numpy(np.spacing(np.abs(t64.numpy()).astype(np.float32)).astype(np.float64))


# ---- part C: the fp32-relative bar -----------------------------------------------------------------------------------------------
_RATIOS = {}


def _chan_max(t, axis):
    t = t.movedim(axis, 0)
    return t.reshape(t.shape[0], -1).amax(1)


def rel_bar(family, got, ref64, ref32, axis, shape):
    """max over channels of (kernel error / max|ref|) / (4 e32 + 2^-23), asserted <= 1 and recorded per family"""
    ref64 = ref64.double()
    if ref64.dim() == 0 or axis is None:
        got, ref64, ref32, axis = got.reshape(1, -1), ref64.reshape(1, -1), ref32.reshape(1, -1), 0
    scale = _chan_max(ref64.abs(), axis) + 1e-300
    e32 = _chan_max((ref32.double() - ref64).abs(), axis) / scale
    ek = _chan_max((got.cpu().double() - ref64).abs(), axis) / scale
    ratio = float((ek / (4 * e32 + 2.0 ** -23)).max())
    worst = _RATIOS.get(family)
    if worst is None or ratio > worst["max_ratio"]:
        _RATIOS[family] = {"max_ratio": round(ratio, 4), "shape": list(shape)}
        path = os.environ.get("RD_LEVEL0_RATIOS")
        if path:
            with open(path, "w") as f:
                json.dump(_RATIOS, f, indent=1, sort_keys=True)
    print(f"{family} {tuple(shape)}: ratio {ratio:.4f} (kernel {float(ek.max()):.3e}, e32 {float(e32.max()):.3e})")
    assert ratio <= 1.0, f"{family} {tuple(shape)}: normalised error {float(ek.max()):.3e} > 4 x {float(e32.max()):.3e} + 2^-23 (ratio {ratio:.3f})"


# ---- part A ---------------------------------------------------------------------------------------------------------------------
int_first_case = functools.lru_cache(maxsize=None)(R.int_first_case)
int_last_case = functools.lru_cache(maxsize=None)(R.int_last_case)


def _run_first_exact(n, h, w, cin, cout, tag):
    from resdepth_amd import ops
    c = int_first_case(n, h, w, cin, cout)
    assert c["max_mag"] < 2 ** 23
    x = D(c["x"])
    exact(ops.conv3x3_first_fwd(x, D(c["w"])), c["z"], f"first fwd {tag} {(n, h, w, cin, cout)}")
    exact(ops.conv3x3_first_bwd_weight(x, D(c["dz"])), c["dw"], f"first wgrad {tag} {(n, h, w, cin, cout)}")


@pytest.mark.parametrize("cin,cout", R.FIRST_PAIRS)
def test_first_convolution_exact(cin, cout, route):
    """conv3x3_first_fwd / conv3x3_first_bwd_weight on every <CIN, COUT / 4> instantiation and every spatial class (one tile,
    ragged both ways, smaller than a tile, odd H and W -- x is NCHW, so odd W puts every second row at a 4-byte alignment --,
    N = 3), bit for bit against fp64."""
    for n, h, w in R.SPATIAL:
        _run_first_exact(n, h, w, cin, cout, route)


@pytest.mark.parametrize("cin,cout", R.GENERIC_FIRST_PAIRS)
def test_first_convolution_exact_on_the_generic_route(cin, cout):
    """channel pairs without a segment kernel: conv_first_kernel<CI> (5 and 6 input channels; 48 = 12 channel quads, 21 pixel
    slots and four idle threads per block)"""
    for n, h, w in R.SPATIAL:
        _run_first_exact(n, h, w, cin, cout, "generic pair")


def _run_last_exact(n, h, w, c, xc, bias, tag):
    from resdepth_amd import ops
    k = int_last_case(n, h, w, c, xc, bias)
    assert k["max_mag"] < 2 ** 23
    s, dout = D(k["s"]), D(k["dout"])
    tag = f"{tag} {(n, h, w, c, xc, bias)}"
    exact(ops.conv3x3_last_fwd(s, D(k["w"]), D(k["b"]), D(k["x"])), k["out"], "last fwd " + tag)
    exact(ops.conv3x3_last_bwd_data(dout, D(k["w"]), c), k["ds"], "last dgrad " + tag)
    dw, db = ops.conv3x3_last_bwd_weight(s, dout, want_bias=True)
    exact(dw, k["dw"], "last wgrad " + tag)
    exact(db, k["db"], "last dbias " + tag)


@pytest.mark.parametrize("c", R.LAST_WIDTHS)
def test_last_convolution_exact(c, last_route):
    """conv3x3_last_fwd (bias on / off, x_channels 1 and 3), conv3x3_last_bwd_data, conv3x3_last_bwd_weight + bias gradient:
    tile kernels for C in {16, 32, 64} (default), the generic kernels for C = 20 and for every width with the knob at 0."""
    for i, (n, h, w) in enumerate(R.SPATIAL):
        _run_last_exact(n, h, w, c, 3 if i % 2 else 1, i % 3 != 0, last_route)
    _run_last_exact(1, 18, 34, c, 3, False, last_route)
    _run_last_exact(1, 7, 9, c, 1, True, last_route)


def test_block_loops_exact(route):
    """More tiles than persistent blocks: the first weight gradient (1024 blocks; 512 on the generic route) and the last weight
    gradient (1024 blocks) walk several tiles per block, with a remainder (tiles % blocks != 0), on tiny images and on images of
    several ragged tiles."""
    from resdepth_amd import ops
    for n, h, w in R.LOOP_SHAPES:
        nt = R.tiles(n, h, w)
        assert nt > R.MAX_BLOCKS and nt % R.MAX_BLOCKS != 0, nt
        c = int_first_case(n, h, w, 3, 32)
        assert c["max_mag"] < 2 ** 23
        exact(ops.conv3x3_first_bwd_weight(D(c["x"]), D(c["dz"])), c["dw"], f"first wgrad block loop {route} {(n, h, w)}")
        if route in ("default", "generic"):
            k = int_last_case(n, h, w, 32, 3, True)
            assert k["max_mag"] < 2 ** 23
            dw, db = ops.conv3x3_last_bwd_weight(D(k["s"]), D(k["dout"]))
            exact(dw, k["dw"], f"last wgrad block loop {route} {(n, h, w)}")
            exact(db, k["db"], f"last dbias block loop {route} {(n, h, w)}")


# ---- part B ---------------------------------------------------------------------------------------------------------------------
def _flavour(t, flavour):
    return t if flavour == "randn" else t.abs() + 0.5


B_SHAPE = (2, 18, 34)           # ragged both ways, 1224 pixels <= 2048


@functools.lru_cache(maxsize=None)
def _first_real_case(cin, cout, flavour):
    n, h, w = B_SHAPE
    g = torch.Generator().manual_seed(31 * cin + cout + (1 if flavour == "randn" else 2))
    x = _flavour(torch.randn(n, cin, h, w, generator=g), flavour)
    wt = _flavour(torch.randn(cout, cin, 3, 3, generator=g), flavour) / 3
    dz = _flavour(torch.randn(n, h, w, cout, generator=g), flavour)
    z, zmag = R.first_fwd(x, wt)
    dw, dwmag = R.first_wgrad(x, dz)
    return dict(x=x, w=wt, dz=dz, z=z, zmag=zmag, dw=dw, dwmag=dwmag)


@pytest.mark.parametrize("flavour", ["randn", "positive"])
@pytest.mark.parametrize("cin,cout", R.FIRST_PAIRS)
def test_first_convolution_bound(cin, cout, flavour, route):
    from resdepth_amd import ops
    n, h, w = B_SHAPE
    c = _first_real_case(cin, cout, flavour)
    z = ops.conv3x3_first_fwd(D(c["x"]), D(c["w"]))
    within(z, c["z"], (9 * cin + 2) * U * c["zmag"], f"first fwd {route}")
    dw = ops.conv3x3_first_bwd_weight(D(c["x"]), D(c["dz"]))
    within(dw, c["dw"], (n * h * w + 2) * U * c["dwmag"], f"first wgrad {route}")


@pytest.mark.parametrize("flavour", ["randn", "positive"])
@pytest.mark.parametrize("c", R.LAST_WIDTHS)
def test_last_convolution_bound(c, flavour, last_route):
    from resdepth_amd import ops
    n, h, w = B_SHAPE
    g = torch.Generator().manual_seed(17 * c + (1 if flavour == "randn" else 2))
    s = _flavour(torch.randn(n, h, w, c, generator=g), flavour)
    wt = _flavour(torch.randn(1, c, 3, 3, generator=g), flavour) / (3 * c ** 0.5)
    b = _flavour(torch.randn(1, generator=g), flavour)
    x = _flavour(torch.randn(n, 2, h, w, generator=g), flavour)
    dout = _flavour(torch.randn(n, 1, h, w, generator=g), flavour)
    out, omag = R.last_fwd(s, wt, b, x)
    within(ops.conv3x3_last_fwd(D(s), D(wt), D(b), D(x)), out, (9 * c + 2 + 2) * U * omag, "last fwd")
    ds, dsmag = R.last_dgrad(dout, wt)
    within(ops.conv3x3_last_bwd_data(D(dout), D(wt), c), ds, (9 + 2) * U * dsmag, "last dgrad")
    dw, db, dwmag, dbmag = R.last_wgrad(s, dout)
    gdw, gdb = ops.conv3x3_last_bwd_weight(D(s), D(dout))
    within(gdw, dw, (n * h * w + 2) * U * dwmag, "last wgrad")
    within(gdb, db, (n * h * w + 2) * U * dbmag, "last dbias")


@pytest.mark.parametrize("cin,cout", R.FIRST_PAIRS)
def test_first_convolution_statistics_epilogues(cin, cout, act_route):
    """conv3x3_first_fwd_stats / conv3x3_first_fwd_bn: per-tile fp32 partials of 512 pixels (T), combined in fp64.  Channel mean
    within (T + 2) 2^-24 mean|z|; invstd and the running statistics at the same relative size times the conditioning factor
    (1 + mean^2 / var) of the sum-of-squares form (inputs keep |mean| / std <= 2, asserted)."""
    from resdepth_amd import ops
    n, h, w, T = 3, 40, 72, 512                     # 3 x 3 ragged tiles per image
    g = torch.Generator().manual_seed(5 * cin + cout)
    x = torch.randn(n, cin, h, w, generator=g) + 0.4
    wt = torch.randn(cout, cin, 3, 3, generator=g) / 3
    cnt = n * h * w
    z64, _ = R.first_fwd(x, wt)
    mean, var, invstd = R.bn_stats(z64)
    assert float((mean.abs() / var.sqrt()).max()) <= 2.0
    absmean = z64.abs().reshape(-1, cout).mean(0)
    cond = 1 + mean ** 2 / var
    z, sums = ops.conv3x3_first_fwd_stats(D(x), D(wt))
    within(sums[:cout] / cnt, mean, (T + 2) * U * absmean, "stats: mean")
    rm0, rv0 = torch.randn(cout, generator=g), torch.rand(cout, generator=g) + 0.5
    rm, rv, nbt = D(rm0.clone()), D(rv0.clone()), torch.zeros((), dtype=torch.long, device=dev())
    z2, gm, gi = ops.conv3x3_first_fwd_bn(D(x), D(wt), rm, rv, nbt)
    assert torch.equal(z2, z) and int(nbt) == 1
    within(gm, mean, (T + 2) * U * absmean + ulp32(mean), "bn: mean")
    rel = ((gi.cpu().double() - invstd).abs() / invstd) / ((T + 2) * U * cond + 2 * U)
    assert float(rel.max()) <= 1.0, f"bn: invstd beyond (T + 2) 2^-24 (1 + mean^2 / var) by {float(rel.max()):.3g}; factor up to {float(cond.max()):.2f}"
    nrm, nrv = R.bn_running_update(rm0, rv0, mean, var, cnt)
    within(rm, nrm, 0.1 * (T + 2) * U * absmean + 2 * ulp32(nrm), "bn: running mean")
    vb = 0.1 * var * cnt / (cnt - 1.0) * (T + 2) * U * cond + 2 * ulp32(nrv)
    err = (rv.cpu().double() - nrv).abs()
    assert bool((err <= vb).all()), f"bn: running var beyond (T + 2) 2^-24 (1 + mean^2 / var), worst {float((err / vb).max()):.3g}; factor up to {float(cond.max()):.2f}"


# ---- part C ---------------------------------------------------------------------------------------------------------------------
def _dyadic_bn(c, g):
    """BatchNorm parameters on small dyadic grids: invstd * gamma, mean * that and beta - that are exact in fp32, so the affine
    map of the kernel is ONE rounding (the fmaf) and the propagated bound below is rigorous"""
    mean = torch.randint(-4, 5, (c,), generator=g).float() / 8
    invstd = torch.randint(2, 7, (c,), generator=g).float() / 4
    gamma = torch.randint(1, 5, (c,), generator=g).float() / 2 * (torch.randint(0, 2, (c,), generator=g).float() * 2 - 1)
    beta = torch.randint(-4, 5, (c,), generator=g).float() / 4
    return mean, invstd, gamma, beta


@pytest.mark.parametrize("cin,cout", R.FIRST_PAIRS)
def test_first_convolution_with_activation_epilogue(cin, cout, act_route):
    """conv3x3_first_fwd_act: `a` within the part-B bound of z carried through the affine map (x |gamma invstd|, the activation is
    1-Lipschitz) + 2 ulp of the result; `pooled` == the 2 x 2 maximum of the kernel's own `a`, bit for bit."""
    from resdepth_amd import ops
    n, h, w = B_SHAPE
    c = _first_real_case(cin, cout, "randn")
    g = torch.Generator().manual_seed(cin + cout)
    mean, invstd, gamma, beta = _dyadic_bn(cout, g)
    x = D(c["x"])
    assert ops.conv3x3_first_fwd_act_available(x, cout)
    for pool, slope, sdev in ((True, 0.0, None), (False, 0.01, None), (True, 0.0, 0.25)):
        s_eff = float(np.float32(slope)) if sdev is None else sdev
        y = (c["z"] - mean.double()) * (invstd.double() * gamma.double()) + beta.double()
        a64 = torch.where(y > 0, y, y * s_eff)
        a, pooled = ops.conv3x3_first_fwd_act(x, D(c["w"]), D(mean), D(invstd), D(gamma), D(beta), slope,
                                              slope_dev=None if sdev is None else torch.full((1,), sdev, device=dev()), pool=pool)
        bnd = (9 * cin + 2) * U * c["zmag"] * (invstd * gamma).abs().double() + 2 * ulp32(a64)
        within(a, a64, bnd, f"fwd_act a {act_route} pool={pool} slope={s_eff}")
        if pool:
            assert torch.equal(nchw(pooled), F.max_pool2d(nchw(a), 2, 2)), f"fwd_act pooled {act_route}"
        else:
            assert pooled is None


def _block_case(n, h, w, cin, cout, seed, ties=False):
    """a first block as a forward would leave it: z, its batch statistics, idx from the forward's own max-pool"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, h, w, generator=g)
    z = torch.randn(n, h, w, cout, generator=g) * 1.3 + 0.2
    if ties:
        z = torch.round(z)                              # few distinct values: most windows hold their maximum more than once
    mean, var, invstd = R.bn_stats(z)
    mean, invstd = mean.float(), invstd.float()
    gamma, beta = torch.randn(cout, generator=g), torch.randn(cout, generator=g) * 0.3
    g_full = torch.randn(n, h, w, cout, generator=g)
    g_pool = torch.randn(n, h // 2, w // 2, cout, generator=g)
    dout = torch.randn(n, 1, h, w, generator=g)
    wl = torch.randn(1, cout, 3, 3, generator=g) / 3
    return dict(x=x, z=z, mean=mean, invstd=invstd, gamma=gamma, beta=beta, g_full=g_full, g_pool=g_pool, dout=dout, wl=wl)


def _idx(k, slope):
    return R.bn_act_pool_fwd(k["z"], k["mean"], k["invstd"], k["gamma"], k["beta"], slope, True)[2]


def _fused_wgrad(k, slope, sdev, training, mode, family, shape):
    """mode: 'full' (g_full + g_pool), 'pool' (g_pool only), 'skip' (g_full only), 'last' (LastConvGrad + g_pool)"""
    from resdepth_amd import ops
    s_eff = float(np.float32(slope)) if sdev is None else sdev
    idx = _idx(k, s_eff)
    gf = k["g_full"] if mode in ("full", "skip") else None
    gp = k["g_pool"] if mode != "skip" else None
    dout, wl = (k["dout"], k["wl"]) if mode == "last" else (None, None)
    cnt = k["z"].numel() // k["z"].shape[-1]
    args = (k["x"], k["z"], k["mean"], k["invstd"], k["gamma"], k["beta"], s_eff, gf, gp, idx if gp is not None else None, cnt, training)
    dw64, b64 = R.first_wgrad_of_block_backward(*args, dout=dout, w_last=wl)
    dw32, _ = R.first_wgrad_of_block_backward(*args, dout=dout, w_last=wl, dtype=F32)
    cout = k["z"].shape[-1]
    gfd = ops.LastConvGrad(D(dout), D(wl), cout) if mode == "last" else D(gf)
    got = ops.conv3x3_first_bwd_weight_bn(D(k["x"]), D(k["z"]), D(k["mean"]), D(k["invstd"]), D(k["gamma"]), D(k["beta"]), slope,
                                          gfd, D(gp), D(idx) if gp is not None else None, D(b64["sums"].reshape(-1).contiguous()),
                                          cnt, training, slope_dev=None if sdev is None else torch.full((1,), sdev, device=dev()))
    rel_bar(family, got, dw64, dw32, 0, shape + (mode, "train" if training else "eval"))


@pytest.mark.parametrize("cin,cout", [(cin, cout) for cin in (1, 2, 3) for cout in (32, 64, 128)])
def test_fused_first_weight_gradient(cin, cout, wgrad_pipe):
    """conv3x3_first_bwd_weight_bn against the fp64 composite (block backward, then the weight gradient), idx from a real
    forward: g_full given / absent / LastConvGrad, training and eval form, scalar and on-device slope.  Nine pairs on the
    segment kernel, six on the matrix kernel (Cout = 128 has none: the default knob leaves it on the segment kernel)."""
    n, h, w = B_SHAPE
    k = _block_case(n, h, w, cin, cout, 100 * cin + cout)
    fam = f"first_wgrad_bn_{'vector' if cout == 128 else wgrad_pipe}"
    _fused_wgrad(k, 0.01, None, True, "full", fam, (n, h, w, cin, cout))
    _fused_wgrad(k, 0.0, None, False, "pool", fam, (n, h, w, cin, cout))
    _fused_wgrad(k, 0.0, 0.25, True, "skip", fam, (n, h, w, cin, cout))
    if cout <= 64:
        _fused_wgrad(k, 0.0, 0.25, True, "last", fam, (n, h, w, cin, cout))
        _fused_wgrad(k, 0.01, None, False, "last", fam, (n, h, w, cin, cout))


def test_fused_first_weight_gradient_block_loop_and_ties(wgrad_pipe):
    """the same with more tiles than blocks (1100 images of 2 x 2: every block but 76 walks one tile, 76 walk two) and with a z of
    few distinct values, so that most pooling windows tie and the routed position is the FIRST maximum"""
    n, h, w = 1100, 2, 2
    assert R.tiles(n, h, w) > R.MAX_BLOCKS
    fam = f"first_wgrad_bn_{wgrad_pipe}"
    _fused_wgrad(_block_case(n, h, w, 3, 32, 7), 0.01, None, True, "full", fam, (n, h, w, 3, 32))
    _fused_wgrad(_block_case(n, h, w, 3, 64, 8), 0.0, None, True, "last", fam, (n, h, w, 3, 64))
    n, h, w = B_SHAPE
    kt = _block_case(n, h, w, 2, 64, 9, ties=True)
    win = R._windows(R.bn_act_pool_fwd(kt["z"], kt["mean"], kt["invstd"], kt["gamma"], kt["beta"], 0.0, True)[0])
    assert float(((win == win.amax(-1, keepdim=True)).sum(-1) > 1).double().mean()) > 0.3       # ties are common
    _fused_wgrad(kt, 0.0, None, True, "full", fam, (n, h, w, 2, 64, "ties"))


@pytest.mark.parametrize("pool", [True, False])
@pytest.mark.parametrize("c", [16, 32, 64, 128])
def test_bn_backward_at_level0_widths(c, pool):
    """bn_act_bwd_reduce / bn_act_bwd_apply against the fp64 backward: the outside anchor of the chain tests that compare
    fused kernels with these two"""
    from resdepth_amd import ops
    n, h, w = B_SHAPE
    k = _block_case(n, h, w, 1, c, 50 + c)
    cnt = n * h * w
    for slope, training in ((0.01, True), (0.0, False)):
        s_eff = float(np.float32(slope))
        idx = _idx(k, s_eff) if pool else None
        gp = k["g_pool"] if pool else None
        args = (k["z"], k["mean"], k["invstd"], k["gamma"], k["beta"], s_eff, k["g_full"], gp, idx, cnt, training)
        b64, b32 = R.bn_act_bwd(*args), R.bn_act_bwd(*args, dtype=F32)
        dargs = (D(k["z"]), D(k["mean"]), D(k["invstd"]), D(k["gamma"]), D(k["beta"]), slope, D(k["g_full"]), D(gp), D(idx))
        dgam, dbet = torch.empty(c, device=dev()), torch.empty(c, device=dev())
        sums = ops.bn_act_bwd_reduce(*dargs, dgamma=dgam, dbeta=dbet)
        rel_bar("bn_act_bwd_reduce", sums.view(4, c), b64["sums"], b32["sums"], 0, (n, h, w, c, pool))
        rel_bar("bn_act_bwd_reduce", torch.stack([dbet, dgam]), b64["sums"][:2], b32["sums"][:2], 0, (n, h, w, c, pool, "params"))
        dz = ops.bn_act_bwd_apply(*dargs, D(b64["sums"].reshape(-1).contiguous()), cnt, training)
        rel_bar("bn_act_bwd_apply", dz, b64["dz"], b32["dz"], 3, (n, h, w, c, pool, training))


TAIL_CASES = [(2, 9, 5, 16, 16), (2, 9, 5, 32, 32), (2, 9, 5, 64, 64), (2, 9, 5, 128, 32), (2, 9, 5, 256, 64),
              (1100, 1, 1, 16, 32)]      # coarse 9 x 5 -> 18 x 10, not multiples of the tile; 1100 tiles > 1024 blocks


@pytest.mark.parametrize("n,hc,wc,cin,c0", TAIL_CASES)
def test_tail_against_the_uncomposed_layers(n, hc, wc, cin, c0, head_pipe):
    """tail_compose + convt_last_bwd_data, convt_last_bwd_weight, conv3x3_last_fwd_tail, conv3x3_last_bwd_tail_fused (+
    tail_wl_finish) against fp64 of ConvTranspose2d 2 x 2 -> skip add -> 3 x 3 convolution to one channel, layer by layer."""
    from resdepth_amd import ops
    h, w = 2 * hc, 2 * wc
    if n > 1000:
        assert ops.load().rd_conv3x3_last_bwd_tail_blocks(n, h, w) < R.tiles(n, h, w)
    g = torch.Generator().manual_seed(cin + c0 + n)
    xc = torch.randn(n, hc, wc, cin, generator=g)
    wt = torch.randn(cin, c0, 2, 2, generator=g) / cin ** 0.5
    bt = torch.randn(c0, generator=g) * 0.2
    wl = torch.randn(1, c0, 3, 3, generator=g) / 3
    bl = torch.randn(1, generator=g)
    xin = torch.randn(n, 3, h, w, generator=g)
    dout = torch.randn(n, 1, h, w, generator=g)
    z = torch.randn(n, h, w, c0, generator=g)
    mean, invstd = torch.randn(c0, generator=g) * 0.2, torch.rand(c0, generator=g) + 0.5
    gamma, beta = torch.randn(c0, generator=g), torch.randn(c0, generator=g) * 0.3
    slope = float(np.float32(0.01))
    zc = torch.randn(n, hc, wc, cin, generator=g)                 # the block that feeds the up-convolution (statistics hook)
    mc, ic = torch.randn(cin, generator=g) * 0.2, torch.rand(cin, generator=g) + 0.5
    gc, bc = torch.randn(cin, generator=g), torch.randn(cin, generator=g) * 0.3
    ref = {}
    for dt in (F64, F32):
        a0 = R.bn_act_pool_fwd(z, mean, invstd, gamma, beta, slope, False, dtype=dt)[0]
        out, s = R.tail_forward(xc, wt, bt, a0, wl, bl, xin, dtype=dt)
        b = R.tail_backward(xc, s, wt, wl, dout, dtype=dt)
        b["out"] = out
        b["sums"] = R.bn_act_bwd(z, mean, invstd, gamma, beta, slope, b["g"], None, None, n * h * w, True, dtype=dt)["sums"]
        b["sums_c"] = R.bn_act_bwd(zc, mc, ic, gc, bc, slope, b["dxc"], None, None, n * hc * wc, True, dtype=dt)["sums"]
        b["pooled"] = R.bn_act_pool_fwd(z, mean, invstd, gamma, beta, slope, True, dtype=dt)[1]
        ref[dt] = b
    r64, r32 = ref[F64], ref[F32]
    shape = (n, hc, wc, cin, c0)
    skip = {"z": D(z), "mean": D(mean), "invstd": D(invstd), "gamma": D(gamma), "beta": D(beta), "slope": 0.01, "slope_dev": None}
    assert ops.tail_available(cin, c0)
    m, v, vt, b9 = ops.tail_compose(D(wt), D(wl), D(bt), forward=True)
    rel_bar("tail_convt_dgrad", ops.convt_last_bwd_data(D(dout), v), r64["dxc"], r32["dxc"], 3, shape)
    c16 = torch.empty(cin, 16, dtype=torch.float64, device=dev())
    rel_bar("tail_convt_wgrad", ops.convt_last_bwd_weight(D(xc), D(dout), D(wl), c16=c16), r64["dwt"], r32["dwt"], 0, shape)
    out = ops.conv3x3_last_fwd_tail(skip, ops.tail_t16(D(xc), v), b9, D(wl), D(bl), D(xin))
    rel_bar("tail_last_fwd", out, r64["out"], r32["out"], None, shape)
    fam = f"tail_head_{head_pipe}"
    wpart, stat = ops.conv3x3_last_bwd_tail_fused(skip, D(dout), D(wl))
    dw, db = ops.tail_wl_finish(wpart, c16, D(wt), D(bt))
    rel_bar(fam + "_dw", dw, r64["dw_last"], r32["dw_last"], 1, shape)
    rel_bar(fam + "_dbias", db, r64["db_last"], r32["db_last"], None, shape)
    sums = ops.bn_bwd_stats_finalize([stat], c0)
    rel_bar(fam + "_bn_sums", sums.view(4, c0), r64["sums"], r32["sums"], 0, shape)
    # the same quantities through the statistics hooks and the folded forms (rows 0: the shape has no statistics epilogue)
    hook = ops.BnHook(skip["z"], skip["mean"], skip["invstd"], skip["gamma"], skip["beta"], 0.01, None, 1)
    ds, part = ops.conv3x3_last_bwd_data(D(dout), D(wl), c0, bn=hook)
    rel_bar("last_dgrad_hook_ds", ds, r64["g"], r32["g"], 3, shape)
    if part[1]:
        rel_bar("last_dgrad_hook_bn_sums", ops.bn_bwd_stats_finalize([part], c0).view(4, c0), r64["sums"], r32["sums"], 0, shape)
    hookc = ops.BnHook(D(zc), D(mc), D(ic), D(gc), D(bc), 0.01, None, 1)
    dprev, partc = ops.convt_last_bwd_data(D(dout), v, bn=hookc)
    rel_bar("tail_convt_dgrad", dprev, r64["dxc"], r32["dxc"], 3, shape)
    if partc[1]:
        rel_bar("tail_convt_dgrad_hook_bn_sums", ops.bn_bwd_stats_finalize([partc], cin).view(4, cin), r64["sums_c"], r32["sums_c"],
                0, shape)
    dw2, db2 = ops.conv3x3_last_bwd_weight_tail(skip, D(dout), c16, D(wt), D(bt))
    rel_bar("tail_last_wgrad_dw", dw2, r64["dw_last"], r32["dw_last"], 1, shape)
    rel_bar("tail_last_wgrad_dbias", db2, r64["db_last"], r32["db_last"], None, shape)
    pooled, _, _, skip9 = ops.bn_act_pool_fwd_tailskip(skip["z"], skip["mean"], skip["invstd"], skip["gamma"], skip["beta"], 0.01, D(wl))
    rel_bar("tailskip_pooled", pooled, r64["pooled"], r32["pooled"], 3, shape)
    rel_bar("tail_last_fwd_pre", ops.conv3x3_last_fwd_tail_pre(skip9, ops.tail_t16(D(xc), v), b9, D(bl), D(xin)), r64["out"],
            r32["out"], None, shape)
