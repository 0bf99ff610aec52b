"""split2h -- two fp16 terms / three products per multiply, chosen per launch inside libresdepth_hip.so (-m gpu).
csrc/rd_mfma_dev.h, include/resdepth_hip.h (rd_quant_next), DESIGN.md 3.1h.

What the mode promises, and what this file pins:
  * per op (conv3x3 / convT2x2 x forward, data gradient, weight gradient): |out - ref64| <= 3 * 2^-22 * sum_k |a_k| |b_k| from the
    split (12 u, u = 2^-24) plus the accumulation's own fp32 roundings -- measured rms BELOW the exact-f32 MFMA chain on every
    operand flavour (hi / lo accumulators), the 1e-30 .. 1e30 `range` operands and 1e-36 operands included;
  * the magnitude slots: every producer's epilogue leaves exactly max |x| of the tensor it wrote (bit pattern), so the scale a
    consumer derives is a pure function of the tensor -- run-to-run identical results;
  * fallback: an operand without a slot, or with an infinite element, runs the six-product body -- BIT-identical to split3 mode,
    fp32's non-finite pattern included; a NaN element needs no fallback (it stays NaN in both terms);
  * the three-product bodies really run (a slot given -> results differ in the last bits from split3, never by more than the bound);
  * the whole net: every test of tests/test_unet_gpu.py runs in this mode when it is the process default (it is: GPUTEST runs
    them all), and a selection re-runs under RD_MFMA=split3 in a child process so the six-product arithmetic stays a tested
    configuration."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
U = 2.0 ** -24


@pytest.fixture()
def lib():
    from resdepth_amd import _lib
    _lib.load()
    before = _lib.tune_get("mfma_products")
    _lib.tune_set("mfma_products", 3)
    yield _lib
    _lib.tune_set("mfma_products", before)
    _lib.tune_set("mfma_f32", 0)
    _lib.tune_set("nt_tile", -1)


def _slot_max(t):
    """largest of the sixteen words of a tensor's magnitude slot, as a float"""
    s = t._rd_amax.view(16, 32)[:, 0].max().item()
    return torch.tensor([s], dtype=torch.int32).view(torch.float32).item()


@pytest.mark.parametrize("family,tile", [("conv", -1), ("conv", 0), ("conv", 1), ("conv", 2), ("convt", -1)])
# mates20 / mates30 / half30 (split_numerics.wide): outputs computed only from operands 2^-20 .. 2^-30 below a large element
# elsewhere in the same tensor -- on one scale per tensor they would be 2^-9-class (hundreds of u); the slot guard
# (rd_mfma_dev.h: quant_select) must send them to the six-product body
@pytest.mark.parametrize("flavour", ["randn", "pos", "range", "int24", "tiny", "mates20", "mates30", "half30"])
def test_per_op_error_bound_and_below_the_exact_f32_chain(lib, family, tile, flavour):
    import split_numerics as SN
    g = torch.Generator().manual_seed(7)
    ref, den, run = (SN.conv_cases if family == "conv" else SN.convt_cases)(flavour, g)
    lib.tune_set("nt_tile", tile)
    out = run()
    lib.tune_set("mfma_f32", 1)
    exact = run()
    lib.tune_set("mfma_f32", 0)
    for k in ref:
        if tile != -1 and k == "wgrad":
            continue
        s_max, s_rms = SN.nerr(out[k], ref[k], den[k])
        f_max, f_rms = SN.nerr(exact[k], ref[k], den[k])
        assert torch.isfinite(out[k]).all()
        # analytic: 12 u from the split + what the fp32 accumulation of this K does anyway (the exact kernel's own error)
        assert s_max <= 12.0 + 2.5 * f_max + 4.0, (family, tile, flavour, k, s_max, f_max)
        # measured (r06): 0.17 .. 0.23 u rms on randn (exact-f32: 0.34 .. 0.47), 1.8 .. 5.9 on pos (2.8 .. 16.5), 1.2 .. 1.8 on range
        assert s_rms <= 1.5 * f_rms + 0.5, (family, tile, flavour, k, s_rms, f_rms)


@pytest.mark.parametrize("family,tile", [("conv", -1), ("conv", 0), ("conv", 1), ("conv", 2), ("convt", -1)])
def test_channelwise_small_operands_keep_the_absolute_contract(lib, family, tile):
    """chan24: a few input channels of x and of the weight x 2^-24 -- inside every producer block, so the guard does not fire and
    the three-product body runs.  No relative bar: the documented bound for an arbitrary tensor, per output,
    |out - ref64| <= 12 u sum|a||b| + 2^-39 (amax(a) sum|b| + amax(b) sum|a|) + (the exact-f32 chain's own error).  It fails if the
    fp16 terms stop keeping subnormals or the scale is derived wrongly."""
    import split_numerics as SN
    g = torch.Generator().manual_seed(7)
    ref, den, run, floor = (SN.conv_cases if family == "conv" else SN.convt_cases)("chan24", g, floor=True)
    lib.tune_set("nt_tile", tile)
    out = run()
    lib.tune_set("mfma_f32", 1)
    exact = run()
    lib.tune_set("mfma_f32", 0)
    lib.tune_set("mfma_products", 6)
    six = run()
    lib.tune_set("mfma_products", 3)
    for k in ref:
        if tile != -1 and k == "wgrad":
            continue
        assert torch.isfinite(out[k]).all()
        err = (out[k].double() - ref[k]).abs()
        bound = 16 * U * den[k] + floor[k] + 2.5 * (exact[k].double() - ref[k]).abs()
        assert bool((err <= bound).all()), (family, tile, k, float((err / bound).max()))
        assert not torch.equal(out[k], six[k]), (family, tile, k, "the three-product body did not run")


@pytest.mark.parametrize("flavour", ["mates30", "half30"])
def test_conv1x1_wide_range_operands(lib, flavour):
    """rd_conv1x1_* take slots as well (operands tagged by rd_amax): the same wide-range construction and bar"""
    from resdepth_amd import ops
    g = torch.Generator().manual_seed(13)
    n, h, w, cin, cout = 2, 16, 16, 512, 128
    x = torch.randn(n, h, w, cin, generator=g)
    wt = torch.randn(cout, cin, generator=g) * 0.05
    gy = torch.randn(n, h, w, cout, generator=g)
    gyw = gy.clone()
    if flavour == "mates30":
        x[1] *= 2.0 ** -30
        gy[1] *= 2.0 ** -30
        gyw[0] = 0.0
    else:
        x[:, h // 2:] *= 2.0 ** -30
        gy[:, h // 2:] *= 2.0 ** -30
        gyw[:, :h // 2] = 0.0
    xd, wd, gd, gwd = x.double(), wt.double(), gy.double(), gyw.double()
    ref = {"fwd": xd @ wd.t(), "dgrad": gd @ wd, "wgrad": gwd.reshape(-1, cout).t() @ xd.reshape(-1, cin)}
    den = {"fwd": xd.abs() @ wd.abs().t(), "dgrad": gd.abs() @ wd.abs(), "wgrad": gwd.abs().reshape(-1, cout).t() @ xd.abs().reshape(-1, cin)}

    def run():
        tg = lambda t: ops.amax_of(t.to(DEV))
        wf, wtd = ops.pack_conv1x1_weight(wt.view(cout, cin, 1, 1).to(DEV))      # packed operands (both split forms)
        return {"fwd": ops.conv1x1_fwd(tg(x), wf).cpu(), "dgrad": ops.conv1x1_bwd_data(tg(gy), wtd).cpu(),
                "wgrad": ops.conv1x1_bwd_weight(tg(x), tg(gyw)).reshape(cout, cin).cpu()}
    out = run()
    lib.tune_set("mfma_f32", 1)
    exact = run()
    lib.tune_set("mfma_f32", 0)
    import split_numerics as SN
    for k in ref:
        s_max, _ = SN.nerr(out[k], ref[k], den[k])
        f_max, _ = SN.nerr(exact[k], ref[k], den[k])
        assert s_max <= 12.0 + 2.5 * f_max + 4.0, (flavour, k, s_max, f_max)


def test_three_product_body_runs_when_slots_are_given_and_six_product_body_when_not(lib):
    from resdepth_amd import ops
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 16, 16, 256, generator=g).to(DEV)
    w = (torch.randn(128, 256, 3, 3, generator=g) * 0.05).to(DEV)
    wf, _ = ops.pack_conv3x3_weight(w)
    assert getattr(wf, "_rd_amax", None) is not None and abs(_slot_max(wf) - float(w.abs().max())) == 0.0
    z6 = ops.conv3x3_fwd(x, wf)                           # x carries no slot: six products
    lib.tune_set("mfma_products", 6)
    wf6, _ = ops.pack_conv3x3_weight(w)
    z6_ref = ops.conv3x3_fwd(x, wf6)
    lib.tune_set("mfma_products", 3)
    assert torch.equal(z6, z6_ref), "an operand without a slot must run the six-product body, bit for bit"
    xt = ops.amax_of(x.clone())
    assert abs(_slot_max(xt) - float(x.abs().max())) == 0.0
    z3 = ops.conv3x3_fwd(xt, wf)
    assert not torch.equal(z3, z6), "with both slots the three-product body must run"
    ref = F.conv2d(x.permute(0, 3, 1, 2).double().cpu(), w.double().cpu(), None, 1, 1).permute(0, 2, 3, 1)
    den = F.conv2d(x.permute(0, 3, 1, 2).double().cpu().abs(), w.double().cpu().abs(), None, 1, 1).permute(0, 2, 3, 1)
    for z in (z3, z6):
        assert float(((z.double().cpu() - ref).abs() / den).max()) <= 16 * U
    assert torch.equal(ops.conv3x3_fwd(xt, wf), z3)      # same slots, same bits


@pytest.mark.parametrize("what", ["x=+inf", "x=-inf", "x=nan", "w=+inf", "x=+inf,w=0", "x=nan,x2=+inf"])
def test_nonfinite_operands_fall_back_to_six_products_and_match_fp32(lib, what):
    from resdepth_amd import ops
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 64, 16, 16, generator=g)
    wt = torch.randn(128, 64, 3, 3, generator=g) * 0.05
    val = {"+inf": float("inf"), "-inf": float("-inf"), "nan": float("nan"), "0": 0.0}
    for item in what.split(","):
        name, v = item.split("=")
        if name == "x":
            x[0, 5, 7, 9] = val[v]
        elif name == "x2":
            x[1, 9, 3, 3] = val[v]
        elif v == "0":
            wt[:, 5] = 0.0
        else:
            wt[3, 2, 1, 1] = val[v]
    ref = F.conv2d(x, wt, None, 1, 1)
    wf, wd = ops.pack_conv3x3_weight(wt.to(DEV))
    xd = ops.amax_of(x.permute(0, 2, 3, 1).contiguous().to(DEV))
    out = ops.conv3x3_fwd(xd, wf).permute(0, 3, 1, 2).cpu()
    assert torch.equal(torch.isnan(out), torch.isnan(ref))
    assert torch.equal(torch.isinf(out), torch.isinf(ref))
    assert torch.equal(out[torch.isinf(ref)], ref[torch.isinf(ref)])
    fin = torch.isfinite(ref)
    assert float((out[fin] - ref[fin]).abs().max()) <= 1e-4
    if "inf" in what:
        # an infinite maximum: the launch took the six-product body -> the same bits as split3 mode
        lib.tune_set("mfma_products", 6)
        wf6, _ = ops.pack_conv3x3_weight(wt.to(DEV))
        out6 = ops.conv3x3_fwd(x.permute(0, 2, 3, 1).contiguous().to(DEV), wf6).permute(0, 3, 1, 2).cpu()
        lib.tune_set("mfma_products", 3)
        assert torch.equal(out.nan_to_num(7.0), out6.nan_to_num(7.0))


def test_every_producer_leaves_the_exact_maximum_in_its_slot(lib):
    """The epilogues that feed three-product GEMMs: BN + activation (+ pool), transposed convolution (+ skip), convolution data
    gradient, BN backward apply, the inference forms."""
    from resdepth_amd import ops
    g = torch.Generator().manual_seed(5)
    n, h, w, c = 2, 32, 32, 64
    z = (torch.randn(n, h, w, c, generator=g) * 3).to(DEV)
    mean, invstd = torch.randn(c, generator=g).to(DEV) * 0.1, (torch.rand(c, generator=g) + 0.5).to(DEV)
    gamma, beta = (torch.rand(c, generator=g) + 0.5).to(DEV), torch.randn(c, generator=g).to(DEV) * 0.1
    with lib.AmaxPool(DEV):
        a, _, _ = ops.bn_act_pool_fwd(z, mean, invstd, gamma, beta, 0.0, False)
        assert _slot_max(a) == float(a.abs().max())
        _, p, idx = ops.bn_act_pool_fwd(z, mean, invstd, gamma, beta, 0.01, True, want_a=False)
        assert _slot_max(p) == float(p.abs().max())
        wt = (torch.randn(c, c, 2, 2, generator=g) * 0.1).to(DEV)
        wtf, wtd = ops.pack_convt2x2_weight(wt)
        bias = torch.randn(c, generator=g).to(DEV)
        skip = torch.randn(n, 2 * h, 2 * w, c, generator=g).to(DEV)
        s = ops.convt2x2_fwd(a, wtf, bias, skip)
        assert _slot_max(s) == float(s.abs().max())
        s2 = ops.convt2x2_fwd_bnskip(a, wtf, bias, skip, mean, invstd, gamma, beta, 0.0)
        assert _slot_max(s2) == float(s2.abs().max())
        w3 = (torch.randn(c, c, 3, 3, generator=g) * 0.05).to(DEV)
        wf, wd = ops.pack_conv3x3_weight(w3)
        gy = ops.amax_of(torch.randn(n, h, w, c, generator=g).to(DEV) * 1e-4)
        dx = ops.conv3x3_bwd_data(gy, wd)
        assert _slot_max(dx) == float(dx.abs().max())
        sums = ops.bn_act_bwd_reduce(z, mean, invstd, gamma, beta, 0.0, gy, None, None)
        dz = ops.bn_act_bwd_apply(z, mean, invstd, gamma, beta, 0.0, gy, None, None, sums, float(n * h * w), True)
        assert _slot_max(dz) == float(dz.abs().max())
        # inference forms: folded convolution + activation (+ pool) -- 64-channel levels take the patch kernels
        shift = torch.randn(c, generator=g).to(DEV) * 0.1
        wff = ops.pack_conv3x3_weight_folded(w3, gamma * invstd)
        aa, pp = ops.conv3x3_fwd_act(a, wff, shift, 0.0, pool=True)
        assert _slot_max(aa) == float(aa.abs().max()) and _slot_max(pp) == float(pp.abs().max())
        x0 = torch.randn(n, 3, 64, 64, generator=g).to(DEV)
        w0 = (torch.randn(c, 3, 3, 3, generator=g) * 0.2).to(DEV)
        if ops.conv3x3_first_fwd_act_available(x0, c):
            a0, p0 = ops.conv3x3_first_fwd_act(x0, w0, mean, invstd, gamma, beta, 0.0, None, pool=True)
            assert _slot_max(p0) == float(p0.abs().max())


@pytest.mark.parametrize("c,n,h,w", [(64, 2, 32, 32), (64, 3, 16, 48), (128, 2, 16, 32), (128, 1, 32, 64)])
def test_fwd_act_commits_both_slots_exactly_when_the_pool_drops_the_maximum(lib, c, n, h, w):
    """rd_conv3x3_fwd_act with pool=True commits twice in a row (out slot, pooled slot): the 64- and 128-channel patch kernels at
    a LeakyReLU slope > 0 on data whose largest |a| is a negative value that the max-pool drops.  Each slot must hold exactly its
    tensor's maximum (amax_commit's trailing barrier: the second commit must not overwrite the first one's LDS words)."""
    from resdepth_amd import ops
    g = torch.Generator().manual_seed(c + h)
    x = ops.amax_of(torch.randn(n, h, w, 64, generator=g).to(DEV))
    w3 = (torch.randn(c, 64, 3, 3, generator=g) * 0.05).to(DEV)
    shift = torch.randn(c, generator=g).to(DEV) * 0.1
    shift[c // 3] = -60.0                 # one channel far below zero: its most negative a is the largest |a|, never pooled
    wff = ops.pack_conv3x3_weight_folded(w3, (torch.rand(c, generator=g) + 0.5).to(DEV))
    with lib.AmaxPool(DEV):
        aa, pp = ops.conv3x3_fwd_act(x, wff, shift, 0.5, pool=True)
    amax_a, amax_p = float(aa.abs().max()), float(pp.abs().max())
    assert amax_a > amax_p and float(aa.min()) == -amax_a, "the construction must put the largest |a| where the pool drops it"
    assert _slot_max(aa) == amax_a and _slot_max(pp) == amax_p


def test_a_rejected_call_leaves_no_slots_armed(lib):
    """rd_quant_next arms slots for the NEXT call; a call that fails its argument checks (here: a workspace too small) must clear
    them, or the next ordinary call of this thread would take them (include/resdepth_hip.h)."""
    import threading
    from resdepth_amd import ops
    L = lib.load()
    g = torch.Generator().manual_seed(17)
    n, h, w, c = 2, 16, 16, 64
    z = (torch.randn(n, h, w, c, generator=g) * 3).to(DEV)
    mean, invstd = torch.randn(c, generator=g).to(DEV) * 0.1, (torch.rand(c, generator=g) + 0.5).to(DEV)
    gamma, beta = (torch.rand(c, generator=g) + 0.5).to(DEV), torch.randn(c, generator=g).to(DEV) * 0.1
    x = torch.randn(n, h, w, c, generator=g).to(DEV)
    wf, _ = ops.pack_conv3x3_weight((torch.randn(c, c, 3, 3, generator=g) * 0.05).to(DEV))
    zz = torch.empty(n, h, w, c, device=DEV)
    sums = torch.empty(2 * c, dtype=torch.float64, device=DEV)
    armed = [torch.zeros(lib.AMAX_WORDS, dtype=torch.int32, device=DEV) for _ in range(4)]

    def ordinary():
        a, p, _ = ops.bn_act_pool_fwd(z, mean, invstd, gamma, beta, 0.01, True)      # a producer, no pool: no rd_quant_next
        return a, p, ops.conv3x3_fwd(x, wf)                                          # a consumer without slots
    L.rd_quant_next(*[t.data_ptr() for t in armed])
    rc = L.rd_conv3x3_fwd_stats(x.data_ptr(), wf.data_ptr(), zz.data_ptr(), sums.data_ptr(), n, h, w, c, c, None, 0,
                                torch.cuda.current_stream().cuda_stream)
    assert rc != 0 and b"workspace" in L.rd_last_error_string()
    got = ordinary()
    torch.cuda.synchronize()
    fresh = []
    t = threading.Thread(target=lambda: fresh.append(ordinary()))
    t.start()
    t.join()
    torch.cuda.synchronize()
    assert all(int(s.abs().max()) == 0 for s in armed), "a slot armed before the rejected call was taken by a later one"
    for a, b in zip(got, fresh[0]):
        assert torch.equal(a, b)


def test_results_are_bit_reproducible_and_weight_gradients_match_fp64(lib):
    from resdepth_amd import ops
    g = torch.Generator().manual_seed(9)
    n, h, w, ci, co = 4, 32, 32, 128, 64
    x = torch.randn(n, h, w, ci, generator=g).to(DEV)
    dz = (torch.randn(n, h, w, co, generator=g) * 1e-5).to(DEV)      # gradient-sized magnitudes: far below fp16's own range
    outs = []
    for _ in range(2):
        outs.append(ops.conv3x3_bwd_weight(ops.amax_of(x.clone()), ops.amax_of(dz.clone())))
    assert torch.equal(outs[0], outs[1])
    ref = torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2).double().cpu(), (co, ci, 3, 3), dz.permute(0, 3, 1, 2).double().cpu(),
                                      stride=1, padding=1)
    rel = float((outs[0].double().cpu() - ref).norm() / ref.norm())
    assert rel <= 2e-6, rel


def test_whole_net_parity_in_split3_mode_in_a_child_process():
    """The six-product arithmetic stays a tested configuration: the reference fixtures, the full-size step and cfg-S under the
    oracle with RD_MFMA=split3 (the library reads the switch once, at load time)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RESDEPTH_HIP_LIB", "RD_TUNE")}
    env["RD_MFMA"] = "split3"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_unet_gpu.py"), "-q", "-x", "-m", "gpu",
                        "-k", "tiny_net_against_reference_fixture or full_size_against_oracle_and_reference_digest or "
                              "(other_baseline_configs_against_oracle and cfg-S) or determinism_and_tile_independence"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=2400)
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
