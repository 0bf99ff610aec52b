"""The last convolution's skip term taken in level 0's BN / activation / pool pass (-m gpu; include/resdepth_hip_tail.h,
UNet.fold_tail_skip): ops.bn_act_pool_fwd_tailskip + ops.conv3x3_last_fwd_tail_pre must give the BITS of the pair they replace,
ops.bn_act_pool_fwd + ops.conv3x3_last_fwd_tail, which stay as the fallback and are the reference here -- pooled values, arg-max
bytes, z at the arg-max, the magnitude slot and the network's output; a model with the path on must train exactly like one with
it off; and a launch plan must hold the two new launches.

The magnitude slot.  A producer block commits its maximum to line (blockIdx & 15) of the slot, and its smallest non-zero block
maximum (complemented) to word 1 of that line (rd_mfma_dev.h: amax_commit).  The reference kernel's blocks are element ranges,
the fused kernel's are 16 x 32 image tiles, so the sixteen lines cannot hold the same words one by one; what a consumer reads is
their maximum (amax_read_wave2).  Checked here: the word-0 maximum equals the reference's bit for bit, and EVERY word of the fused
slot equals what the documented rule gives for the reference's pooled tensor cut into tiles (computed on the host)."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32 = torch.int32
TILE_H, TILE_W = 16, 32                # ET_H, ET_W of rd_edge_conv.hip


def bits(t):
    return t.contiguous().view(I32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def _inputs(n, h, w, c0, slope_kind, cin=16):
    """Seeded operands of one case on the device; slope_kind: 0.0, 0.2 or "prelu" (a device-resident slope).  Planted in z
    (NHWC), each in a pooling window of its own and each in a different tile position: four equal values (the first must win),
    a window that a ReLU clamps to zero in all four places, a NaN (it must win and reach pooled, zpool and nine outputs), -0.0."""
    g = torch.Generator().manual_seed(1000 * n + 10 * h + w + c0)
    z = torch.randn(n, h, w, c0, generator=g)
    mean, invstd = torch.randn(c0, generator=g) * 0.2, torch.rand(c0, generator=g) + 0.5
    gamma, beta = torch.rand(c0, generator=g) + 0.5, torch.randn(c0, generator=g) * 0.3      # gamma > 0: z = -100 gives y < 0
    z[0, 0:2, 0:2, 1] = 0.75                          # top-left corner of the image
    z[n - 1, h - 2:h, w - 2:w, c0 - 1] = -100.0       # bottom-right corner (a ragged tile where h, w are no tile multiples)
    z[0, 2:4, 4:6, :] = -100.0                        # every channel of a window
    z[0, 5, 7, 2] = float("nan")
    z[n - 1, h - 1, 0, 0] = float("nan")              # on the image border: its ring neighbours are zero padding
    z[0, 8, 10, 3] = -0.0
    z[0, 8:10, 12:14, 5] = -0.0
    wt = torch.randn(cin, c0, 2, 2, generator=g) / cin ** 0.5
    bt = torch.randn(c0, generator=g) * 0.2
    wl = torch.randn(1, c0, 3, 3, generator=g) / 3
    bl = torch.randn(1, generator=g)
    xc = torch.randn(n, h // 2, w // 2, cin, generator=g)
    xin = torch.randn(n, 3, h, w, generator=g)
    d = {k: v.to(DEV) for k, v in dict(z=z, mean=mean, invstd=invstd, gamma=gamma, beta=beta, wt=wt, bt=bt, wl=wl, bl=bl, xc=xc,
                                        xin=xin).items()}
    d["slope"], d["slope_dev"] = (0.0, torch.tensor([0.15], device=DEV)) if slope_kind == "prelu" else (slope_kind, None)
    return d


def _expected_slot(p):
    """The sixteen (word 0, word 1) pairs amax_commit leaves for pooled tensor p [n, h2, w2, c] when a block is one 16 x 32
    image tile = 8 x 16 pooled pixels, tiles numbered image-major, row-major: word 0 of line l = the largest |p| bits over the
    tiles with index = l (mod 16), a NaN ignored (v_max); word 1 = the largest complement of a non-zero tile maximum."""
    n, h2, w2, _ = p.shape
    mag = torch.nan_to_num(p.abs(), nan=0.0, posinf=float("inf")).cpu()
    th, tw = TILE_H // 2, TILE_W // 2
    w0, w1 = [0] * 16, [0] * 16
    tl = 0
    for img in range(n):
        for ty in range(-(-h2 // th)):
            for tx in range(-(-w2 // tw)):
                m = int(mag[img, ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].max().view(I32))
                line = tl & 15
                w0[line] = max(w0[line], m)
                if m:
                    w1[line] = max(w1[line], 0xFFFFFFFF - m)
                tl += 1
    return w0, w1


def _slot_words(slot):
    s = slot.view(16, -1).cpu().to(torch.int64) & 0xFFFFFFFF
    assert int((s[:, 2:] != 0).sum()) == 0, "words beyond 0 and 1 of a line were written"
    return [int(v) for v in s[:, 0]], [int(v) for v in s[:, 1]]


SHAPES = [(1, 16, 32, 64),       # one tile, all four borders
          (2, 34, 66, 64),       # ragged tiles in both directions
          (3, 32, 64, 16),       # LP = 2
          (1, 18, 34, 32)]       # LP = 4, ragged


@pytest.mark.parametrize("slope_kind", [0.0, 0.2, "prelu"])
@pytest.mark.parametrize("n,h,w,c0", SHAPES)
def test_the_fused_pair_gives_the_bits_of_the_pair_it_replaces(n, h, w, c0, slope_kind):
    from resdepth_amd import _lib, ops
    d = _inputs(n, h, w, c0, slope_kind)
    bn = (d["mean"], d["invstd"], d["gamma"], d["beta"])
    with _lib.AmaxPool(DEV):
        _, p_ref, idx_ref, zp_ref = ops.bn_act_pool_fwd(d["z"], *bn, d["slope"], True, d["slope_dev"], want_a=False, want_zpool=True)
        p, idx, zp, skip9 = ops.bn_act_pool_fwd_tailskip(d["z"], *bn, d["slope"], d["wl"], d["slope_dev"], want_zpool=True)
        p_nz, idx_nz, zp_nz, skip9_nz = ops.bn_act_pool_fwd_tailskip(d["z"], *bn, d["slope"], d["wl"], d["slope_dev"])
    assert same_bits(p, p_ref) and same_bits(idx, idx_ref) and same_bits(zp, zp_ref)
    assert zp_nz is None and same_bits(p_nz, p_ref) and same_bits(idx_nz, idx_ref) and same_bits(skip9_nz, skip9)
    # the planted values did what they were planted for
    assert int(idx_ref[0, 0, 0, 1]) == 0 and float(p_ref[0, 0, 0, 1]) == float(p_ref[0, 0, 0, 1])       # equal values: the first
    assert bool(torch.isnan(p_ref[0, 2, 3, 2])) and bool(torch.isnan(zp_ref[0, 2, 3, 2])) and int(idx_ref[0, 2, 3, 2]) == 3
    assert bool(torch.isnan(p_ref[n - 1, h // 2 - 1, 0, 0])) and bool(torch.isnan(skip9[n - 1, h - 1, 0]))
    if slope_kind == 0.0:
        assert float(p_ref[0, 1, 2].abs().max()) == 0.0 and int(idx_ref[0, 1, 2].max()) == 0           # all clamped: the first
    # the magnitude slot (three-product mode; elsewhere nobody asks for one)
    s_ref, s_new = _lib.slot_of(p_ref), _lib.slot_of(p)
    assert (s_ref is None) == (s_new is None)
    if s_new is not None:
        (r0, _), (g0, g1) = _slot_words(s_ref), _slot_words(s_new)
        assert max(g0) == max(r0) and max(g0) > 0, "the slot's maximum differs from the reference's"
        assert (g0, g1) == _expected_slot(p_ref), "the slot's words are not those of one commit per 16 x 32 tile"
        assert _slot_words(_lib.slot_of(p_nz)) == (g0, g1)
    # the network's output through both tails, with and without bias, with and without the outer residual
    skip = {"z": d["z"], "mean": bn[0], "invstd": bn[1], "gamma": bn[2], "beta": bn[3], "slope": d["slope"], "slope_dev": d["slope_dev"]}
    _, v, _, b9 = ops.tail_compose(d["wt"], d["wl"], d["bt"], forward=True)
    t16 = ops.tail_t16(d["xc"], v)
    for bias in (d["bl"], None):
        for xres in (d["xin"], None):
            want = ops.conv3x3_last_fwd_tail(skip, t16, b9, d["wl"], bias, xres)
            got = ops.conv3x3_last_fwd_tail_pre(skip9, t16, b9, bias, xres)
            assert same_bits(got, want), (bias is not None, xres is not None)
            assert int(torch.isnan(want).sum()) == 9 + 4          # an interior NaN reaches nine outputs, a corner NaN four


def test_the_fused_pair_against_torch_in_fp64():
    """`out` of the fused pair against torch in fp64 on the materialised tensors (lib/UNet.py:218-244), at the tolerance of the
    same check of rd_conv3x3_last_fwd_tail (tests/test_ops_gpu.py: rel-L2 3e-6, max-abs 50 x that), on the ragged shape; the
    pooled outputs against F.max_pool2d of the materialised activation."""
    from resdepth_amd import ops
    from test_ops_gpu import close
    n, h, w, cin, c0, slope = 2, 34, 66, 16, 64, 0.2
    g = torch.Generator().manual_seed(5)
    xc = torch.randn(n, cin, h // 2, w // 2, generator=g)
    z = torch.randn(n, c0, h, w, generator=g)
    wt = torch.randn(cin, c0, 2, 2, generator=g) / cin ** 0.5
    bt, wl, bl = torch.randn(c0, generator=g) * 0.2, torch.randn(1, c0, 3, 3, generator=g) / 3, torch.randn(1, generator=g)
    xin = torch.randn(n, 3, h, w, generator=g)
    mean, invstd = torch.randn(c0, generator=g) * 0.2, torch.rand(c0, generator=g) + 0.5
    gamma, beta = torch.randn(c0, generator=g), torch.randn(c0, generator=g) * 0.3
    y = (z.double() - mean.double().view(1, -1, 1, 1)) * (invstd.double() * gamma.double()).view(1, -1, 1, 1) + beta.double().view(1, -1, 1, 1)
    a0 = torch.where(y > 0, y, y * slope)
    s = F.conv_transpose2d(xc.double(), wt.double(), bt.double(), stride=2) + a0
    out_ref = F.conv2d(s, wl.double(), bl.double(), padding=1) + xin.double()[:, 0:1]
    to = lambda t: t.to(DEV)                                                                          # noqa: E731
    zh, xch = to(z.permute(0, 2, 3, 1).contiguous()), to(xc.permute(0, 2, 3, 1).contiguous())
    p, _, _, skip9 = ops.bn_act_pool_fwd_tailskip(zh, to(mean), to(invstd), to(gamma), to(beta), slope, to(wl))
    _, v, _, b9 = ops.tail_compose(to(wt), to(wl), to(bt), forward=True)
    out = ops.conv3x3_last_fwd_tail_pre(skip9, ops.tail_t16(xch, v), b9, to(bl), to(xin))
    close(out.cpu(), out_ref.float(), tol=3e-6, name="fused tail forward")
    close(p.permute(0, 3, 1, 2).cpu(), F.max_pool2d(a0, 2).float(), tol=3e-6, name="pooled")


def test_shapes_the_kernel_does_not_take_are_refused():
    from resdepth_amd import ops
    one = torch.ones(24, device=DEV)
    z = torch.zeros(1, 4, 4, 24, device=DEV)
    with pytest.raises(RuntimeError, match="C in"):
        ops.bn_act_pool_fwd_tailskip(z, one, one, one, one, 0.0, torch.zeros(1, 24, 3, 3, device=DEV))


# ---- model level ----------------------------------------------------------------------------------------------------------------
def _batch(n=2, h=32, w=64, seed=21):
    g = torch.Generator().manual_seed(seed)
    x, t = torch.randn(n, 3, h, w, generator=g).to(DEV), torch.randn(n, 1, h, w, generator=g).to(DEV)
    mask = (torch.rand(n, 1, h, w, generator=g) > 0.2).to(torch.uint8).to(DEV)
    return x, t, mask, torch.zeros(n, device=DEV), torch.ones(n, device=DEV) * 2.0


class _count_fused:
    """how often the forward took the fused level-0 op"""

    def __enter__(self):
        from resdepth_amd import ops
        self.ops, self.orig, self.calls = ops, ops.bn_act_pool_fwd_tailskip, 0

        def counted(*a, **kw):
            self.calls += 1
            return self.orig(*a, **kw)
        ops.bn_act_pool_fwd_tailskip = counted
        return self

    def __exit__(self, *exc):
        self.ops.bn_act_pool_fwd_tailskip = self.orig
        return False


def _two_models(**kw):
    from resdepth_amd import UNet
    kw = dict(dict(n_input_channels=3, start_kernel=16, depth=2), **kw)
    torch.manual_seed(3)
    sd = copy.deepcopy(UNet(**kw).state_dict())
    models = []
    for fold in (True, False):
        m = UNet(**kw)
        m.load_state_dict(sd)
        m = m.to(DEV).train()
        assert m.fold_tail_skip is True, "the path is the default"
        m.fold_tail_skip = fold
        models.append(m)
    return models


@pytest.mark.parametrize("kw,expect_fused", [(dict(), 1), (dict(act_fn_encoder="prelu", act_fn_decoder="lrelu"), 1),
                                             (dict(do_BN=False, bias_conv_layer=True), 1), (dict(depth=1), 1),
                                             (dict(start_kernel=8), 0), (dict(up_mode="bilinear"), 0)])
def test_a_model_trains_the_same_bits_with_the_path_on_and_off(kw, expect_fused):
    """forward + loss + backward of two models from one seed: output, loss, every gradient and the BN running statistics.  A C0
    outside {16, 32, 64} and a bilinear decoder fall back (no fused launch) and match as well."""
    from resdepth_amd import masked_l1_loss
    on, off = _two_models(**kw)
    batch = _batch()
    res = []
    for m in (on, off):
        with _count_fused() as cnt:
            out = m(batch[0])
            loss = masked_l1_loss(out, *batch[1:])
            loss.backward()
            torch.cuda.synchronize()
        res.append((out.detach(), loss.detach(), cnt.calls))
    assert res[0][2] == expect_fused and res[1][2] == 0
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    for (k, a), (_, b) in zip(on.named_parameters(), off.named_parameters()):
        assert a.grad is not None and torch.equal(a.grad, b.grad), k
    for (k, a), (_, b) in zip(on.named_buffers(), off.named_buffers()):
        assert torch.equal(a, b), k


def test_the_other_forwards_take_the_path_and_a_kept_skip_falls_back():
    """The no-grad training-mode forward and the unfolded eval forward go through the fused op and match; keep_skips=True (the
    skip activation is a tensor: the two-kernel tail) does not, and matches too."""
    on, off = _two_models()
    x = _batch()[0]
    with torch.no_grad():
        with _count_fused() as cnt:
            a, b = on(x), off(x)
        assert cnt.calls == 1 and torch.equal(a, b)
    for m in (on, off):
        m.eval()
        m.fold_eval_bn = False
    with torch.no_grad():
        with _count_fused() as cnt:
            a, b = on(x), off(x)
        assert cnt.calls == 1 and torch.equal(a, b)
    on.train(), off.train()
    with _count_fused() as cnt:
        (a, sa), (b, sb) = (m._engine_forward(x, True, save=True, keep_skips=True) for m in (on, off))
    assert cnt.calls == 0 and torch.equal(a, b) and torch.equal(sa["enc"][0]["a"], sb["enc"][0]["a"])


def test_a_launch_plan_holds_the_two_launches():
    """PlannedTrainStep at the model-level shape with the path on: recorded, the first replay verified (not rejected), and the
    replayed losses and final state those of the eager iteration."""
    from resdepth_amd import FusedAdam, UNet
    from resdepth_amd.plan import PlannedTrainStep
    kw = dict(n_input_channels=3, start_kernel=16, depth=2)
    torch.manual_seed(3)
    sd = copy.deepcopy(UNet(**kw).state_dict())
    batches = [_batch(seed=30), _batch(seed=31)]
    res = []
    for planned in (False, True):
        m = UNet(**kw)
        m.load_state_dict(sd)
        m = m.to(DEV).train()
        assert m.fold_tail_skip
        opt = FusedAdam(m.parameters(), lr=2e-3, weight_decay=1e-5)
        step = PlannedTrainStep(m, opt, warmup=1 if planned else 1 << 60)
        with _count_fused() as cnt:
            losses, how = [], []
            for k in range(5):
                losses.append(step(*batches[k % 2]).clone())
                how.append(step.why_eager)
            torch.cuda.synchronize()
        res.append((m, torch.stack(losses).cpu(), how, step, cnt.calls))
    (me, le, _, _, calls_e), (mp, lp, how, step, _) = res
    assert calls_e == 5
    assert step.plan_rejected is None, step.plan_rejected
    assert how[-1] is None and step.replays >= 2, how
    assert torch.equal(le, lp), (le, lp)
    for k, v in me.state_dict().items():
        assert torch.equal(v, mp.state_dict()[k]), k
