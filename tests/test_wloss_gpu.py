"""Per-pixel weights for the fused training losses on the GPU (-m gpu; include/resdepth_hip_wloss.h): masked_loss(weight=...)
against the fp64 oracle of tests/wloss_ref.py over the shapes, masks, kinds and slope weights of tests/test_loss_gpu.py (they
cross the strip, the grid cap, and the scalar and vector paths), bit identity with the unweighted family at w == 1, the
global normalisers under data parallelism, the weight tiles GpuTrainSet / GpuValSet cut from HBM rasters against a numpy
reference, and the Trainer, GraphedTrainStep and PlannedTrainStep with a weight.

Bars (derived as in tests/test_loss_gpu.py, not measured): r is bit-identical in kernel and oracle, the sums are fp64, every
term of D, S, Q, Wc is non-negative and each fp32 result is one rounding of an fp64 value: 1e-6 relative on loss and MAE and
1e-6 * (|g_data| + |g_slope|) per gradient element leave room for a handful of 2^-24 roundings."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

import loss_ref
import wloss_ref
from test_graph_gpu import KW, _batches, _fresh, _same_state
from test_loss_gpu import LAMBDAS, MASKS, SHAPES, SPECS, TKW, _data, _loaders, _OtherHalf, _trainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WEIGHTS = ["uniform", "levels"]


def _weights(shape, mask, which, seed=0):
    """uniform in [0, 4] with about 20 % exact zeros, or values in {0, 1, 3}; the first seed that leaves Wc > 0."""
    m = mask.reshape(shape) != 0
    for s in range(seed, seed + 64):
        g = torch.Generator().manual_seed(7919 * s + sum(shape) + len(which))
        if which == "uniform":
            w = torch.rand(shape, generator=g) * 4.0
            w[torch.rand(shape, generator=g) < 0.2] = 0.0
        else:
            w = torch.tensor([0.0, 1.0, 3.0])[torch.randint(0, 3, shape, generator=g)]
        if float((w * m).sum()) > 0.0:
            return w
    raise AssertionError("no weight plane with Wc > 0")


def _run(yp, y, m, w, mean, std, kind, delta, lam, gout=None, **kw):
    """-> loss, mae (python floats), gradient (host, fp32)"""
    from resdepth_amd import masked_loss
    x = yp.to(DEV).requires_grad_()
    loss, mae = masked_loss(x, y.to(DEV), m.to(DEV), mean, std, kind=kind, delta=delta, slope_weight=lam, return_mae=True,
                            weight=w.to(DEV), **kw)
    assert loss.shape == () and mae.shape == () and not mae.requires_grad
    (loss if gout is None else gout * loss).backward()
    return float(loss.detach()), float(mae), x.grad.cpu()


def _judge(got, o, mask, w=None, lam=None):
    loss, mae, grad = got
    assert abs(loss - o["loss"]) <= 1e-6 * o["loss"], (loss, o["loss"])
    assert abs(mae - o["mae"]) <= 1e-6 * o["mae"], (mae, o["mae"])
    want = o["g_data"] + o["g_slope"]
    bar = 1e-6 * (o["g_data"].abs() + o["g_slope"].abs())
    err = (grad.double() - want).abs()
    assert bool((err <= bar).all()), (float((err - bar).max()), int((err > bar).sum()))
    assert int((grad[mask.reshape(grad.shape) == 0] != 0).sum()) == 0          # exactly 0 at masked pixels
    if w is not None and lam == 0.0:
        assert int((grad[w.reshape(grad.shape) == 0] != 0).sum()) == 0         # exactly 0 data gradient at w = 0 pixels


def _params():
    out = []
    for shape in SHAPES:
        for mk in MASKS:
            if mk == "sample_masked" and shape[0] == 1:
                continue                                  # needs a second sample to keep C > 0
            out.append(pytest.param(shape, mk, id="x".join(map(str, shape)) + "-" + mk))
    return out


@pytest.mark.parametrize("shape,mask_kind", _params())
def test_loss_mae_and_gradient_against_the_oracle(shape, mask_kind):
    yp, y, m, mean, std = _data(shape, mask_kind)
    plain_mae = loss_ref.masked_loss_oracle(yp, y, m, mean, std, "l1", 1.0, 0.0)["mae"]
    for which in WEIGHTS:
        w = _weights(shape, m, which)
        for kind, delta in SPECS:
            for lam in LAMBDAS:
                o = wloss_ref.weighted_loss_oracle(yp, y, m, w, mean, std, kind, delta, lam)
                assert o["Wc"] > 0.0 and o["C"] > 0.0
                assert o["mae"] == plain_mae                                   # the MAE does not see the weights
                got = _run(yp, y, m, w, mean, std, kind, delta, lam)
                _judge(got, o, m, w, lam)
                if o["Q"] == 0.0:
                    assert float(o["g_slope"].abs().max()) == 0.0
                    assert got[0] == _run(yp, y, m, w, mean, std, kind, delta, 0.0)[0] and got[0] == got[0]


@pytest.mark.parametrize("lam", LAMBDAS)
def test_all_zero_weights_give_a_nan_loss_and_a_zero_gradient(lam):
    """Wc == 0 with valid pixels: what C == 0 gives the unweighted loss; the MAE stays the plain masked MAE."""
    yp, y, m, mean, std = _data((2, 1, 8, 16), "bernoulli")
    w = torch.zeros(2, 1, 8, 16)
    o = wloss_ref.weighted_loss_oracle(yp, y, m, w, mean, std, "huber", 0.5, lam)
    assert o["Wc"] == 0.0 and o["Q"] == 0.0 and o["C"] > 0.0
    loss, mae, grad = _run(yp, y, m, w, mean, std, "huber", 0.5, lam)
    assert loss != loss and abs(mae - o["mae"]) <= 1e-6 * o["mae"]
    assert int((grad != 0).sum()) == 0 and bool(torch.isfinite(grad).all())
    # and no valid pixel at all: both NaN, zeros
    loss, mae, grad = _run(yp, y, torch.zeros_like(m), torch.ones_like(w), mean, std, "l2", 1.0, lam)
    assert loss != loss and mae != mae and int((grad != 0).sum()) == 0


def _three(fn, yp):
    x = yp.to(DEV).requires_grad_()
    loss, mae = fn(x)
    loss.backward()
    return loss.detach().clone(), mae.clone(), x.grad.clone()


@pytest.mark.parametrize("shape", [(3, 1, 5, 7), (2, 1, 8, 16), (1, 1, 6, 300), (3, 1, 64, 64), (1100, 1, 2, 3)],
                         ids=lambda s: "x".join(map(str, s)))
def test_unit_weights_give_the_bits_of_the_unweighted_loss(shape):
    from resdepth_amd import masked_l1_loss, masked_loss
    yp, y, m, mean, std = _data(shape, "bernoulli")
    yd, md, one = y.to(DEV), m.to(DEV), torch.ones(shape, device=DEV)
    for kind, delta in SPECS:
        for lam in LAMBDAS:
            if kind == "l1" and lam == 0.0:
                continue
            kw = dict(kind=kind, delta=delta, slope_weight=lam, return_mae=True)
            a = _three(lambda x: masked_loss(x, yd, md, mean, std, **kw), yp)
            b = _three(lambda x: masked_loss(x, yd, md, mean, std, weight=one, **kw), yp)
            c = _three(lambda x: masked_loss(x, yd, md, mean, std, weight=one[:, 0], **kw), yp)        # [N,H,W]
            for u, v, z in zip(a, b, c):
                assert torch.equal(u, v) and torch.equal(u, z), (kind, lam)
    # plain L1 has kernels of its own (another summation order): within the bar
    x = yp.to(DEV).requires_grad_()
    l1 = masked_l1_loss(x, yd, md, mean, std)
    l1.backward()
    lw, mw, gw = _three(lambda x: masked_loss(x, yd, md, mean, std, kind="l1", return_mae=True, weight=one), yp)
    assert abs(float(lw) - float(l1)) <= 1e-6 * float(l1) and abs(float(mw) - float(l1)) <= 1e-6 * float(l1)
    assert bool(((gw - x.grad).abs() <= 1e-6 * x.grad.abs()).all())


def test_a_weight_offset_by_four_bytes_takes_the_scalar_path_with_the_same_bits():
    from resdepth_amd import masked_loss
    shape = (2, 1, 8, 16)
    yp, y, m, mean, std = _data(shape, "bernoulli")
    w = _weights(shape, m, "uniform")
    numel = w.numel()
    res = []
    for off in (0, 1):
        buf = torch.zeros(numel + 4, device=DEV)
        buf[off:off + numel] = w.reshape(-1).to(DEV)
        wd = buf[off:off + numel].view(shape)
        assert wd.is_contiguous() and (wd.data_ptr() % 16 == 0) == (off == 0)
        for lam in LAMBDAS:
            res.append(_three(lambda x: masked_loss(x, y.to(DEV), m.to(DEV), mean, std, kind="huber", delta=0.5, slope_weight=lam,
                                                    return_mae=True, weight=wd), yp))
    for a, b in zip(res[:2], res[2:]):
        for u, v in zip(a, b):
            assert torch.equal(u, v)


def test_two_calls_give_the_same_bits():
    from resdepth_amd import masked_loss
    shape = (3, 1, 64, 64)
    yp, y, m, mean, std = _data(shape, "bernoulli")
    wd = _weights(shape, m, "uniform").to(DEV)
    res = [_three(lambda x: masked_loss(x, y.to(DEV), m.to(DEV), mean, std, kind="huber", delta=0.5, slope_weight=0.3,
                                        return_mae=True, weight=wd), yp) for _ in range(2)]
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_a_wrong_weight_shape_raises():
    from resdepth_amd import masked_loss
    yp, y, m, mean, std = _data((2, 1, 8, 16), "ones")
    for shape in ((2, 1, 8, 15), (1, 1, 8, 16), (2, 2, 8, 16), (2 * 8 * 16,)):
        with pytest.raises(ValueError, match="weight of shape"):
            masked_loss(yp.to(DEV), y.to(DEV), m.to(DEV), mean, std, kind="l2", weight=torch.ones(shape, device=DEV))
    with pytest.raises(RuntimeError, match="HIP device"):
        masked_loss(yp.to(DEV), y.to(DEV), m.to(DEV), mean, std, kind="l2", weight=torch.ones(2, 1, 8, 16))


def test_the_upstream_gradient_is_read_from_the_device():
    shape = (2, 1, 8, 16)
    yp, y, m, mean, std = _data(shape, "bernoulli")
    w = _weights(shape, m, "uniform")
    o = wloss_ref.weighted_loss_oracle(yp, y, m, w, mean, std, "huber", 0.5, 0.3, gout=2.5)
    got = _run(yp, y, m, w, mean, std, "huber", 0.5, 0.3, gout=torch.tensor(2.5, device=DEV))
    _judge(got, o, m)
    plain = _run(yp, y, m, w, mean, std, "huber", 0.5, 0.3)
    assert float(got[2].abs().max()) > 2.0 * float(plain[2].abs().max())


@pytest.mark.parametrize("kind,delta,lam", [("l2", 1.0, 0.3), ("huber", 0.5, 0.0), ("l1", 1.0, 0.3), ("l1", 1.0, 0.0)])
def test_the_normalisers_are_global_under_data_parallelism(kind, delta, lam):
    from resdepth_amd import masked_loss, ops
    from resdepth_amd.loss import _check_spec, _kernel_args, _prep
    shape = (4, 1, 9, 12)
    yp, y, m, mean, std = _data(shape, "bernoulli")
    w = _weights(shape, m, "uniform")
    code, d, scale = _kernel_args(*_check_spec(kind, delta, lam)[:2])

    def partial(h):
        a = _prep(yp[h].to(DEV), y[h], m[h], mean[h], std[h])
        return ops.weighted_loss_partial(a[0], a[1], a[2], w[h].to(DEV).contiguous(), a[3], a[4], code, d, scale)
    halves = [slice(0, 2), slice(2, 4)]
    part = [partial(h) for h in halves]
    whole = partial(slice(0, 4))
    assert torch.equal(whole[6:], torch.zeros(2, dtype=torch.float64, device=DEV)) and float(whole[5]) > 0.0
    grads, losses = [], []
    for i, h in enumerate(halves):
        sync = _OtherHalf(part[1 - i])
        x = yp[h].to(DEV).requires_grad_()
        loss = masked_loss(x, y[h].to(DEV), m[h].to(DEV), mean[h], std[h], kind=kind, delta=delta, slope_weight=lam, grad_sync=sync,
                           weight=w[h].to(DEV))
        loss.backward()
        grads.append(x.grad)
        losses.append(float(loss))
        assert float(sync.seen[1]) == float(whole[1])                                       # C: an integer count, exactly
        for slot in (4, 5):                              # fp64 sums of non-integers in another order
            assert abs(float(sync.seen[slot]) - float(whole[slot])) <= 2.0 ** -50 * float(whole[slot]), slot
        assert torch.equal(sync.seen[6:], torch.zeros(2, dtype=torch.float64, device=DEV))
    x = yp.to(DEV).requires_grad_()
    lw = masked_loss(x, y.to(DEV), m.to(DEV), mean, std, kind=kind, delta=delta, slope_weight=lam, weight=w.to(DEV))
    lw.backward()
    got, want = torch.cat(grads).double(), x.grad.double()
    assert bool(((got - want).abs() <= 2.0 ** -22 * want.abs()).all())
    assert abs(losses[0] - float(lw)) <= 1e-6 * float(lw) and abs(losses[1] - float(lw)) <= 1e-6 * float(lw)


# ---- weight tiles from HBM rasters --------------------------------------------------------------------------------------------
T = 8
TABLE = [0.0, 1.0, 3.0, 0.5, 2.0, 4.0]


def _rasters(f32_first):
    """Two rasters: 23 x 29 (rows that are no multiple of 4 pixels: the scalar path) and 24 x 32; one carries fp32 weights -- a
    COPY of its ground truth, so its weight tiles must be its raw target tiles -- and one uint8 classes with a table."""
    from resdepth_amd import GpuPatchSampler
    out, host = [], []
    for k, (h, w) in enumerate(((23, 29), (24, 32))):
        rng = np.random.RandomState(70 + k)
        gt = (rng.rand(h, w) * 50.0 + 400.0 + 100.0 * k).astype(np.float32)
        dsm = (gt + rng.randn(h, w)).astype(np.float32)
        orthos = (rng.rand(2, h, w) * 200 + 20).astype(np.float32)
        classes = rng.randint(0, len(TABLE), (h, w)).astype(np.uint8)
        f32 = (k == 0) == f32_first
        kw = dict(weight_raster=gt.copy()) if f32 else dict(weight_raster=classes, class_weights=TABLE)
        out.append(GpuPatchSampler(dsm, gt, orthos, tile_size=T, nodata=-9999.0, dsm_std=2.0 + k, ortho_std=50.0, **kw))
        host.append((gt, None) if f32 else (classes, TABLE))
    return out, host


def _datasets(samplers, **kw):
    return [dict(sampler=s, area_defn={"x_extent": [(0, s.w - 1)], "y_extent": [(0, s.h - 1)]}, image_pairs=[[0, 1]], **kw)
            for s in samplers]


@pytest.mark.parametrize("f32_first", [True, False], ids=["f32_23x29", "f32_24x32"])
def test_weight_tiles_are_the_numpy_reference_bit_for_bit(f32_first):
    from resdepth_amd import GpuTrainSet, GpuValSet
    samplers, host = _rasters(f32_first)
    np.random.seed(3)
    ts = GpuTrainSet(_datasets(samplers, n_samples=24), "geom-stereo", batch_size=48, transform_dsm=False)
    ids, pos, _ = ts.sample_list()
    n = len(ids)
    assert n == 48
    pos = pos.copy()
    pos[::2, 1] &= ~3                                       # rows that start 16-byte (fp32) / 4-byte (classes) aligned
    ts._cols[1], ts._cols[2] = pos[:, 0], pos[:, 1]
    # samples 2p (aligned) and 2p + 1 share code p: all four rotations with every flip combination on each raster
    aug = np.array([[(j // 2) % 4, (j // 8) % 2, (j // 16) % 2] for j in range(n)])
    for part in (aug[:24], aug[24:]):
        codes = {tuple(a) for a in part}
        assert len(codes) == 12 and {a[0] for a in codes} == {0, 1, 2, 3} and len({a[1:] for a in codes}) == 3
    assert len({tuple(a) for a in aug}) == 16
    b = ts.assemble(np.arange(n), aug=aug)
    assert set(b) >= {"input", "target", "loss_mask", "loss_weight"}
    lw = b["loss_weight"]
    assert lw.shape == (n, 1, T, T) and lw.dtype == torch.float32 and lw.is_contiguous()
    got = lw.cpu().numpy()
    vec_rows = 0
    for i in range(n):
        raster, table = host[ids[i]]
        want = wloss_ref.weight_tile(raster, table, pos[i], T, aug[i])
        assert np.array_equal(got[i, 0], want), (i, ids[i], pos[i], aug[i])
        vec_rows += int(ids[i] == 1 and aug[i][0] == 0 and aug[i][2] == 0 and pos[i][1] % 4 == 0)
        if table is None:                                   # the fp32 weights are the ground truth: oriented as the target is
            assert np.array_equal(got[i, 0], b["target"][i, 0].cpu().numpy()), i
    assert vec_rows >= 2                                    # the 24 x 32 raster took the wide loads
    # an iterated epoch carries the field, whatever the draws
    for batch in ts:
        assert batch["loss_weight"].shape == (batch["input"].shape[0], 1, T, T)
        assert bool(torch.isfinite(batch["loss_weight"]).all()) and float(batch["loss_weight"].min()) >= 0.0
    # validation tiles: box-flagged samples, no augmentation; the box cuts the mask, never the weights
    vs = GpuValSet(_datasets(samplers), "geom-stereo", batch_size=5, transform_dsm=False, stride=5)
    ds = vs.dataset
    k0 = 0
    for k in range(len(vs)):
        vb = vs.assemble(k)
        m = vb["input"].shape[0]
        assert vb["loss_weight"].shape == (m, 1, T, T)
        g = vb["loss_weight"].cpu().numpy()
        for i in range(m):
            raster, table = host[ds.dataset_id[k0 + i]]
            assert np.array_equal(g[i, 0], wloss_ref.weight_tile(raster, table, ds.pos[k0 + i], T, (0, 0, 0))), (k, i)
        k0 += m
    assert k0 == len(ds) and bool((~vb["loss_mask"]).any())              # some mask was cut by its box


def test_an_invalid_sample_row_gives_nan_weights():
    from resdepth_amd import GpuTrainSet
    samplers, _ = _rasters(True)
    np.random.seed(3)
    ts = GpuTrainSet(_datasets(samplers, n_samples=2), "geom-stereo", batch_size=4)
    tab = ts.table(np.arange(4))
    tab[1, 0], tab[0, 1], tab[2, 2] = 23 - T + 1, 7, -1                # below the raster, no such raster, left of the raster
    b = ts._assemble(torch.from_numpy(tab))
    lw = b["loss_weight"].cpu()
    assert bool(torch.isnan(lw[:3]).all()) and bool(torch.isfinite(lw[3]).all())
    assert bool(torch.isnan(b["input"][:3]).all())                      # as the patches do


def test_weights_are_checked_and_all_samplers_or_none_carry_them():
    from resdepth_amd import GpuPatchSampler, GpuTrainSet, GpuValSet
    samplers, _ = _rasters(True)
    z = np.zeros((23, 29), dtype=np.float32)
    plain = GpuPatchSampler(z + 400, z + 400, np.zeros((2, 23, 29), dtype=np.float32), tile_size=T)
    assert plain.weight is None
    for cls in (GpuTrainSet, GpuValSet):
        kw = dict(n_samples=2) if cls is GpuTrainSet else {}
        with pytest.raises(ValueError, match="weight raster"):
            cls(_datasets([samplers[0], plain], **kw), "geom-stereo", batch_size=2)
        b = next(iter(cls(_datasets([plain], **kw), "geom-stereo", batch_size=2)))
        assert "loss_weight" not in b
    bad = [dict(weight_raster=z - 1.0), dict(weight_raster=z + float("nan")), dict(weight_raster=z + float("inf")),
           dict(weight_raster=np.zeros((23, 28), dtype=np.float32)), dict(weight_raster=z.astype(np.uint8)),
           dict(weight_raster=z.astype(np.uint8), class_weights=[1.0, -1.0]), dict(weight_raster=z.astype(np.uint8), class_weights=[]),
           dict(weight_raster=z.astype(np.uint8), class_weights=[float("nan")]), dict(weight_raster=z, class_weights=[1.0]),
           dict(weight_raster=z.astype(np.uint8) + 2, class_weights=[1.0, 2.0]), dict(class_weights=[1.0]),
           dict(weight_raster=z.astype(np.uint8), class_weights=[1.0] * 257)]
    for kw in bad:
        with pytest.raises(ValueError, match="weight"):
            GpuPatchSampler(z + 400, z + 400, None, tile_size=T, **kw)


# ---- Trainer ------------------------------------------------------------------------------------------------------------------
class _WithWeights:
    """A loader whose batches carry a host `loss_weight` (what a DataLoader over a weighted dataset yields)."""

    def __init__(self, loader, seed):
        self.loader, self.seed = loader, seed
        self.dataset, self.batch_size, self.drop_last = loader.dataset, loader.batch_size, False

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for k, batch in enumerate(self.loader):
            yield dict(batch, loss_weight=_weights(tuple(batch["target"].shape), batch["loss_mask"], "uniform", seed=self.seed + k))


@pytest.fixture(scope="module")
def sd0():
    from resdepth_amd import UNet
    torch.manual_seed(0)
    return copy.deepcopy(UNet(**TKW).state_dict())


def _hand_epoch(sd0, loader, loss_fn):
    """The Trainer's train epoch as a plain loop -> model, optimizer, losses, plain masked MAEs of the predictions"""
    from resdepth_amd import FusedAdam, UNet, masked_l1_loss
    model = UNet(**TKW)
    model.load_state_dict(sd0)
    model = model.to(DEV).train()
    opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=1e-5)
    losses, maes = [], []
    for batch in loader:
        x, y, m = batch["input"].to(DEV), batch["target"].to(DEV), batch["loss_mask"].to(DEV)
        mean, std = torch.flatten(batch["dsm_mean"]), torch.flatten(batch["dsm_std"])
        y_pred = model(x)
        with torch.no_grad():
            maes.append(float(masked_l1_loss(y_pred.detach(), y, m, mean, std)))
        w = batch.get("loss_weight")
        loss = loss_fn(y_pred, y, m, mean, std, None if w is None else w.to(DEV))
        loss.backward()
        losses.append(float(loss.detach().double()))
        opt.step()
        for p in model.parameters():
            p.grad = None
    torch.cuda.synchronize()
    return model, opt, losses, maes


@pytest.mark.parametrize("prefetch", [1, 0])
def test_trainer_with_l1_and_weights_logs_the_weighted_loss_and_keeps_the_plain_mae(sd0, tmp_path, prefetch):
    from resdepth_amd import masked_loss
    tr = _trainer(tmp_path, sd0, nn.L1Loss(reduction="mean"), prefetch_batches=prefetch)
    tr.loader = {"train": _WithWeights(tr.loader["train"], 100), "val": _WithWeights(tr.loader["val"], 200)}
    assert tr._loss_module is None                       # built when the first weight arrives
    meters = tr.inference_one_epoch(0, "val")
    assert set(meters) == {"MAE_metric"} and tr._loss_module is not None and tr._loss_module.kind == "l1"
    meters = tr.inference_one_epoch(0, "train")
    assert set(meters) == {"MAE_metric", "loss"} and meters["loss"].count == meters["MAE_metric"].count == 3
    model, opt, losses, maes = _hand_epoch(sd0, _WithWeights(_loaders()[0], 100),
                                           lambda yp, y, m, mean, std, w: masked_loss(yp, y, m, mean, std, kind="l1", weight=w))
    _same_state(tr.model, tr.optimizer, model, opt)
    s = 0.0
    for v in losses:
        s += v
    assert meters["loss"].avg == s / len(losses)
    want = sum(maes) / len(maes)
    assert abs(meters["MAE_metric"].avg - want) <= 1e-6 * want
    assert abs(meters["loss"].avg - want) > 1e-3 * want               # the optimised value is not the MAE


def test_trainer_sees_the_weights_of_its_first_batch(sd0, tmp_path):
    from resdepth_amd import FusedAdam, Trainer, UNet
    from test_loss_gpu import _args
    model = UNet(**TKW)
    model.load_state_dict(sd0)
    train, val = _loaders()
    tr = Trainer(_args(tmp_path, model, FusedAdam(model.parameters(), lr=1e-3), _WithWeights(train, 100), val, nn.L1Loss()))
    assert tr._loss_module is not None and set(tr.stats_meter("train")) == {"MAE_metric", "loss"}
    assert set(tr.inference_one_batch(next(iter(tr.loader["train"])), "train")) == {"MAE_metric", "loss"}
    assert set(tr.inference_one_batch(next(iter(tr.loader["val"])), "val")) == {"MAE_metric"}


def test_trainer_without_weights_leaves_the_bits_of_a_loop_over_masked_l1_loss(sd0, tmp_path):
    from resdepth_amd import masked_l1_loss
    tr = _trainer(tmp_path, sd0, nn.L1Loss(reduction="mean"))
    meters = tr.inference_one_epoch(0, "train")
    assert set(meters) == {"MAE_metric"} and tr._loss_module is None
    model, opt, losses, _ = _hand_epoch(sd0, _loaders()[0], lambda yp, y, m, mean, std, w: masked_l1_loss(yp, y, m, mean, std))
    _same_state(tr.model, tr.optimizer, model, opt)
    s = 0.0
    for v in losses:
        s += v
    assert meters["MAE_metric"].avg == s / len(losses)


def test_trainer_passes_the_weights_to_the_planned_step(sd0, tmp_path):
    res = []
    for planned in (False, True):
        tr = _trainer(tmp_path / ("p" if planned else "e"), sd0, nn.L1Loss(), n_train=30, launch_plan=planned)
        tr.loader["train"] = _WithWeights(tr.loader["train"], 300)
        tr._weighted_module()
        res.append((tr, tr.inference_one_epoch(0, "train")))
    (te, me), (tp, mp) = res
    assert tp._graphed is not None and tp._graphed.plan_rejected is None and tp._graphed.replays >= 3
    for k in ("MAE_metric", "loss"):
        assert me[k].avg == mp[k].avg and me[k].count == mp[k].count == 8
    assert me["loss"].avg != me["MAE_metric"].avg
    _same_state(te.model, te.optimizer, tp.model, tp.optimizer)


# ---- captured graph and launch plan ---------------------------------------------------------------------------------------------
def _eight_steps(make_step, loss):
    """tests/test_loss_gpu.py::_eight_steps with a weight: eight steps, one ragged batch, one batch WITHOUT a weight (eager: the
    capture holds a weight buffer), one non-contiguous and one fp64 weight (eager: torch would convert them)."""
    from resdepth_amd import UNet
    torch.manual_seed(0)
    sd = copy.deepcopy(UNet(**KW).state_dict())
    full, ragged = _batches(4, 4), _batches(3, 1, seed=40)
    seq = [full[k % 4] for k in range(10)]
    seq[5] = ragged[0]
    ws = [_weights(tuple(b[1].shape), b[2].cpu(), "uniform", seed=k).to(DEV) for k, b in enumerate(seq)]
    ws[7] = None
    wide = torch.zeros(4, 1, 64, 128, device=DEV)
    wide[..., ::2] = ws[8]
    ws[8] = wide[..., ::2]
    ws[9] = ws[9].double()
    assert not ws[8].is_contiguous()
    res = []
    for replayed in (False, True):
        model, opt = _fresh(sd)
        step = make_step(model, opt, warmup=2 if replayed else 1 << 60, loss=loss)
        losses, maes, how = [], [], []
        for k, (b, w) in enumerate(zip(seq, ws)):
            if k == 4:
                opt.param_groups[0]["lr"] *= 0.5
            losses.append(step(*b, weight=w).clone())
            if w is not None or loss is not None:
                maes.append(step.mae.clone())
            how.append(step.why_eager)
            assert all(p.grad is None for p in model.parameters())
        torch.cuda.synchronize()
        res.append((model, opt, torch.stack(losses).cpu(), torch.stack(maes).cpu(), how, step))
    (me, oe, le, ae, _, _), (mg, og, lg, ag, how, step) = res
    assert how[:3] == ["warm-up", "warm-up", "capture preparation"] and how[3] is None and how[4] is None
    assert how[5] == "batch shape differs from the captured one" and how[6] is None and step.replays == 3
    assert "loss weight" in how[7] and "contiguous" in how[8] and "float32" in how[9], how
    assert torch.equal(le, lg), (le, lg)
    assert torch.equal(ae, ag), (ae, ag)
    _same_state(me, oe, mg, og)
    return step


def test_planned_iterations_with_a_weight_leave_the_bits_of_eager_ones():
    from resdepth_amd import MaskedLoss
    from resdepth_amd.plan import PlannedTrainStep
    step = _eight_steps(PlannedTrainStep, MaskedLoss("huber", 0.5, 0.3))
    assert step.plan_rejected is None, step.plan_rejected
    assert step.n_launches > 40 and step.n_segments == 1


def test_graphed_iterations_with_a_weight_leave_the_bits_of_eager_ones():
    from resdepth_amd import GraphedTrainStep
    _eight_steps(GraphedTrainStep, None)                 # plain L1 with a weight: the weighted L1 kernels, the MAE beside it
