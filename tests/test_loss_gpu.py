"""resdepth_amd.masked_loss on the GPU (-m gpu) against the oracle of tests/loss_ref.py: L2 / Huber / smooth-L1 / L1 data terms
with and without the slope-consistency term, on shapes that take the scalar and the vector path, more than one tile in each
direction and more than one pass of the grid; then the properties around it -- reproducibility, delegation to the L1 kernels,
the upstream gradient, the global normaliser -- and the Trainer, GraphedTrainStep and PlannedTrainStep with such a loss.

Bars (derived, not measured): r is bit-identical in kernel and oracle, the sums are fp64, every loss term is non-negative
and each fp32 result is one rounding of an fp64 value: 1e-6 relative leaves room for a handful of 2^-24 roundings."""
import copy
import os
import types

import pytest
import torch
from torch import nn
from torch.utils.data import DataLoader

import loss_ref
from test_graph_gpu import KW, _batches, _fresh, _same_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

GRID_PASS = (1100, 1, 2, 3)          # one tile per sample: more tiles than the grid has blocks
SHAPES = [(3, 1, 5, 7), (2, 1, 1, 9), (2, 1, 9, 1), (1, 1, 1, 1), (2, 1, 8, 16), (2, 1, 70, 12), (1, 1, 6, 300), (3, 1, 64, 64),
          GRID_PASS]
MASKS = ["ones", "bernoulli", "checkerboard", "sample_masked", "single_pixel", "bernoulli_u8"]
SPECS = [("l2", 1.0), ("huber", 0.5), ("smooth_l1", 2.0), ("l1", 1.0)]
LAMBDAS = [0.0, 0.3]


def _data(shape, mask_kind, seed=0):
    """std in [0.5, 8], mean in [-50, 400], residuals of a few metres (host tensors)."""
    g = torch.Generator().manual_seed(1000 * seed + sum(shape) + 7 * len(mask_kind))
    n, _, h, w = shape
    y = torch.randn(shape, generator=g)
    std = torch.rand(n, generator=g) * 7.5 + 0.5
    mean = torch.rand(n, generator=g) * 450.0 - 50.0
    yp = y + torch.randn(shape, generator=g) * (2.0 / std).reshape(n, 1, 1, 1)
    if mask_kind == "ones":
        m = torch.ones(shape, dtype=torch.bool)
    elif mask_kind in ("bernoulli", "bernoulli_u8"):
        m = torch.rand(shape, generator=g) < 0.7
        m[0, 0, 0, 0] = True
        if mask_kind == "bernoulli_u8":              # any non-zero byte is "valid"
            m = m.to(torch.uint8) * torch.randint(1, 256, shape, generator=g).to(torch.uint8)
    elif mask_kind == "checkerboard":
        ii, jj = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        m = (((ii + jj) % 2) == 0).expand(shape).clone()
    elif mask_kind == "sample_masked":
        m = torch.rand(shape, generator=g) < 0.7
        m[0, 0, 0, 0] = True
        m[n - 1] = False
    elif mask_kind == "single_pixel":
        m = torch.zeros(shape, dtype=torch.bool)
        m[n - 1, 0, h // 2, w - 1] = True
    return yp, y, m, mean, std


def _run(yp, y, m, mean, std, kind, delta, lam, gout=None, **kw):
    """-> loss, mae (python floats), gradient (host, fp32)"""
    from resdepth_amd import masked_loss
    x = yp.to(DEV).requires_grad_()
    loss, mae = masked_loss(x, y.to(DEV), m.to(DEV), mean, std, kind=kind, delta=delta, slope_weight=lam, return_mae=True, **kw)
    assert loss.shape == () and mae.shape == () and not mae.requires_grad
    (loss if gout is None else gout * loss).backward()
    return float(loss.detach()), float(mae), x.grad.cpu()


def _judge(got, o, mask):
    loss, mae, grad = got
    assert abs(loss - o["loss"]) <= 1e-6 * o["loss"], (loss, o["loss"])
    assert abs(mae - o["mae"]) <= 1e-6 * o["mae"], (mae, o["mae"])
    want = o["g_data"] + o["g_slope"]
    bar = 1e-6 * (o["g_data"].abs() + o["g_slope"].abs())
    err = (grad.double() - want).abs()
    assert bool((err <= bar).all()), (float((err - bar).max()), int((err > bar).sum()))
    assert int((grad[mask.reshape(grad.shape) == 0] != 0).sum()) == 0          # exactly 0 at masked pixels


def _params():
    out = []
    for shape in SHAPES:
        for mk in MASKS:
            if mk == "sample_masked" and shape[0] == 1:
                continue                                  # needs a second sample to keep C > 0
            out.append(pytest.param(shape, mk, id="x".join(map(str, shape)) + "-" + mk))
    return out


def test_the_shapes_cross_the_strip_and_the_grid():
    from resdepth_amd import _lib
    assert 70 > _lib.LOSS_STRIP_ROWS and 300 > _lib.LOSS_STRIP_COLS
    assert 5 < _lib.LOSS_STRIP_ROWS and 7 < _lib.LOSS_STRIP_COLS and 64 % _lib.LOSS_STRIP_ROWS == 0
    assert GRID_PASS[0] > _lib.LOSS_MAX_BLOCKS              # one tile per sample of GRID_PASS
    assert GRID_PASS[2] <= _lib.LOSS_STRIP_ROWS and GRID_PASS[3] <= _lib.LOSS_STRIP_COLS


@pytest.mark.parametrize("shape,mask_kind", _params())
def test_loss_mae_and_gradient_against_the_oracle(shape, mask_kind):
    yp, y, m, mean, std = _data(shape, mask_kind)
    for kind, delta in SPECS:
        for lam in LAMBDAS:
            o = loss_ref.masked_loss_oracle(yp, y, m, mean, std, kind, delta, lam)
            got = _run(yp, y, m, mean, std, kind, delta, lam)
            _judge(got, o, m)
            if mask_kind in ("checkerboard", "single_pixel") or shape[2] * shape[3] == 1:
                assert o["Q"] == 0 and o["C"] > 0 and float(o["g_slope"].abs().max()) == 0.0
                assert got[0] == _run(yp, y, m, mean, std, kind, delta, 0.0)[0] and got[0] == got[0]   # finite, no slope term


@pytest.mark.parametrize("shape", [(3, 1, 5, 7), (2, 1, 8, 16), (1, 1, 40, 72)], ids=lambda s: "x".join(map(str, s)))
def test_a_block_of_zero_residual_gets_no_data_gradient_and_flat_neighbours_add_nothing(shape):
    yp, y, m, mean, std = _data(shape, "ones", seed=2)
    n, _, h, w = shape
    hb, wb = h // 2 + 1, w // 2 + 1
    yp[:, :, :hb, :wb] = y[:, :, :hb, :wb]
    for kind, delta in SPECS:
        o = loss_ref.masked_loss_oracle(yp, y, m, mean, std, kind, delta, 0.3)
        assert float(o["r"][:, :, :hb, :wb].abs().max()) == 0.0 and int(o["k"][:, :, :hb - 1, :wb - 1].abs().max()) == 0
        got = _run(yp, y, m, mean, std, kind, delta, 0.3)
        _judge(got, o, m)
        assert float(got[2][:, :, :hb - 1, :wb - 1].abs().max()) == 0.0
        assert float(got[2][:, :, hb - 1, :wb - 1].abs().max()) > 0.0       # the block's last row sees the residuals below it


def test_non_contiguous_offsets_take_the_scalar_path_with_the_same_result():
    """A batch whose storage starts 4 bytes into an allocation (16-byte alignment lost, W % 4 == 0): the one-element path,
    bit for bit what the vector path gives."""
    from resdepth_amd import masked_loss
    shape = (2, 1, 8, 16)
    yp, y, m, mean, std = _data(shape, "bernoulli")
    numel = yp.numel()
    res = []
    for off in (0, 1):
        buf = torch.zeros(numel + 4, device=DEV)
        buf[off:off + numel] = yp.reshape(-1).to(DEV)
        x = buf[off:off + numel].view(shape).detach().requires_grad_()
        assert x.is_contiguous() and (x.data_ptr() % 16 == 0) == (off == 0)
        loss, mae = masked_loss(x, y.to(DEV), m.to(DEV), mean, std, kind="huber", delta=0.5, slope_weight=0.3, return_mae=True)
        loss.backward()
        res.append((loss.detach().clone(), mae.clone(), x.grad.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_two_calls_give_the_same_bits():
    from resdepth_amd import masked_loss
    yp, y, m, mean, std = _data((3, 1, 64, 64), "bernoulli")
    res = []
    for _ in range(2):
        x = yp.to(DEV).requires_grad_()
        loss, mae = masked_loss(x, y.to(DEV), m.to(DEV), mean, std, kind="huber", delta=0.5, slope_weight=0.3, return_mae=True)
        loss.backward()
        res.append((loss.detach().clone(), mae.clone(), x.grad.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_l1_without_a_slope_term_is_masked_l1_loss_bit_for_bit():
    from resdepth_amd import masked_l1_loss, masked_loss, MaskedLoss
    yp, y, m, mean, std = _data((3, 1, 5, 7), "bernoulli")
    res = []
    for fn in (lambda x: masked_l1_loss(x, y.to(DEV), m.to(DEV), mean, std),
               lambda x: masked_loss(x, y.to(DEV), m.to(DEV), mean, std, kind="l1", slope_weight=0.0),
               lambda x: MaskedLoss("smooth_l1", delta=0.0)(x, y.to(DEV), m.to(DEV), mean, std)):
        x = yp.to(DEV).requires_grad_()
        loss = fn(x)
        loss.backward()
        res.append((loss.detach().clone(), x.grad.clone()))
    for other in res[1:]:
        assert torch.equal(res[0][0], other[0]) and torch.equal(res[0][1], other[1])
    loss, mae = masked_loss(yp.to(DEV), y.to(DEV), m.to(DEV), mean, std, return_mae=True)
    assert torch.equal(loss, mae) and torch.equal(loss, res[0][0])


def test_the_upstream_gradient_is_read_from_the_device():
    yp, y, m, mean, std = _data((2, 1, 8, 16), "bernoulli")
    o = loss_ref.masked_loss_oracle(yp, y, m, mean, std, "huber", 0.5, 0.3, gout=2.5)
    got = _run(yp, y, m, mean, std, "huber", 0.5, 0.3, gout=torch.tensor(2.5, device=DEV))
    _judge(got, o, m)
    plain = _run(yp, y, m, mean, std, "huber", 0.5, 0.3)
    assert float(got[2].abs().max()) > 2.0 * float(plain[2].abs().max())


class _OtherHalf:
    """duck-typed grad_sync: the all-reduce over two ranks, the other rank's sums given"""

    def __init__(self, other_sums):
        self.other, self.seen = other_sums, None

    def allreduce_loss_sums(self, sums, numel):
        sums.add_(self.other)
        self.seen = sums.clone()
        return 2 * numel


@pytest.mark.parametrize("kind,delta,lam", [("l2", 1.0, 0.3), ("huber", 0.5, 0.0), ("l1", 1.0, 0.3)])
def test_the_normalisers_are_global_under_data_parallelism(kind, delta, lam):
    from resdepth_amd import masked_loss, ops
    from resdepth_amd.loss import _check_spec, _kernel_args, _prep
    yp, y, m, mean, std = _data((4, 1, 9, 12), "bernoulli")
    code, d, scale = _kernel_args(*_check_spec(kind, delta, lam)[:2])
    halves = [slice(0, 2), slice(2, 4)]
    part = [ops.masked_loss_partial(*_prep(yp[h].to(DEV), y[h], m[h], mean[h], std[h]), code, d, scale) for h in halves]
    whole = ops.masked_loss_partial(*_prep(yp.to(DEV), y, m, mean, std), code, d, scale)
    grads, losses = [], []
    for i, h in enumerate(halves):
        sync = _OtherHalf(part[1 - i])
        x = yp[h].to(DEV).requires_grad_()
        loss = masked_loss(x, y[h].to(DEV), m[h].to(DEV), mean[h], std[h], kind=kind, delta=delta, slope_weight=lam, grad_sync=sync)
        loss.backward()
        grads.append(x.grad)
        losses.append(float(loss))
        assert float(sync.seen[1]) == float(whole[1]) and float(sync.seen[4]) == float(whole[4])       # C and Q, exactly
        assert torch.equal(sync.seen[5:], torch.zeros(3, dtype=torch.float64, device=DEV))
    x = yp.to(DEV).requires_grad_()
    lw = masked_loss(x, y.to(DEV), m.to(DEV), mean, std, kind=kind, delta=delta, slope_weight=lam)
    lw.backward()
    got, want = torch.cat(grads).double(), x.grad.double()
    assert bool(((got - want).abs() <= 2.0 ** -22 * want.abs()).all())
    assert abs(losses[0] - float(lw)) <= 1e-6 * float(lw) and abs(losses[1] - float(lw)) <= 1e-6 * float(lw)


# ---- Trainer ----------------------------------------------------------------------------------------------------------------
TKW = dict(n_input_channels=2, start_kernel=8, depth=2, bias_conv_layer=True)


def _args(tmp, model, opt, train, val, criterion, **extra):
    return types.SimpleNamespace(
        model=model, optimizer=opt, scheduler=None, criterion=criterion, trainloader=train, valloader=val, n_epochs=1,
        evaluate_rate=1, save_model_rate=1, freq_average_train_loss=1000, save_dir=str(tmp),
        log_file=os.path.join(str(tmp), "training.log"), checkpoint_dir=os.path.join(str(tmp), "checkpoints"),
        tboard_log_dir=os.path.join(str(tmp), "tb"), pretrained_path=None, **extra)


def _loaders(n_train=12):
    from resdepth_amd import SyntheticDsmOrthoDataset
    return (DataLoader(SyntheticDsmOrthoDataset(n_train, 2, 32, seed=3), batch_size=4, shuffle=False),
            DataLoader(SyntheticDsmOrthoDataset(6, 2, 32, seed=4), batch_size=4, shuffle=False))


def _trainer(tmp, sd0, criterion, n_train=12, **extra):
    from resdepth_amd import UNet, FusedAdam, Trainer
    model = UNet(**TKW)
    model.load_state_dict(sd0)
    opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=1e-5)
    train, val = _loaders(n_train)
    return Trainer(_args(tmp, model, opt, train, val, criterion, **extra))


def _inline_epoch(sd0, loss_fn, oracle_spec=None):
    """The Trainer's train epoch as a plain loop -> (model, optimizer, oracle MAEs of the batches as they were predicted)"""
    from resdepth_amd import UNet, FusedAdam
    model = UNet(**TKW)
    model.load_state_dict(sd0)
    model = model.to(DEV).train()
    opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=1e-5)
    maes, losses = [], []
    for batch in _loaders()[0]:
        x, y, m = batch["input"].to(DEV), batch["target"].to(DEV), batch["loss_mask"].to(DEV)
        mean, std = torch.flatten(batch["dsm_mean"]), torch.flatten(batch["dsm_std"])
        y_pred = model(x)
        if oracle_spec is not None:
            o = loss_ref.masked_loss_oracle(y_pred, y, m, mean, std, *oracle_spec)
            maes.append(o["mae"])
            losses.append(o["loss"])
        loss = loss_fn(y_pred, y, m, mean, std)
        loss.backward()
        opt.step()
        for p in model.parameters():
            p.grad = None
    torch.cuda.synchronize()
    return model, opt, maes, losses


@pytest.fixture(scope="module")
def sd0():
    from resdepth_amd import UNet
    torch.manual_seed(0)
    return copy.deepcopy(UNet(**TKW).state_dict())


@pytest.fixture(scope="module")
def l1_run(sd0, tmp_path_factory):
    tr = _trainer(tmp_path_factory.mktemp("l1"), sd0, nn.L1Loss(reduction="mean"))
    meters = tr.inference_one_epoch(0, "train")
    return tr, meters


def test_trainer_with_l1_leaves_the_bits_of_a_loop_over_masked_l1_loss(sd0, l1_run):
    from resdepth_amd import masked_l1_loss
    tr, meters = l1_run
    assert set(meters) == {"MAE_metric"} and meters["MAE_metric"].count == 3
    model, opt, _, _ = _inline_epoch(sd0, lambda *a: masked_l1_loss(*a))
    _same_state(tr.model, tr.optimizer, model, opt)


@pytest.mark.parametrize("name", ["huber", "l2_slope"])
def test_trainer_optimises_the_criterion_and_keeps_the_mae_as_its_metric(sd0, l1_run, tmp_path, name):
    from resdepth_amd import MaskedLoss, masked_loss
    criterion, spec = {"huber": (nn.HuberLoss(delta=1.0), ("huber", 1.0, 0.0)),
                       "l2_slope": (MaskedLoss("l2", slope_weight=0.3), ("l2", 1.0, 0.3))}[name]
    tr = _trainer(tmp_path, sd0, criterion)
    meters = tr.inference_one_epoch(0, "train")
    assert set(meters) == {"MAE_metric", "loss"} and meters["loss"].count == meters["MAE_metric"].count == 3
    model, opt, maes, losses = _inline_epoch(
        sd0, lambda *a: masked_loss(*a, kind=spec[0], delta=spec[1], slope_weight=spec[2]), oracle_spec=spec)
    _same_state(tr.model, tr.optimizer, model, opt)
    want = sum(maes) / len(maes)
    got = meters["MAE_metric"].avg
    print(f"{name}: MAE_metric {got!r} oracle {want!r}; loss {meters['loss'].avg!r} oracle {sum(losses) / len(losses)!r}")
    assert abs(got - want) <= 1e-5 and abs(got - want) <= 1e-5 * want
    assert abs(meters["loss"].avg - sum(losses) / len(losses)) <= 1e-5 * (sum(losses) / len(losses))
    assert abs(meters["loss"].avg - got) > 1e-3 * got                # the optimised value is not the MAE
    tl1 = l1_run[0]
    assert any(not torch.equal(v, tl1.model.state_dict()[k]) for k, v in tr.model.state_dict().items()
               if v.dtype.is_floating_point)
    # validation: the same function under no_grad, the MAE alone
    val = tr.inference_one_epoch(0, "val")
    assert set(val) == {"MAE_metric"} and val["MAE_metric"].count == 2
    tr.model.eval()
    want_val = []
    with torch.no_grad():
        for batch in tr.loader["val"]:
            x, y, m = batch["input"].to(DEV), batch["target"].to(DEV), batch["loss_mask"].to(DEV)
            o = loss_ref.masked_loss_oracle(tr.model(x), y, m, torch.flatten(batch["dsm_mean"]), torch.flatten(batch["dsm_std"]), *spec)
            want_val.append(o["mae"])
    wv = sum(want_val) / len(want_val)
    assert abs(val["MAE_metric"].avg - wv) <= 1e-5 * min(1.0, wv)
    one = tr.inference_one_batch(next(iter(tr.loader["val"])), "val")
    assert set(one) == {"MAE_metric"}
    one = tr.inference_one_batch(next(iter(tr.loader["train"])), "train")
    assert set(one) == {"MAE_metric", "loss"}


def test_trainer_refuses_a_criterion_without_a_fused_form(sd0, tmp_path):
    with pytest.raises(NotImplementedError, match="nn.HuberLoss"):
        _trainer(tmp_path, sd0, nn.MSELoss(reduction="sum"))
    with pytest.raises(NotImplementedError, match="MaskedLoss"):
        _trainer(tmp_path, sd0, nn.BCELoss())


def test_trainer_passes_its_criterion_to_the_planned_step(sd0, tmp_path):
    from resdepth_amd import MaskedLoss
    res = []
    for planned in (False, True):
        tr = _trainer(tmp_path / ("p" if planned else "e"), sd0, MaskedLoss("l2", slope_weight=0.3), n_train=30, launch_plan=planned)
        meters = tr.inference_one_epoch(0, "train")
        res.append((tr, meters))
    (te, me), (tp, mp) = res
    assert tp._graphed is not None and tp._graphed.plan_rejected is None and tp._graphed.replays >= 3
    assert tp._graphed.loss is tp._loss_module
    for k in ("MAE_metric", "loss"):
        assert me[k].avg == mp[k].avg and me[k].count == mp[k].count == 8
    _same_state(te.model, te.optimizer, tp.model, tp.optimizer)


# ---- captured graph and launch plan -----------------------------------------------------------------------------------------
def _eight_steps(make_step):
    """tests/test_plan_gpu.py::test_planned_iterations_leave_the_bits_of_eager_ones, eight steps, one ragged batch"""
    from resdepth_amd import MaskedLoss, UNet
    torch.manual_seed(0)
    sd = copy.deepcopy(UNet(**KW).state_dict())
    full, ragged = _batches(4, 4), _batches(3, 1, seed=40)
    seq = [full[k % 4] for k in range(8)]
    seq[5] = ragged[0]
    res = []
    for replayed in (False, True):
        model, opt = _fresh(sd)
        step = make_step(model, opt, warmup=2 if replayed else 1 << 60, loss=MaskedLoss("huber", 0.5, 0.3))
        losses, maes, how = [], [], []
        for k, b in enumerate(seq):
            if k == 4:
                opt.param_groups[0]["lr"] *= 0.5
            losses.append(step(*b).clone())
            maes.append(step.mae.clone())
            how.append(step.why_eager)
            assert all(p.grad is None for p in model.parameters())
        torch.cuda.synchronize()
        res.append((model, opt, torch.stack(losses).cpu(), torch.stack(maes).cpu(), how, step))
    (me, oe, le, ae, _, _), (mg, og, lg, ag, how, step) = res
    assert how[:3] == ["warm-up", "warm-up", "capture preparation"] and how[3] is None and how[4] is None
    assert how[5] == "batch shape differs from the captured one" and how[6] is None and how[7] is None and step.replays == 4
    assert torch.equal(le, lg), (le, lg)
    assert torch.equal(ae, ag), (ae, ag)
    assert bool((le != ae).all())                     # two different quantities
    _same_state(me, oe, mg, og)
    return step


def test_planned_iterations_with_a_masked_loss_leave_the_bits_of_eager_ones():
    from resdepth_amd.plan import PlannedTrainStep
    step = _eight_steps(PlannedTrainStep)
    assert step.plan_rejected is None, step.plan_rejected
    assert step.n_launches > 40 and step.n_segments == 1


def test_graphed_iterations_with_a_masked_loss_leave_the_bits_of_eager_ones():
    from resdepth_amd import GraphedTrainStep
    _eight_steps(GraphedTrainStep)
