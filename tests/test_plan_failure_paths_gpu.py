"""The failure paths of the recorded launch plan and of the captured HIP graph (-m gpu): what happens when a plan cannot be used
or has to be dropped (resdepth_amd/plan.py, resdepth_amd/graph.py).

  * the first replay's bit-for-bit verification rejects the plan (one flipped bit in a parameter, a BatchNorm buffer, either
    Adam moment or the loss): the call is the eager iteration, and so is every later one;
  * a recording that cannot become a plan (poisoned by the library, an exception inside the capture);
  * keep_grads=True on both step classes;
  * batches the loss has to convert (mask / target / mean / std of another dtype, non-contiguous tensors);
  * a larger eager batch between replays (the shared weight-gradient stream's scratch buffers are replaced under the plan);
  * one rank of two rejects;
  * optimizer.load_state_dict between replays.

The reference of every case is the eager iteration -- the same step class with warmup=1 << 60 -- from the same state_dict over the
same batches: the plan's specification is "leave exactly the bits the eager iteration leaves", so every comparison is
torch.equal and no tolerance appears anywhere.  Every forced failure is a host-side perturbation."""
import copy
import functools
import os
import sys
import types
import weakref

import pytest
import torch
from torch.utils.data import DataLoader, Dataset

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_graph_gpu import _args, _batches, _fresh, _same_state, KW, DEV  # noqa: E402

pytestmark = pytest.mark.gpu
NEVER = 1 << 60
REJECTED = "the first replay did not reproduce the eager iteration bit for bit"


@functools.lru_cache(maxsize=None)
def _sd0():
    from resdepth_amd import UNet
    torch.manual_seed(0)
    return copy.deepcopy(UNet(**KW).state_dict())


def _classes():
    from resdepth_amd import GraphedTrainStep
    from resdepth_amd.plan import PlannedTrainStep
    return {"graph": GraphedTrainStep, "plan": PlannedTrainStep}


def _run(cls, seq, warmup, keep_grads=False, hook=None, between=None, **kw):
    """One training run from _sd0() over `seq`; the loss, why_eager and -- keep_grads -- a copy of every gradient after each
    call.  `hook(step)` instruments the step before the first call, `between(k, step, model, opt)` runs before call k."""
    model, opt = _fresh(_sd0())
    step = _classes()[cls](model, opt, warmup=warmup, keep_grads=keep_grads, **kw)
    captures = []
    real_capture = step._capture
    step._capture = lambda batch: (captures.append(step._calls), real_capture(batch))[1]
    step.test_captures = captures            # the call numbers at which a recording was ATTEMPTED
    if hook is not None:
        hook(step)
    losses, how, grads = [], [], []
    for k, b in enumerate(seq):
        if between is not None:
            between(k, step, model, opt)
        out = step(*b)
        assert isinstance(out, torch.Tensor) and out.is_cuda and out.dim() == 0, (k, out)
        losses.append(out.clone())
        how.append(step.why_eager)
        if keep_grads:
            assert all(p.grad is not None for p in step.params), k
            grads.append([p.grad.clone() for p in step.params])
        else:
            assert all(p.grad is None for p in step.params), k               # lib/Trainer.py:221-222
    torch.cuda.synchronize()
    return types.SimpleNamespace(model=model, opt=opt, step=step, losses=torch.stack(losses).cpu(), how=how, grads=grads,
                                 captures=captures, opt_step=float(opt.state_dict()["state"][0]["step"]))


def _same_run(e, r):
    assert torch.equal(e.losses, r.losses), (e.losses, r.losses)
    _same_state(e.model, e.opt, r.model, r.opt)
    assert e.opt_step == r.opt_step == float(len(e.how)), (e.opt_step, r.opt_step)


def _same_grads(e, r):
    assert len(e.grads) == len(r.grads) == len(e.how)
    for k, (ge, gr) in enumerate(zip(e.grads, r.grads)):
        for i, (a, b) in enumerate(zip(ge, gr)):
            assert torch.equal(a, b), (k, i, r.how[k])


# ---- the batch sequences and their eager runs: computed once, shared, left unchanged ---------------------------------------
@functools.lru_cache(maxsize=None)
def _seq(name):
    if name == "full8":
        full = _batches(4, 4)
        return [full[k % 4] for k in range(8)]
    if name == "ragged12":
        full, ragged = _batches(4, 4), _batches(3, 1, seed=40)
        seq = [full[k % 4] for k in range(12)]
        seq[7] = ragged[0]
        return seq
    if name == "larger10":
        small, large = _batches(2, 3), _batches(6, 1, seed=60)
        seq = [small[k % 3] for k in range(10)]
        seq[5] = large[0]
        return seq
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _eager(name, cls="plan"):
    """The all-eager run over _seq(name), with every call's gradients (keep_grads changes what a call leaves, not what it
    computes: _eager starts from 'no gradient' either way)."""
    return _run(cls, _seq(name), NEVER, keep_grads=True)


# ---- 1. rejection at the first replay ----------------------------------------------------------------------------------------
def _flip(t):
    """XOR the low mantissa bit of the largest element of a float32 tensor (never a zero: the change is one ulp of a normal)."""
    flat = t.view(-1) if t.dim() else t.view(1)
    i = int(flat.abs().argmax())
    flat[i:i + 1].view(torch.int32).bitwise_xor_(1)


def _target(step, what):
    m, o = step.model, step.optimizer
    if what == "param":
        return m._flat_param
    if what == "bn_buffer":
        return next(b for k, b in m.named_buffers() if k.endswith("running_var"))
    if what == "exp_avg":
        return o._flat_state[0][1]
    if what == "exp_avg_sq":
        return o._flat_state[0][2]
    if what == "loss":
        return step._loss
    raise KeyError(what)


def _perturb_first_plan_run(what):
    def hook(step):
        real, n = step._run_plan, [0]

        def run():
            real()
            n[0] += 1
            if n[0] == 1:
                _flip(_target(step, what))
        step._run_plan = run
        step.plan_runs = n
    return hook


@pytest.mark.parametrize("keep_grads", [False, True])
@pytest.mark.parametrize("what", ["param", "bn_buffer", "exp_avg", "exp_avg_sq", "loss"])
def test_a_plan_rejected_at_its_first_replay_hands_the_call_to_the_eager_iteration(what, keep_grads):
    """The first run of the plan leaves one wrong bit in `what`: the verification must see it (this pins what _snapshot covers),
    the call must return the eager iteration's loss and leave its gradients as keep_grads asks, and the run goes on eagerly.
    Before the fix: TypeError from zip(self.params, None) with keep_grads, a None loss without."""
    e = _eager("full8")
    r = _run("plan", _seq("full8"), 1, keep_grads=keep_grads, hook=_perturb_first_plan_run(what))
    s = r.step
    assert r.how[:2] == ["warm-up", "capture preparation"]
    assert s.plan_rejected == REJECTED and r.how[2] == REJECTED
    assert all(h is not None for h in r.how[2:]), r.how                      # that call and every later one ran eagerly
    assert s.replays == 0                                                    # the rejected call is not a replay
    assert r.captures == [3] and s.recordings == 1 and s.plan_runs == [1]    # and no second recording is attempted
    _same_run(e, r)                                                          # opt_step == 8: the rejected step counted once
    if keep_grads:
        _same_grads(e, r)


# ---- 2. a recording that cannot become a plan --------------------------------------------------------------------------------
def _poison(step):
    from resdepth_amd import _lib
    real = step._record_begin

    def begin():
        real()
        _lib.load().rd_plan_poison(b"forced by the test")
    step._record_begin = begin


def _capture_step_raises_once(step):
    opt, n = step.optimizer, [0]
    real = opt.capture_step

    def capture_step():
        n[0] += 1
        if n[0] == 1:
            raise RuntimeError("forced by the test")
        return real()
    opt.capture_step = capture_step


@pytest.mark.parametrize("how", ["poisoned", "raises"])
def test_a_recording_that_cannot_become_a_plan_leaves_the_call_to_the_eager_iteration(how):
    """The recording's forward ran the weight-packing bookkeeping without a pack kernel executing: the eager iteration that takes
    the call must pack again, or it trains on weights one optimizer step old."""
    e = _eager("ragged12")
    r = _run("plan", _seq("ragged12"), 1, hook=_poison if how == "poisoned" else _capture_step_raises_once)
    s = r.step
    assert r.how[:2] == ["warm-up", "capture preparation"]
    assert r.how[2].startswith("plan unavailable"), r.how[2]
    assert ("forced by the test" if how == "poisoned" else "RuntimeError") in r.how[2], r.how[2]
    assert r.captures == [3] and s.replays == 0 and s.recordings == 0        # tried once, never again
    assert all(h is not None for h in r.how), r.how
    if how == "raises":                                                      # torch is not left in capture mode
        assert not torch.cuda.is_current_stream_capturing()
        t = torch.arange(8, device=DEV, dtype=torch.float32) * 2
        torch.cuda.synchronize()
        assert t.tolist() == [0.0, 2.0, 4.0, 6.0, 8.0, 10.0, 12.0, 14.0]
    _same_run(e, r)                                                          # 9 further steps after the failed recording


# ---- 3. keep_grads=True ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["graph", "plan"])
def test_keep_grads_leaves_each_iterations_own_gradients(cls):
    """Warm-up, capture preparation, replays, one ragged batch (eager), replays again: after EVERY call p.grad holds that
    iteration's gradients -- the eager run's, bit for bit -- never a sum with what the previous call left."""
    e = _eager("ragged12", cls)
    r = _run(cls, _seq("ragged12"), 2, keep_grads=True)
    assert r.how[:3] == ["warm-up", "warm-up", "capture preparation"] and r.how[3] is None
    assert r.how[7] == "batch shape differs from the captured one" and r.how[8] is None and r.step.replays == 8
    assert getattr(r.step, "plan_rejected", None) is None
    _same_grads(e, r)
    _same_run(e, r)


# ---- 4. batches the loss has to convert --------------------------------------------------------------------------------------
FORMS = ["bool_mask", "uint8_mask", "float32_mask", "int64_mask", "float64_target", "float64_mean_std", "noncontiguous_input",
         "noncontiguous_target"]


def _as_form(b, form):
    x, y, mask, mean, std = b
    if form == "bool_mask":
        mask = mask != 0
    elif form == "uint8_mask":
        mask = (mask != 0).to(torch.uint8)
    elif form == "float32_mask":
        mask = (mask != 0).to(torch.float32)
    elif form == "int64_mask":
        mask = (mask != 0).to(torch.int64)
    elif form == "float64_target":
        y = y.double()
    elif form == "float64_mean_std":
        mean, std = mean.double(), std.double()
    elif form == "noncontiguous_input":
        x = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)           # same values, channels-last strides
        assert not x.is_contiguous()
    elif form == "noncontiguous_target":
        y = y.transpose(2, 3).contiguous().transpose(2, 3)
        assert not y.is_contiguous()
    else:
        raise KeyError(form)
    assert torch.equal(x, b[0]) and torch.equal(y.float(), b[1])
    return x, y, mask, mean, std


@functools.lru_cache(maxsize=None)
def _form_seq(form):
    if form == "uint8_then_float32_mask":
        return [_as_form(b, "uint8_mask" if k < 4 else "float32_mask") for k, b in enumerate(_seq("full8"))]
    return [_as_form(b, form) for b in _seq("full8")]


@functools.lru_cache(maxsize=None)
def _form_eager(form):
    return _run("plan", _form_seq(form), NEVER)


VARIANTS = {"plan_verified": ("plan", dict(verify=True)), "plan_unverified": ("plan", dict(verify=False)), "graph": ("graph", {})}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("form", FORMS + ["uint8_then_float32_mask"])
def test_batches_the_loss_has_to_convert_keep_the_bits(form, variant):
    """loss._prep converts such a batch with torch kernels.  A hipGraph captures them (the control); a launch plan's recorder does
    not see them, so they must not run inside the recorded region -- and this must not be left to the first replay's
    verification, which verify=False does not have.  The last form switches from a uint8 to a float32 mask of the same shape
    after four steps."""
    cls, kw = VARIANTS[variant]
    e = _form_eager(form)
    r = _run(cls, _form_seq(form), 1, **kw)
    assert getattr(r.step, "plan_rejected", None) is None, r.step.plan_rejected
    assert r.how[:2] == ["warm-up", "capture preparation"]
    if cls == "plan":
        for k, h in enumerate(r.how[2:]):
            # a replay -- or an eager call that says which tensor the plan cannot hold, and why
            assert h is None or any(w in h for w in ("input", "target", "mask", "mean", "std")), (k + 2, h)
    if form in ("bool_mask", "uint8_mask"):
        assert r.how[2:] == [None] * 6 and r.step.replays == 6, r.how        # ordinary batches stay on the fast path
    _same_run(e, r)
    _same_run(_eager("full8"), r)                                            # and the form changes nothing: the values are the same


class _Float32Mask(Dataset):
    def __init__(self, ds):
        self.ds = ds

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, i):
        item = dict(self.ds[i])
        item["loss_mask"] = torch.as_tensor(item["loss_mask"]).to(torch.float32)
        return item


def test_trainer_with_a_launch_plan_on_a_float32_mask_dataset_equals_the_eager_trainer(tmp_path):
    from resdepth_amd import UNet, FusedAdam, Trainer, SyntheticDsmOrthoDataset
    kw = dict(n_input_channels=2, start_kernel=8, depth=2, bias_conv_layer=True)
    torch.manual_seed(0)
    sd0 = copy.deepcopy(UNet(**kw).state_dict())
    res = []
    for planned in (False, True):
        train = DataLoader(_Float32Mask(SyntheticDsmOrthoDataset(22, 2, 32, seed=3)), batch_size=4, shuffle=False)
        val = DataLoader(_Float32Mask(SyntheticDsmOrthoDataset(6, 2, 32, seed=4)), batch_size=4, shuffle=False)
        model = UNet(**kw)
        model.load_state_dict(sd0)
        opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=1e-5)
        d = tmp_path / ("p" if planned else "e")
        tr = Trainer(_args(d, model, opt, train, val, 2, launch_plan=planned, prefetch_batches=0))
        tr.train()
        res.append((tr, torch.load(os.path.join(str(d), "checkpoints", "Model_last.pth"), weights_only=False)))
    (te, le), (tp, lp) = res
    assert tp._graphed is not None and getattr(tp._graphed, "plan_rejected", None) is None
    assert le["loss_train"] == lp["loss_train"] and le["loss_val"] == lp["loss_val"]
    for k, v in le["model_state_dict"].items():
        assert torch.equal(v.cpu(), lp["model_state_dict"][k].cpu()), k
    _same_state(te.model, te.optimizer, tp.model, tp.optimizer)


# ---- 5. a larger eager batch between replays ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["plan", "graph"])
def test_a_larger_eager_batch_between_replays_does_not_pull_the_scratch_from_under_the_plan(cls):
    """Recorded at batch 2; call 5 is an eager iteration at batch 6 on the same weight-gradient stream, whose scratch buffers
    _lib.workspace() replaces when they are too small (at these shapes the 1 MiB minimum may already do for batch 6, so the
    test then asks for a larger buffer itself, as a bigger batch would).  The recorded kernels keep raw pointers: every buffer the
    side stream held at recording time must still be alive at its address afterwards, or the step must have recorded again.
    Bits alone could pass by luck -- what a stale pointer hits depends on the allocator."""
    from resdepth_amd import _lib
    seen = {}

    def side_buffers(model):
        key = (model._side_stream.device.index, model._side_stream.cuda_stream)
        return {k: b for k, b in _lib._ws.items() if k[:2] == key}

    def between(k, step, model, opt):
        if k == 3:                                                           # recorded and verified by call 2
            held = side_buffers(model)
            assert held and step.replays == 1, (held.keys(), step.replays)
            seen["held"] = {key: (weakref.ref(b), b.data_ptr(), b.numel()) for key, b in held.items()}
            seen["captures"] = len(step.test_captures)
        if k == 6:                                                           # right after the batch-6 call
            assert step.why_eager == "batch shape differs from the captured one"
            now = side_buffers(model)
            with torch.cuda.stream(model._side_stream):
                for key, (_, _, numel) in seen["held"].items():
                    if now[key].numel() == numel:                            # batch 6 fitted: a still larger demand
                        _lib.workspace(2 * numel, DEV, slot=key[2])
            now = side_buffers(model)
            assert all(now[key].numel() > numel for key, (_, _, numel) in seen["held"].items())
            seen["alive"] = all(ref() is not None and ref().data_ptr() == ptr for ref, ptr, _ in seen["held"].values())

    e = _eager("larger10", cls)
    r = _run(cls, _seq("larger10"), 1, between=between)
    assert getattr(r.step, "plan_rejected", None) is None
    rerecorded = len(r.captures) > seen["captures"]
    assert seen["alive"] or rerecorded, "the recorded kernels point into scratch buffers that went back to the allocator"
    assert r.step.recordings == len(r.captures)
    assert r.how[5] == "batch shape differs from the captured one" and r.how[6:] == [None] * 4, r.how
    _same_run(e, r)


# ---- 6. one rank of two rejects ----------------------------------------------------------------------------------------------
def test_world2_one_rank_rejecting_makes_both_ranks_fall_back_together(tmp_path):
    """Rank 1's first plan run leaves one wrong bit in a parameter; rank 0's is clean.  The verification's decision is a MIN
    all-reduce: both ranks drop the plan in the same call (neither waits in a collective the other never issues), both
    finish every step eagerly, with the bits of the eager data-parallel run."""
    from test_dp_world2_gpu import run_world
    outs = {}
    for plan in (0, 1):
        d = tmp_path / f"p{plan}"
        d.mkdir()
        extra = dict(reject_rank=1) if plan else {}
        outs[plan] = run_world(d, "plan", coll="staged", batch=4, steps=7, bucket_mb=16, plan=plan, timeout=900, **extra)
    for r in range(2):
        e, p = outs[0][r], outs[1][r]
        assert p["rejected"] == REJECTED, (r, p["rejected"])
        assert p["replays"] == 0 and p["how"][2] == REJECTED and all(h is not None for h in p["how"]), (r, p["how"])
        assert len(p["losses"]) == 7 and torch.equal(e["losses"], p["losses"]), (r, e["losses"], p["losses"])
        assert e["opt_step"] == p["opt_step"] == 7.0
        for k, v in e["state"].items():
            assert torch.equal(v, p["state"][k]), (r, k)
    for k, v in outs[1][0]["state"].items():            # and both ranks hold the same model
        if v.dtype.is_floating_point and "running" not in k:
            assert torch.equal(v, outs[1][1]["state"][k]), k


# ---- 7. checkpoint round trip under a plan -----------------------------------------------------------------------------------
def test_checkpoint_round_trip_and_load_state_dict_record_again():
    """test_graph_gpu's checkpoint scenario for the launch plan: optimizer.load_state_dict between replays replaces the moment
    buffers the plan points into, so the plan is dropped and recorded again -- and the new plan passes its own first-replay
    verification."""
    from resdepth_amd.plan import PlannedTrainStep
    bs = _batches(4, 3)
    ckpt = {}
    res = []
    for planned in (False, True):
        model, opt = _fresh(_sd0())
        step = PlannedTrainStep(model, opt, warmup=1 if planned else NEVER)
        for k in range(5):
            step(*bs[k % 3])
        sd = copy.deepcopy(opt.state_dict())
        assert float(sd["state"][0]["step"]) == 5.0
        if not planned:
            ckpt["opt"], ckpt["model"] = sd, copy.deepcopy(model.state_dict())
        else:
            assert step.replays == 3 and step.recordings == 1 and step._verified
            for i in sd["state"]:
                for k in sd["state"][i]:
                    assert torch.equal(sd["state"][i][k].cpu(), ckpt["opt"]["state"][i][k].cpu()), (i, k)
        model.load_state_dict(ckpt["model"])
        opt.load_state_dict(copy.deepcopy(ckpt["opt"]))
        losses, how = [], []
        for k in range(5):
            losses.append(step(*bs[k % 3]).clone())
            how.append(step.why_eager)
        torch.cuda.synchronize()
        if planned:
            assert how == ["capture preparation", None, None, None, None], how
            assert step.recordings == 2 and step.replays == 7 and step._verified and step.plan_rejected is None
        res.append((model, opt, torch.stack(losses).cpu()))
    (me, oe, le), (mp, op, lp) = res
    assert torch.equal(le, lp), (le, lp)
    _same_state(me, oe, mp, op)
    assert float(op.state_dict()["state"][0]["step"]) == 10.0
