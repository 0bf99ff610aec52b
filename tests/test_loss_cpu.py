"""The masked training losses beyond L1, without a GPU: the oracle of tests/loss_ref.py against torch's own autograd and against
a literal double loop, the criterion mapping, the host-side validation of resdepth_amd.masked_loss, and the side header
include/resdepth_hip_loss.h against _lib.SIGNATURES_LOSS and the library."""
import os
import re

import pytest
import torch
from torch import nn

import loss_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _batch(shape, seed):
    """De-normalised values inside ONE binade ([256, 512)): there fp32 p - t is exact, so the float64 autograd reference below,
    which subtracts in float64, sees the residual the oracle holds."""
    g = torch.Generator().manual_seed(seed)
    n = shape[0]
    y = torch.randn(shape, generator=g)
    std = torch.rand(n, generator=g) * 7.5 + 0.5
    yp = y + torch.randn(shape, generator=g) * (2.0 / std).reshape(n, 1, 1, 1)
    mean = torch.tensor([300.0, 320.0, 400.0])[:n]
    mask = torch.rand(shape, generator=g) < 0.7
    return yp, y, mask, mean, std


@pytest.mark.parametrize("kind,delta,crit", [
    ("l1", 1.0, nn.L1Loss()), ("l2", 1.0, nn.MSELoss()), ("huber", 0.5, nn.HuberLoss(delta=0.5)),
    ("huber", 3.0, nn.HuberLoss(delta=3.0)), ("smooth_l1", 2.0, nn.SmoothL1Loss(beta=2.0)),
    ("smooth_l1", 0.0, nn.SmoothL1Loss(beta=0.0))])
def test_the_oracle_is_the_generic_expression_under_torch_autograd(kind, delta, crit):
    """lib/Trainer.py:87-100 applied the generic way in float64: zero the masked pixels of both de-normalised tensors, apply the
    criterion, multiply by numel / mask.sum()."""
    yp, y, mask, mean, std = _batch((3, 1, 5, 7), 5)
    o = loss_ref.masked_loss_oracle(yp, y, mask, mean, std, kind, delta, 0.0)
    sd, mu = std.reshape(3, 1, 1, 1), mean.reshape(3, 1, 1, 1)
    p32, t32 = yp * sd + mu, y * sd + mu
    assert float(p32.min()) >= 256.0 and float(p32.max()) < 512.0 and float(t32.min()) >= 256.0 and float(t32.max()) < 512.0
    p = p32.double().requires_grad_()
    t, m = t32.double(), mask.double()
    loss = crit(p * m, t * m) * m.numel() / m.sum()
    loss.backward()
    g = p.grad * sd.double()                       # d/dy_pred: p = y_pred * std + mean
    assert abs(o["loss"] - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    assert float((o["g_data"] - g).abs().max()) <= 1e-12 * float(g.abs().max())
    assert float(o["g_slope"].abs().max()) == 0.0
    mae = float(((p.detach() - t).abs() * m).sum() / m.sum())
    assert abs(o["mae"] - mae) <= 1e-12 * mae


def test_pair_sums_and_the_stencil_against_a_literal_double_loop():
    g = torch.Generator().manual_seed(9)
    r = (torch.randn(2, 1, 3, 4, generator=g) * 2).float()
    r[0, 0, 1, 1] = r[0, 0, 1, 2]                  # a flat pair: contributes 0 to S's signs and to k
    m = torch.tensor([[[1, 1, 0, 1], [1, 1, 1, 1], [0, 1, 1, 0]],
                      [[0, 1, 0, 1], [1, 0, 1, 0], [1, 1, 1, 1]]], dtype=torch.bool).reshape(2, 1, 3, 4)
    S, Q, k = loss_ref.pair_terms(r, m)
    S2, Q2, k2 = 0.0, 0, torch.zeros(2, 1, 3, 4, dtype=torch.int64)
    sign = lambda v: (v > 0) - (v < 0)             # noqa: E731
    for n in range(2):
        for i in range(3):
            for j in range(4):
                for di, dj in ((0, 1), (1, 0)):
                    a, b = (n, 0, i, j), (n, 0, i + di, j + dj)
                    if b[2] < 3 and b[3] < 4 and m[a] and m[b]:
                        d = float(r[a] - r[b])     # one fp32 subtraction
                        S2 += abs(d)
                        Q2 += 1
                        k2[a] += sign(d)
                        k2[b] -= sign(d)
    assert Q == Q2 > 0 and abs(S - S2) <= 1e-12 * S2
    assert torch.equal(k * m, k2)
    assert int(k2.abs().max()) <= 4
    # the whole oracle on residuals that ARE these values: y_pred = r, y = 0, std = 1, mean = 0
    o = loss_ref.masked_loss_oracle(r, torch.zeros_like(r), m, torch.zeros(2), torch.ones(2), "l2", 1.0, 0.3)
    assert o["Q"] == Q2 and abs(o["S"] - S2) <= 1e-12 * S2 and torch.equal(o["k"], k2)
    assert abs(o["loss"] - (o["D"] / o["C"] + 0.3 * S2 / Q2)) <= 1e-15
    assert torch.equal(o["g_slope"], 0.3 / Q2 * k2.double())


def test_criterion_spec_maps_what_the_fused_loss_implements_and_names_it_otherwise():
    from resdepth_amd import MaskedLoss
    from resdepth_amd.loss import criterion_spec
    assert criterion_spec(nn.L1Loss()) == ("l1", 1.0, 0.0)
    assert criterion_spec(nn.MSELoss(reduction="mean")) == ("l2", 1.0, 0.0)
    assert criterion_spec(nn.HuberLoss(delta=0.5)) == ("huber", 0.5, 0.0)
    assert criterion_spec(nn.SmoothL1Loss(beta=2.0)) == ("smooth_l1", 2.0, 0.0)
    assert criterion_spec(nn.SmoothL1Loss(beta=0.0)) == ("l1", 1.0, 0.0)
    assert criterion_spec(MaskedLoss("huber", 0.25, 0.3)) == ("huber", 0.25, 0.3)
    assert criterion_spec(MaskedLoss("l2", slope_weight=0.5)) == ("l2", 1.0, 0.5)
    for bad in (nn.L1Loss(reduction="sum"), nn.MSELoss(reduction="none"), nn.HuberLoss(reduction="sum"), nn.BCELoss()):
        with pytest.raises(NotImplementedError) as e:
            criterion_spec(bad)
        for name in ("nn.L1Loss", "nn.MSELoss", "nn.HuberLoss", "nn.SmoothL1Loss", "MaskedLoss"):
            assert name in str(e.value), str(e.value)


def test_masked_loss_validates_on_the_host_and_names_the_argument():
    from resdepth_amd import MaskedLoss, masked_loss
    t = torch.zeros(2, 1, 4, 4)
    m, one = torch.ones(2, 1, 4, 4, dtype=torch.bool), torch.ones(2)
    args = (t, t, m, one, one)
    for kw, word in ((dict(kind="l3"), "kind"), (dict(kind="huber", delta=0.0), "delta"), (dict(kind="huber", delta=-1.0), "delta"),
                     (dict(kind="smooth_l1", delta=float("nan")), "delta"), (dict(kind="l2", slope_weight=-0.1), "slope_weight"),
                     (dict(kind="l2", slope_weight=float("inf")), "slope_weight"),
                     (dict(kind="l2", slope_weight=float("nan")), "slope_weight")):
        with pytest.raises(ValueError, match=word):
            masked_loss(*args, **kw)
        with pytest.raises(ValueError, match=word):
            MaskedLoss(**kw)
    for shape in ((2, 4, 4), (2, 2, 4, 4), (2, 1, 1, 4, 4)):
        z = torch.zeros(shape)
        with pytest.raises(ValueError, match="4-D"):
            masked_loss(z, z, torch.ones(shape, dtype=torch.bool), one, one, kind="l2", slope_weight=0.1)
    with pytest.raises(RuntimeError, match="HIP device"):          # valid arguments: the host tensor is what is refused
        masked_loss(*args, kind="l2")


def _side_header():
    text = open(os.path.join(ROOT, "include", "resdepth_hip_loss.h")).read()
    return text, re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def test_side_header_signatures_constants_and_version():
    from resdepth_amd import _lib
    main = open(os.path.join(ROOT, "include", "resdepth_hip.h")).read()
    assert '#include "resdepth_hip_loss.h"' in main
    assert "rd_masked_loss" not in re.sub(r'#include "resdepth_hip_loss.h".*', "", main)
    _, code = _side_header()
    exported = set(re.findall(r"\b(rd_\w+)\s*\(", code))
    assert exported == set(_lib.SIGNATURES_LOSS) == {"rd_masked_loss_ws_bytes", "rd_masked_loss_partial", "rd_masked_loss_finish"}
    defines = dict(re.findall(r"#define\s+(RD_LOSS_\w+)\s+(\d+)", code))
    assert {k: int(defines[f"RD_LOSS_{k.upper()}"]) for k in _lib.LOSS_KINDS} == _lib.LOSS_KINDS
    assert (int(defines["RD_LOSS_STRIP_ROWS"]), int(defines["RD_LOSS_STRIP_COLS"]), int(defines["RD_LOSS_MAX_BLOCKS"])) == \
        (_lib.LOSS_STRIP_ROWS, _lib.LOSS_STRIP_COLS, _lib.LOSS_MAX_BLOCKS)
    lib = _lib.load()
    assert lib.rd_version() >= 114
    # the scratch query is host arithmetic: one set of five fp64 sums per block, the grid capped
    assert lib.rd_masked_loss_ws_bytes(1, 1, 1) == 40
    assert lib.rd_masked_loss_ws_bytes(3, 33, 65) == 3 * 2 * 2 * 40
    assert lib.rd_masked_loss_ws_bytes(4096, 2, 3) == _lib.LOSS_MAX_BLOCKS * 40
    assert lib.rd_masked_loss_ws_bytes(0, 4, 4) == 0 and lib.rd_masked_loss_ws_bytes(1, 1 << 16, 1 << 15) == 0


def test_the_new_unit_is_built_and_launches_through_rd_launch():
    build = open(os.path.join(ROOT, "resdepth_amd", "csrc", "build.sh")).read()
    # one list of translation units feeds the compile loop and, through the loop's objs array, the link line
    units = re.search(r'^UNITS="([^"]*)"$', build, re.M).group(1).split()
    assert "rd_loss" in units and "for f in $UNITS; do" in build and 'objs+=("$OBJ/$f.o")' in build
    assert re.search(r'^\$HIPCC [^\n]*-shared [^\n]*-o "\$OUT" "\$\{objs\[@\]\}"$', build, re.M)
    src = open(os.path.join(ROOT, "resdepth_amd", "csrc", "rd_loss.hip")).read()
    assert "RD_LAUNCH(" in src and "hipLaunchKernelGGL" not in src and "<<<" not in src and "atomicAdd" not in src
