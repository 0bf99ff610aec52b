"""Per-pixel weighted training losses without a GPU: the oracle of tests/wloss_ref.py against the unweighted oracle and against
central differences, the side header include/resdepth_hip_wloss.h against _lib.SIGNATURES_WLOSS and the library, the host-side
validation of the weight arguments, and the weight-tile reference against the orientation of the target plane."""
import os
import re

import numpy as np
import pytest
import torch

import loss_ref
import wloss_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rd_weighted_loss_ws_bytes", "rd_weighted_loss_partial", "rd_weighted_loss_finish", "rd_assemble_train_weights"}
SPECS = [("l1", 1.0), ("l2", 1.0), ("huber", 0.5), ("smooth_l1", 2.0)]


def _batch(shape, seed):
    g = torch.Generator().manual_seed(seed)
    n = shape[0]
    y = torch.randn(shape, generator=g)
    std = torch.rand(n, generator=g) * 7.5 + 0.5
    yp = y + torch.randn(shape, generator=g) * (2.0 / std).reshape(n, 1, 1, 1)
    mean = torch.rand(n, generator=g) * 450.0 - 50.0
    mask = torch.rand(shape, generator=g) < 0.7
    return yp, y, mask, mean, std


@pytest.mark.parametrize("kind,delta", SPECS)
@pytest.mark.parametrize("lam", [0.0, 0.3])
def test_with_unit_weights_the_oracle_is_the_unweighted_oracle_exactly(kind, delta, lam):
    yp, y, mask, mean, std = _batch((3, 1, 5, 7), 5)
    o = loss_ref.masked_loss_oracle(yp, y, mask, mean, std, kind, delta, lam, gout=1.5)
    w = wloss_ref.weighted_loss_oracle(yp, y, mask, torch.ones(3, 1, 5, 7), mean, std, kind, delta, lam, gout=1.5)
    for key in ("loss", "mae", "A", "C", "D", "S"):
        assert w[key] == o[key], key
    assert w["Q"] == float(o["Q"]) and w["Wc"] == o["C"]
    assert torch.equal(w["K"], o["k"].double())
    assert torch.equal(w["g_data"], o["g_data"]) and torch.equal(w["g_slope"], o["g_slope"])


@pytest.mark.parametrize("kind,delta", SPECS)
def test_the_oracle_gradient_agrees_with_central_differences(kind, delta):
    """2x1x4x5, fp64, away from the kinks: std = 1 and mean = 0 make r = fl(yp) - fl(y) with values given on a 1/64 grid (every
    fp32 operation exact), residuals and neighbour differences at least 0.05 from 0 and from delta, and a step of 2^-10."""
    g = torch.Generator().manual_seed(21)
    shape = (2, 1, 4, 5)
    for _ in range(200):
        r = torch.round((torch.rand(shape, generator=g) * 6.0 - 3.0) * 64.0) / 64.0
        dh, dv = r[..., :, :-1] - r[..., :, 1:], r[..., :-1, :] - r[..., 1:, :]
        far = lambda t, c: bool(((t.abs() - c).abs() >= 0.05).all())          # noqa: E731
        if far(r, 0.0) and far(r, delta) and far(dh, 0.0) and far(dv, 0.0):
            break
    else:
        raise AssertionError("no residual field away from the kinks")
    y = torch.round(torch.randn(shape, generator=g) * 64.0) / 64.0
    yp = (y + r).float()
    y = y.float()
    mask = torch.rand(shape, generator=g) < 0.8
    w = torch.rand(shape, generator=g) * 4.0
    w[0, 0, 1, 2] = 0.0
    mean, std = torch.zeros(2), torch.ones(2)
    lam, h = 0.3, 2.0 ** -10
    o = wloss_ref.weighted_loss_oracle(yp, y, mask, w, mean, std, kind, delta, lam)
    assert o["Wc"] > 0 and o["Q"] > 0
    want = o["g_data"] + o["g_slope"]
    num = torch.zeros(shape, dtype=torch.float64)
    for idx in np.ndindex(*shape):
        vals = []
        for sgn in (1.0, -1.0):
            q = yp.clone()
            q[idx] += sgn * h                                                 # exact in fp32 on this grid
            vals.append(wloss_ref.weighted_loss_oracle(q, y, mask, w, mean, std, kind, delta, lam)["loss"])
        num[idx] = (vals[0] - vals[1]) / (2.0 * h)
    # rho is at most quadratic between the kinks: the central difference is exact up to fp64 rounding of the loss / h
    assert float((num - want).abs().max()) <= 1e-10, float((num - want).abs().max())
    assert float(want[~mask.reshape(shape)].abs().max()) == 0.0


def test_weights_scale_out_of_the_loss_and_zero_weights_drop_out():
    yp, y, mask, mean, std = _batch((2, 1, 6, 5), 8)
    g = torch.Generator().manual_seed(3)
    w = torch.rand(2, 1, 6, 5, generator=g) * 4.0
    w[torch.rand(2, 1, 6, 5, generator=g) < 0.2] = 0.0
    a = wloss_ref.weighted_loss_oracle(yp, y, mask, w, mean, std, "huber", 0.5, 0.3)
    b = wloss_ref.weighted_loss_oracle(yp, y, mask, 4.0 * w, mean, std, "huber", 0.5, 0.3)     # exact scaling by a power of two
    assert a["loss"] == b["loss"] and a["mae"] == b["mae"] and torch.equal(a["g_data"], b["g_data"])
    # w = 0 is the same as masking the pixel out of the data term
    c = wloss_ref.weighted_loss_oracle(yp, y, mask & (w > 0), w, mean, std, "huber", 0.5, 0.0)
    d = wloss_ref.weighted_loss_oracle(yp, y, mask, w, mean, std, "huber", 0.5, 0.0)
    assert abs(c["loss"] - d["loss"]) <= 1e-15 * d["loss"] and float(d["g_data"][w == 0].abs().max()) == 0.0
    assert d["mae"] != c["mae"]                       # the MAE is the plain masked MAE: it still counts the w = 0 pixels
    z = wloss_ref.weighted_loss_oracle(yp, y, mask, torch.zeros_like(w), mean, std, "l2", 1.0, 0.3)
    assert z["loss"] != z["loss"] and z["mae"] == d["mae"]
    assert float(z["g_data"].abs().max()) == 0.0 and float(z["g_slope"].abs().max()) == 0.0


def _side_header():
    text = open(os.path.join(ROOT, "include", "resdepth_hip_wloss.h")).read()
    return text, re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def test_side_header_signatures_constants_and_exports():
    from resdepth_amd import _lib
    text, code = _side_header()
    exported = set(re.findall(r"\b(rd_\w+)\s*\(", code))
    assert exported == set(_lib.SIGNATURES_WLOSS) == NAMES
    for name, (_, args) in _lib.SIGNATURES_WLOSS.items():
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1)
        assert len(decl.split(",")) == len(args), name
    defines = dict(re.findall(r"#define\s+(RD_WEIGHT_\w+)\s+(\d+)", code))
    assert {k: int(defines[f"RD_WEIGHT_{k.upper()}"]) for k in _lib.WEIGHT_KINDS} == _lib.WEIGHT_KINDS
    assert int(defines["RD_WEIGHT_TABLE"]) == _lib.WEIGHT_TABLE == 256
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.rd_version() == 116                   # the feature is detected by symbol
    # the scratch query is host arithmetic: one set of six fp64 sums per block, the grid capped
    assert lib.rd_weighted_loss_ws_bytes(1, 1, 1) == 48
    assert lib.rd_weighted_loss_ws_bytes(3, 33, 65) == 3 * 2 * 2 * 48
    assert lib.rd_weighted_loss_ws_bytes(4096, 2, 3) == _lib.LOSS_MAX_BLOCKS * 48
    assert lib.rd_weighted_loss_ws_bytes(0, 4, 4) == 0 and lib.rd_weighted_loss_ws_bytes(1, 1 << 16, 1 << 15) == 0
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    for phrase in ("UNWEIGHTED", "left, right, upper, lower", "THE BITS of rd_masked_loss_partial", "and nothing else",
                   "No scratch", "refused (RD_ERR_WS) with nothing launched", "rd::aug_src", "yields NaN", "train_weight_write"):
        assert phrase in flat, phrase
    # rd_weight_raster is 32 bytes, as the descriptor table of the sampler packs it
    from resdepth_amd import sampler
    assert np.dtype(sampler._WEIGHT_DESC).itemsize == 32 and "} rd_weight_raster; /* 32 bytes */" in text


def test_the_header_is_included_once_named_in_the_build_and_launched_through_rd_launch():
    main = open(os.path.join(ROOT, "include", "resdepth_hip.h")).read()
    assert main.count('#include "resdepth_hip_wloss.h"') == 1
    for name in NAMES:
        assert name not in re.sub(r'#include "resdepth_hip_wloss.h".*', "", main), name
    assert "resdepth_hip_wloss.h" in open(os.path.join(ROOT, "resdepth_amd", "csrc", "build.sh")).read()
    csrc = os.path.join(ROOT, "resdepth_amd", "csrc")
    loss = open(os.path.join(csrc, "rd_loss.hip")).read()
    for launch in ("RD_LAUNCH((masked_loss_partial_kernel<V, WT>)", "RD_LAUNCH(masked_loss_reduce_kernel<NSUM_W>",
                   "RD_LAUNCH((masked_loss_finish_kernel<V, SL, WT>)"):
        assert launch in loss, launch                 # the launch plan records them
    assert "hipLaunchKernelGGL" not in loss and "<<<" not in loss and "atomicAdd" not in loss
    ts = open(os.path.join(csrc, "rd_trainset.hip")).read()
    assert "RD_LAUNCH(train_weight_write," in ts and "aug_src(a, T, r, c + j, sr, sc)" in ts


def test_the_names_live_in_this_header_and_this_table_alone():
    from resdepth_amd import _lib
    inc = os.path.join(ROOT, "include")
    for other in sorted(os.listdir(inc)):
        if other != "resdepth_hip_wloss.h":
            body = open(os.path.join(inc, other)).read()
            for name in NAMES:
                assert name not in body, (other, name)
    tables = [t for t in dir(_lib) if t.startswith("SIGNATURES") and t != "SIGNATURES_WLOSS"]
    assert "SIGNATURES" in tables and len(tables) >= 9
    for table in tables:
        assert not NAMES & set(getattr(_lib, table)), table


def test_the_weight_arguments_are_validated_on_the_host():
    from resdepth_amd import MaskedLoss, masked_loss
    from resdepth_amd.graph import GraphedTrainStep
    t = torch.zeros(2, 1, 4, 4)
    m, one = torch.ones(2, 1, 4, 4, dtype=torch.bool), torch.ones(2)
    with pytest.raises(RuntimeError, match="HIP device"):          # a host weight is refused, whatever else is given
        masked_loss(t, t, m, one, one, kind="l2", weight=torch.ones(2, 1, 4, 4))
    with pytest.raises(RuntimeError, match="HIP device"):
        MaskedLoss("l1")(t, t, m, one, one, weight=torch.ones(2, 4, 4))
    why = GraphedTrainStep._weight_reason
    assert why(None) is None and "HIP device" in why(torch.ones(2, 1, 4, 4))


def test_weight_tile_reference_orients_a_tile_as_the_target_plane():
    """numpy crop, table lookup, oracle.sample_oracle.augment: with the ground-truth raster as the weight raster the tile is the
    target plane of oracle.sample_oracle.assemble before its normalisation, for all eight orientations."""
    from oracle import sample_oracle as S
    rng = np.random.default_rng(5)
    H, W, T = 23, 29, 8
    gt = rng.uniform(400.0, 500.0, (H, W)).astype(np.float32)
    din = gt + rng.normal(0, 1, (H, W)).astype(np.float32)
    orthos = rng.uniform(0, 255, (H, W, 2)).astype(np.float32)
    classes = rng.integers(0, 5, (H, W)).astype(np.uint8)
    table = np.array([0.0, 1.0, 3.0, 0.5, 2.0], dtype=np.float32)
    for code in range(8):
        aug = (code & 3, (code >> 2) & 1, 0) if code < 4 else (code & 3, 0, 1)
        pos = (3 + code, 5 + 2 * code)
        ref = S.assemble(din, gt, orthos, pos, [0, 1], T, -9999.0, 2.0, None, 60.0, aug=aug)
        tile = wloss_ref.weight_tile(gt, None, pos, T, aug)
        back = ref["target"][0] * np.float32(2.0) + np.float32(ref["dsm_mean"])
        assert np.abs(tile - back).max() <= 1e-4 * 500.0                     # the same pixels in the same places
        lut = wloss_ref.weight_tile(classes, table, pos, T, aug)
        assert np.array_equal(lut, wloss_ref.weight_tile(table[classes], None, pos, T, aug))
        assert set(np.unique(lut)) <= set(table.tolist())
