"""split2h on a whole net whose operands span a wide range, and the slot guard on ordinary data (-m gpu).
csrc/rd_mfma_dev.h (quant_select, amax_commit), DESIGN.md 3.1h.

One scale per operand TENSOR: a batch mate far below the largest tile of the batch would lose the second fp16 term of its
elements (2^-9-class products) -- the guard (slot word 1: smallest non-zero block maximum) sends such launches to the six-product
body.  A net WITHOUT BatchNorm keeps a tile scaled by 2^28 at 2^28 through every layer, which is the case here.  The guard must
not fire on ordinary data, or the default arithmetic silently becomes the slower one."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import unet_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KW = dict(n_input_channels=3, start_kernel=64, depth=3, do_BN=False, bias_conv_layer=True)     # g7's arguments, widened


@pytest.fixture()
def lib():
    from resdepth_amd import _lib
    _lib.load()
    before = _lib.tune_get("mfma_products")
    _lib.tune_set("mfma_products", 3)
    yield _lib
    _lib.tune_set("mfma_products", before)
    _lib._pool_log = None


def _step(batch, products):
    """one training forward + backward of the no-BN net in mode `products` -> (model, sd0, y, {name: grad})"""
    from resdepth_amd import UNet, masked_l1_loss, _lib
    _lib.tune_set("mfma_products", products)
    torch.manual_seed(3)
    model = UNet(**KW)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).train()
    y = model(batch["input"].to(DEV))
    loss = masked_l1_loss(y, batch["target"], batch["loss_mask"], batch["dsm_mean"], batch["dsm_std"])
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}
    _lib.tune_set("mfma_products", 3)
    return model, sd0, y.detach(), grads


def _check_against_oracle(model, sd0, batch, y, grads, tiles):
    from test_unet_gpu import _oracle_fp64_under_hip_decisions, rel_l2
    spec = O.Spec(**{"depth": 8, **KW})
    yo, _, go, _ = _oracle_fp64_under_hip_decisions(model, sd0, spec, batch["input"], batch["target"], batch["loss_mask"],
                                                    batch["dsm_mean"], batch["dsm_std"], y)
    yc = y.cpu().double()
    fwd = [float((yc[t] - yo[t]).abs().max() / yo[t].abs().max()) for t in tiles]
    assert max(fwd) <= 2e-5, fwd
    for (k, p), gr in zip(model.named_parameters(), go):
        assert rel_l2(grads[k], gr) <= 1e-4, (k, rel_l2(grads[k], gr))
    return fwd


def test_no_bn_net_with_a_batch_mate_2e28_above_the_rest(lib):
    """Batch 4: tile 0's input x 2^28 with an all-false loss mask (it contributes nothing to the gradients); tiles 1-3 must come
    out as if they were alone: forward within 2e-5 of the fp64 oracle relative to each tile's own max |y|, every weight / bias
    gradient within 1e-4 rel-L2 under the HIP run's ReLU / pool decisions.  (2^28 > the 2^18 at which an element's second term
    becomes subnormal: without the guard the tiles' activations are 2^-11-class.)"""
    b = O.synthetic_batch(4, KW["n_input_channels"], 64, seed=29)
    b["input"][0] *= 2.0 ** 28
    b["loss_mask"][0] = False
    model, sd0, y, grads = _step(b, 3)
    assert torch.isfinite(y).all() and all(torch.isfinite(g).all() for g in grads.values())
    _check_against_oracle(model, sd0, b, y, grads, (1, 2, 3))


def test_no_bn_net_on_ordinary_data_keeps_the_three_product_bodies(lib):
    """The same net and batch with tile 0 unscaled: the guard does not simply switch split2h off -- the bits differ from a
    six-product run -- and both stay within the bars of the wide-range test above."""
    b = O.synthetic_batch(4, KW["n_input_channels"], 64, seed=29)
    b["loss_mask"][0] = False
    model, sd0, y, grads = _step(b, 3)
    _check_against_oracle(model, sd0, b, y, grads, (1, 2, 3))
    model6, _, y6, grads6 = _step(b, 6)
    assert not torch.equal(y, y6), "the three-product bodies did not run"
    assert any(not torch.equal(grads[k], grads6[k]) for k in grads)
    _check_against_oracle(model6, sd0, b, y6, grads6, (1, 2, 3))


def _written_slots(pools):
    out = []
    for pool in pools:
        for i in range(pool.n):
            words = pool.buf[i * pool.words:(i + 1) * pool.words].cpu().numpy()
            for j in range(max(1, pool.img)):
                w = words[j * 512:(j + 1) * 512]
                if w.any():
                    out.append(w)
    return out


def test_guard_does_not_fire_on_ordinary_data(lib):
    """A BatchNorm net of cfg-S's shape (3 input channels, 64 start channels, depth 5) at batch 2: every magnitude slot its
    training forward, its backward and a per-image inference forward wrote passes the guard, i.e. the three-product body is
    selected for every operand they produced."""
    from resdepth_amd import UNet, masked_l1_loss
    kw = dict(n_input_channels=3, start_kernel=64, depth=5, bias_conv_layer=True)
    torch.manual_seed(0)
    model = UNet(**kw).to(DEV).train()
    b = O.synthetic_batch(2, 3, 256, seed=21)
    lib._pool_log = []
    y = model(b["input"].to(DEV))
    loss = masked_l1_loss(y, b["target"], b["loss_mask"], b["dsm_mean"], b["dsm_std"])
    loss.backward()
    torch.cuda.synchronize()
    train_pools, lib._pool_log = lib._pool_log, []
    model.eval()
    with torch.no_grad():
        model(b["input"].to(DEV))
    torch.cuda.synchronize()
    eval_pools, lib._pool_log = lib._pool_log, None
    assert len(train_pools) >= 2 and any(p.img for p in eval_pools), (len(train_pools), [p.img for p in eval_pools])
    for name, pools in (("train", train_pools), ("eval", eval_pools)):
        slots = _written_slots(pools)
        assert len(slots) >= 10, (name, len(slots))
        bad = [(lib.slot_decode(w)) for w in slots if not lib.slot_takes_three_products(w)]
        assert not bad, (name, len(slots), bad)
