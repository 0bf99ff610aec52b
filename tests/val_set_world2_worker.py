"""One rank of a world-size-N validation epoch over a GpuValSet shard, with the PROCESSES SHARING cuda:0 (torch.distributed over
gloo through tests/host_staged_collectives.py, as tests/dp_world2_worker.py).  Every rank keeps both rasters resident, reads
its runs of the global batches (tiling.val_shard_batches; the last batch is replicated on every rank) and runs
Trainer.inference_one_epoch(0, 'val') under the global loss normaliser.  Driven by tests/test_val_set_world2_gpu.py, which also
imports the scene and the model from here for its single-process run."""
import argparse
import datetime
import os
import sys
import types

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

T = 64
PER_RANK_BATCH = 4
# (raster shape, area, pairs, nodata, dsm_std, ortho_mean, ortho_std): 4 * 5 + 3 * 3 = 29 samples, so a global batch of
# 4 * 2 leaves a tail of 5 that two ranks cannot split
SCENE = (((256, 320), {"x_extent": [(0, 319)], "y_extent": [(0, 255)]}, [[0, 1]], -9999.0, 3.0, 110.0, 50.0),
         ((192, 256), {"x_extent": [(0, 191)], "y_extent": [(0, 191)]}, [[1, 0]], -5000.0, 4.5, None, 44.0))


def make_datasets():
    from resdepth_amd import GpuPatchSampler
    out = []
    for k, ((h, w), area, pairs, nodata, std, omean, ostd) in enumerate(SCENE):
        rng = np.random.RandomState(80 + k)
        dsm = (rng.randn(h, w) * 4 + 420 + 300 * k).astype(np.float32)
        gt = (dsm + rng.randn(h, w) * 1.5).astype(np.float32)
        dsm[100:104, 20:200] = nodata
        gt[30:60, 140:170] = nodata
        gt[::37, ::41] = 0.0
        orthos = (rng.rand(2, h, w) * 200 + 20).astype(np.float32)
        smp = GpuPatchSampler(dsm, gt, orthos, tile_size=T, nodata=nodata, dsm_std=std, ortho_mean=omean, ortho_std=ostd)
        out.append(dict(sampler=smp, area_defn=area, image_pairs=pairs))
    return out


def make_model(dev):
    from resdepth_amd import UNet
    torch.manual_seed(5)
    return UNet(n_input_channels=3, start_kernel=8, depth=3, bias_conv_layer=True).to(dev).eval()


def validation_metric(model, loader, out_dir):
    """Trainer.inference_one_epoch(0, 'val') over `loader` -> (metric, batch sizes the loader yields)."""
    from resdepth_amd import FusedAdam, Trainer
    args = types.SimpleNamespace(
        model=model, optimizer=FusedAdam(model.parameters(), lr=1e-3), scheduler=None, criterion=torch.nn.L1Loss(reduction="mean"),
        trainloader=loader, valloader=loader, n_epochs=1, evaluate_rate=1, save_model_rate=10 ** 9, freq_average_train_loss=20,
        save_dir=out_dir, log_file=None, checkpoint_dir=os.path.join(out_dir, "checkpoints"),
        tboard_log_dir=os.path.join(out_dir, "tb"), pretrained_path=None)
    tr = Trainer(args)
    tr.logger.handlers.clear()
    metric = tr.inference_one_epoch(0, "val")["MAE_metric"].avg
    return metric, [int(b["input"].shape[0]) for b in loader]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--port", type=int, required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(a.port)
    os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=a.rank, world_size=a.world, timeout=datetime.timedelta(seconds=120))
    try:
        import host_staged_collectives
        host_staged_collectives.install()
        from resdepth_amd import GpuValSet, dp
        model = make_model(dev)
        dp.attach(model, sync_bn=False)
        dp.broadcast_parameters(model, 0)
        loader = GpuValSet(make_datasets(), "geom-stereo", batch_size=PER_RANK_BATCH, shard=(a.rank, a.world))
        metric, sizes = validation_metric(model, loader, os.path.join(os.path.dirname(a.out), f"val_out_r{a.rank}"))
        torch.cuda.synchronize()
        torch.save({"metric": metric, "sizes": sizes, "index": loader.dataset.index.tolist(), "n_total": loader.dataset.n_total}, a.out)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
