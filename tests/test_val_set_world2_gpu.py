"""A sharded validation epoch at WORLD SIZE 2 on one GPU (-m gpu): two fresh processes share cuda:0 over gloo
(tests/val_set_world2_worker.py, the harness of tests/test_dp_world2_gpu.py), each runs Trainer.inference_one_epoch(0, 'val')
on its GpuValSet shard -- full global batches split between the ranks, the last one replicated -- and both must report the
metric ONE process reports at the global batch size."""
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "val_set_world2_worker.py")
sys.path.insert(0, HERE)
import val_set_world2_worker as W  # noqa: E402

# In eval mode a prediction is per image (BatchNorm folded into the convolutions, no batch statistics), so a tile's prediction
# does not depend on its batch mates and only the order of the loss partial sums differs between the ranks and one process:
# the 1e-6 bar tests/test_dp_world2_gpu.py holds data-parallel losses to.
REL = 1e-6


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _run_world(tmp_path, world=2, timeout=300):
    """`world` fresh worker processes on cuda:0, each under its own timeout; the first failure stops the run (the others are
    killed) and raises with the workers' stderr."""
    port = _free_port()
    outs = [str(tmp_path / f"val_r{r}.pt") for r in range(world)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, WORKER, "--rank", str(r), "--world", str(world), "--port", str(port),
                               "--out", outs[r]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
             for r in range(world)]
    errs, failed = [], False
    for p in procs:
        try:
            _, err = p.communicate(timeout=5 if failed else timeout)
        except subprocess.TimeoutExpired:
            p.kill()
            _, err = p.communicate()
            err = "TIMEOUT\n" + (err or "")
        errs.append(err)
        if p.returncode != 0 and not failed:
            failed = True
            for q in procs:
                if q.poll() is None:
                    q.kill()                  # exactly the PIDs started above
    if failed:
        raise RuntimeError("\n----\n".join(e[-3000:] for e in errs))
    return [torch.load(o, weights_only=False) for o in outs]


def test_world2_validation_metric_equals_one_process_at_the_global_batch(tmp_path):
    from resdepth_amd import GpuValSet, tiling
    outs = _run_world(tmp_path)
    b, world = W.PER_RANK_BATCH, 2
    n = outs[0]["n_total"]
    assert n % (b * world) and (n % (b * world)) % world                       # the tail is replicated
    for r, o in enumerate(outs):
        want = tiling.val_shard_batches(n, b, (r, world))
        assert o["sizes"] == [k1 - k0 for k0, k1 in want] and o["sizes"][-1] == n % (b * world)
        assert o["index"] == [k for k0, k1 in want for k in range(k0, k1)]
    loader = GpuValSet(W.make_datasets(), "geom-stereo", batch_size=b * world)
    ref, sizes = W.validation_metric(W.make_model(torch.device("cuda", 0)), loader, str(tmp_path / "single"))
    assert len(sizes) == len(outs[0]["sizes"]) and sum(sizes) == n
    print("validation metric: ranks", [o["metric"] for o in outs], "one process", ref)
    for r, o in enumerate(outs):
        assert abs(o["metric"] - ref) <= REL * abs(ref), (r, o["metric"], ref)
