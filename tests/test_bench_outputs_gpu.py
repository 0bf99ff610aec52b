"""bench.py as every pull request runs it (-m gpu): a plain run is the headline alone, `--steps` is the number of timed steps,
and `--dump-outputs DIR` writes what the timed path computed in its last step -- training and the cfg-G sweep."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _bench(args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args, capture_output=True, text=True,
                       timeout=timeout, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_training_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    out = tmp_path / "train"
    o = _bench(["--steps", "3", "--warmup", "1", "--batch", "4", "--dump-outputs", str(out)])
    assert o["steps"] == 3 and o["unit"] == "tiles/s" and o["higher_is_better"] is True and o["dtype"] == "f32"
    assert o["ms_per_step"] > 0 and abs(o["value"] - 4 * 3 / (o["ms_per_step"] * 3e-3)) <= 0.01 * o["value"]
    assert len(o["step_ms_min_max"]) == 2 and o["launch_plan"]["enabled"]
    # nothing beyond the headline without --full
    assert "secondary" not in o and "cpu_baseline" not in o and "host_enqueue_ms" not in o
    assert o["roofline"] is None and o["kernels"] == []
    d = {n: np.load(out / f"{n}.npy") for n in ("loss", "params", "adam_exp_avg", "bn_running_stats")}
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in d.values())
    assert sum(v.nbytes for v in d.values()) <= 64_000_000
    assert d["params"].shape == (12625345,)                      # cfg-S: every parameter, after the last step's Adam update
    assert d["adam_exp_avg"].shape == (2_000_000,) and np.abs(d["adam_exp_avg"]).max() > 0
    assert round(float(d["loss"][0]), 6) == o["loss_first_last"][1]


def test_plain_inference_run_dumps_the_blended_raster(tmp_path):
    out = tmp_path / "infer"
    o = _bench(["--infer", "--raster", "1024", "--batch", "8", "--steps", "1", "--warmup", "1", "--dump-outputs", str(out)])
    assert o["steps"] == 1 and o["ms_per_step"] > 0 and o["roofline"] is None and o["kernels"] == []
    r = np.load(out / "raster.npy")
    assert r.dtype == np.float64 and r.shape == (1024 * 1024,)
    assert abs(float(r.sum()) - o["raster_checksum"]) <= 1e-9 * abs(o["raster_checksum"])
