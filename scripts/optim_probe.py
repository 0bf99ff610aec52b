#!/usr/bin/env python3
"""Time of rd_grad_norm at the parameter counts of the cfg-S and cfg-M models, beside the optimizer launch it would precede
(writes one JSON file).  Variants, alternated in one process after every size and variant has been warmed:
  adam_dev    rd_adam_step_dev: the yardstick (28 B / element)
  grad_norm   rd_grad_norm: partial + reduce (4 B / element)
  pair        rd_grad_norm followed by rd_adam_step_dev: what the norm adds to a step (32 B / element)
Each timing is `--reps` (>= 200) calls replayed from ONE captured HIP graph between two device events (device time, no host in
the way), repeated `--rounds` times with the variants alternated inside a round; median, min and max over the rounds, GB/s
from the algorithmic bytes over the median.  `grad_norm` alone re-reads a gradient (50 / 74 MB) that stays in the 256 MB
memory-side cache; in `pair` the optimizer's 350 / 515 MB pass between two norms, as in a step."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = {"cfg-S": 12625345, "cfg-M": 18394497}
BYTES = {"adam_dev": 28, "grad_norm": 4, "pair": 32}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_step.json"))
    args = ap.parse_args()
    assert args.reps >= 200 and args.rounds >= 1
    from resdepth_amd import _lib, ops
    dev = torch.device("cuda", 0)
    t = 100
    b1, b2, lr = 0.9, 0.999, 2e-4
    scalars = torch.tensor([1.0 - b1, b2, 1.0 - b2, 1e-8, 1e-5, lr / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t), 1.0],
                           dtype=torch.float64).float().to(dev)

    def make(n):
        gen = torch.Generator(device=dev).manual_seed(3)
        p, g = (torch.randn(n, device=dev, generator=gen) for _ in range(2))
        g *= 1e-3
        m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        stats = torch.zeros(2, device=dev, dtype=torch.float64)
        ws = torch.empty(max(_lib.load().rd_grad_norm_ws_bytes(n), 16), device=dev, dtype=torch.uint8)

        def pair():
            ops.grad_norm(g, stats, ws)
            ops.adam_step_dev(p, g, m, v, scalars)
        return {"adam_dev": lambda: ops.adam_step_dev(p, g, m, v, scalars), "grad_norm": lambda: ops.grad_norm(g, stats, ws),
                "pair": pair}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / args.reps          # microseconds per call

    result = {"device": torch.cuda.get_device_name(0), "rd_version": _lib.load().rd_version(), "reps": args.reps,
              "rounds": args.rounds, "bytes_per_element": BYTES, "sizes": {}}
    side = torch.cuda.Stream(device=dev)
    for label, n in SIZES.items():
        variants = make(n)
        graphs = {}
        for name, fn in variants.items():                   # warm-up: code objects, allocator; then the capture
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                for _ in range(args.reps):
                    fn()
            g.replay()
            graphs[name] = g
        torch.cuda.synchronize()
        times = {name: [] for name in variants}
        for _ in range(args.rounds):
            for name in variants:
                times[name].append(timed(graphs[name].replay))
        entry = {"numel": n}
        for name, t in times.items():
            med = statistics.median(t)
            entry[name] = {"us": {"median": med, "min": min(t), "max": max(t)}, "gb_per_s": BYTES[name] * n / (med * 1e-6) / 1e9}
        result["sizes"][label] = entry
        del graphs, variants
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
