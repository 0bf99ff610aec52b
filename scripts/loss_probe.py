#!/usr/bin/env python3
"""Time of the loss launches of one training step -- forward (partial + reduce + finish) and backward (finish with a gradient) --
for three variants, alternated in one process after every shape and variant has been warmed (writes one JSON file):
  l1            the rd_masked_l1_* trio (what masked_l1_loss launches)
  l2            rd_masked_loss_* with kind l2, slope_weight 0            (no halo staged in the backward)
  huber_slope   rd_masked_loss_* with kind huber (delta 0.5), slope_weight 0.3
at 32 x 1 x 256 x 256 and 32 x 1 x 512 x 512, masks Bernoulli(0.7).  All three move 9 B / pixel in the forward and 13 B / pixel in
the backward.  Two timings per variant, each `--reps` (>= 200) forward + backward pairs between two device events, repeated
`--rounds` times with the variants alternated inside a round:
  graph_us   the pairs replayed from ONE captured HIP graph: device time of the four launches, no host in the way
  eager_us   the pairs enqueued by the ops wrappers: what a step sees when the host is the slower side (at these sizes the
             kernels take a few microseconds, an enqueue from Python takes longer)
median, min and max over the rounds; GB/s from the algorithmic bytes (22 B / pixel) over the graph time.  The working set of
either shape (13 bytes per pixel: 27 MB and 109 MB) stays inside the 256 MB memory-side cache from one repetition to the next:
the rates are those of a loss that finds the network's output there, as it does in a step."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_kernels.json"))
    args = ap.parse_args()
    assert args.reps >= 200 and args.rounds >= 1
    from resdepth_amd import _lib, ops
    dev = torch.device("cuda", 0)
    huber, l2 = _lib.LOSS_KINDS["huber"], _lib.LOSS_KINDS["l2"]

    def make(shape):
        g = torch.Generator().manual_seed(3)
        y = torch.randn(shape, generator=g)
        yp = (y + torch.randn(shape, generator=g) * 0.5).to(dev)
        m = (torch.rand(shape, generator=g) < 0.7).to(torch.uint8).to(dev)
        n = shape[0]
        mean, std = (torch.rand(n, generator=g) * 450 - 50).to(dev), (torch.rand(n, generator=g) * 7.5 + 0.5).to(dev)
        gout = torch.ones(1, device=dev)
        t = (yp, y.to(dev), m, mean, std)
        numel = yp.numel()

        def l1():
            s = ops.masked_l1_partial(*t)
            ops.masked_l1_finish(*t, s, numel, want_loss=True, want_grad=False)
            return ops.masked_l1_finish(*t, s, numel, gout=gout, want_loss=False, want_grad=True)[1]

        def new(kind, delta, lam):
            def run():
                s = ops.masked_loss_partial(*t, kind, delta, 1.0)
                ops.masked_loss_finish(*t, s, numel, kind, delta, 1.0, lam, want_grad=False)
                return ops.masked_loss_finish(*t, s, numel, kind, delta, 1.0, lam, gout=gout, want_loss=False, want_mae=False)[2]
            return run
        return {"l1": l1, "l2": new(l2, 1.0, 0.0), "huber_slope": new(huber, 0.5, 0.3)}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / args.reps          # microseconds per forward + backward pair

    result = {"device": torch.cuda.get_device_name(0), "rd_version": _lib.load().rd_version(), "reps": args.reps,
              "rounds": args.rounds, "bytes_per_pixel": {"forward": 9, "backward": 13}, "shapes": {}}
    side = torch.cuda.Stream(device=dev)
    for shape in ((32, 1, 256, 256), (32, 1, 512, 512)):
        variants = make(shape)
        graphs = {}
        for name, fn in variants.items():                   # warm-up: code objects, scratch, allocator; then the capture
            for _ in range(20):
                fn()
            with torch.cuda.stream(side):                   # the capture stream's own scratch exists before the capture
                fn()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                for _ in range(args.reps):
                    fn()
            g.replay()
            graphs[name] = g
        torch.cuda.synchronize()
        times = {name: {"graph_us": [], "eager_us": []} for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                times[name]["graph_us"].append(timed(graphs[name].replay))
            for name, fn in variants.items():
                times[name]["eager_us"].append(timed(lambda: [fn() for _ in range(args.reps)]))
        pixels = shape[0] * shape[2] * shape[3]
        entry = {}
        for name, t in times.items():
            entry[name] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in t.items()}
            entry[name]["graph_gb_per_s"] = 22.0 * pixels / (entry[name]["graph_us"]["median"] * 1e-6) / 1e9
        result["shapes"]["x".join(map(str, shape))] = entry
        del graphs
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
