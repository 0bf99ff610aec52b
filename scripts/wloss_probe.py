#!/usr/bin/env python3
"""Device time of the per-pixel weighted loss launches beside the unweighted ones, and of the weight-tile launch beside the
patch assembly (writes profiles/wloss.json).

Loss kernels at 32 x 1 x 256 x 256, mask Bernoulli(0.7), weights uniform in [0, 4] with 20 % zeros, kind huber (delta 0.5):
  partial          rd_masked_loss_partial   (9 B / pixel)   vs  rd_weighted_loss_partial  (13 B / pixel)
  finish           rd_masked_loss_finish with a gradient, slope_weight 0 (13 B / pixel, no halo)  vs  the weighted one (17 B / pixel)
  finish_slope     the same with slope_weight 0.3 (the halo staged in LDS)
With --parent-lib the unweighted entry points of ANOTHER build of the library (the parent commit's) are timed in the same
process, alternated with this build's: what the templates' new parameter cost the unweighted family, if anything.

Weight tiles: rd_assemble_train_weights for 32 tiles of 256 x 256 cut from a 2048 x 2048 raster (fp32 weights and uint8
classes) against rd_assemble_train_patches for the same sample table (DSM + two views + target + mask: C + 2 planes).

Method (scripts/loss_probe.py): every variant is warmed, then `--reps` (>= 200) calls are captured into ONE HIP graph and the
replay is timed between two device events -- device time of the launches with no host in the way; `--rounds` rounds with the
variants alternated inside a round; median, min and max over the rounds.  The working sets stay inside the 256 MB memory-side
cache from one repetition to the next, as a loss does that finds the network's output there."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libresdepth_hip.so of the parent commit (its unweighted loss entry points)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wloss.json"))
    args = ap.parse_args()
    assert args.reps >= 200 and args.rounds >= 1
    from resdepth_amd import GpuPatchSampler, GpuTrainSet, _lib, ops, sampler
    from resdepth_amd._lib import ptr, stream_ptr
    dev = torch.device("cuda", 0)
    huber = _lib.LOSS_KINDS["huber"]
    shape = (32, 1, 256, 256)
    n, _, h, w = shape
    g = torch.Generator().manual_seed(3)
    y = torch.randn(shape, generator=g)
    yp = (y + torch.randn(shape, generator=g) * 0.5).to(dev)
    y = y.to(dev)
    m = (torch.rand(shape, generator=g) < 0.7).to(torch.uint8).to(dev)
    wt = torch.rand(shape, generator=g) * 4.0
    wt[torch.rand(shape, generator=g) < 0.2] = 0.0
    wt = wt.to(dev)
    mean, std = (torch.rand(n, generator=g) * 450 - 50).to(dev), (torch.rand(n, generator=g) * 7.5 + 0.5).to(dev)
    gout = torch.ones(1, device=dev)
    numel = yp.numel()
    su = ops.masked_loss_partial(yp, y, m, mean, std, huber, 0.5, 1.0)
    sw = ops.weighted_loss_partial(yp, y, m, wt, mean, std, huber, 0.5, 1.0)
    variants = {
        "partial/unweighted": lambda: ops.masked_loss_partial(yp, y, m, mean, std, huber, 0.5, 1.0),
        "partial/weighted": lambda: ops.weighted_loss_partial(yp, y, m, wt, mean, std, huber, 0.5, 1.0),
    }
    for name, lam in (("finish", 0.0), ("finish_slope", 0.3)):
        variants[f"{name}/unweighted"] = lambda lam=lam: ops.masked_loss_finish(
            yp, y, m, mean, std, su, numel, huber, 0.5, 1.0, lam, gout=gout, want_loss=False, want_mae=False)
        variants[f"{name}/weighted"] = lambda lam=lam: ops.weighted_loss_finish(
            yp, y, m, wt, mean, std, sw, numel, huber, 0.5, 1.0, lam, gout=gout, want_loss=False, want_mae=False)
    if args.parent_lib:
        par = C.CDLL(os.path.abspath(args.parent_lib))
        for fname, (res, argt) in _lib.SIGNATURES_LOSS.items():
            fn = getattr(par, fname)
            fn.restype, fn.argtypes = res, argt
        nb = par.rd_masked_loss_ws_bytes(n, h, w)
        pws = torch.empty(nb, dtype=torch.uint8, device=dev)
        psums = torch.empty(8, dtype=torch.float64, device=dev)
        pdyp = torch.empty_like(yp)

        def parent_partial():
            rc = par.rd_masked_loss_partial(ptr(yp), ptr(y), ptr(m), ptr(mean), ptr(std), ptr(psums), n, h, w, huber, 0.5, 1.0,
                                            pws.data_ptr(), nb, stream_ptr())
            assert rc == 0

        def parent_finish(lam):
            rc = par.rd_masked_loss_finish(ptr(yp), ptr(y), ptr(m), ptr(mean), ptr(std), ptr(psums), float(numel), huber, 0.5, 1.0,
                                           lam, ptr(gout), None, None, ptr(pdyp), n, h, w, stream_ptr())
            assert rc == 0
        parent_partial()
        torch.cuda.synchronize()
        assert torch.equal(psums, su), "the parent's sums differ from this build's"
        variants["partial/parent_unweighted"] = parent_partial
        variants["finish/parent_unweighted"] = lambda: parent_finish(0.0)
        variants["finish_slope/parent_unweighted"] = lambda: parent_finish(0.3)

    # ---- weight tiles: one 2048 x 2048 raster, 32 samples of 256 x 256 with random positions and orientations -------------
    T, R = 256, 2048
    rng = np.random.RandomState(5)
    gt = (rng.rand(R, R) * 50 + 400).astype(np.float32)
    dsm = gt + rng.randn(R, R).astype(np.float32)
    orthos = (rng.rand(2, R, R) * 200 + 20).astype(np.float32)
    wr = (rng.rand(R, R) * 4).astype(np.float32)
    classes = rng.randint(0, 6, (R, R)).astype(np.uint8)
    sets = {}
    for kind, kw in (("f32", dict(weight_raster=wr)), ("class_u8", dict(weight_raster=classes, class_weights=[0, 1, 3, .5, 2, 4]))):
        s = GpuPatchSampler(dsm, gt, orthos, tile_size=T, dsm_std=3.0, ortho_std=50.0, **kw)
        np.random.seed(7)
        ts = GpuTrainSet([dict(sampler=s, area_defn={"x_extent": [(0, R - 1)], "y_extent": [(0, R - 1)]}, n_samples=32,
                               image_pairs=[[0, 1]])], "geom-stereo", batch_size=32)
        aug = np.stack([rng.randint(0, 4, 32), rng.randint(0, 2, 32), rng.randint(0, 2, 32)], axis=1)
        tab = torch.from_numpy(ts.table(np.arange(32), aug)).to(dev)
        sets[kind] = (ts, tab)
        variants[f"tiles/weights_{kind}"] = lambda ts=ts, tab=tab: ops.assemble_train_weights(ts._wdesc, 1, tab, ts.views, T)
    ts, tab = sets["f32"]
    variants["tiles/patches"] = lambda: sampler._assemble_train(ts._desc, 1, tab, ts.views, ts.dsm_channel, T, True, {})

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / args.reps          # microseconds per call

    side = torch.cuda.Stream(device=dev)
    graphs = {}
    for name, fn in variants.items():                       # warm-up: code objects, scratch, allocator; then the capture
        for _ in range(20):
            fn()
        with torch.cuda.stream(side):                       # the capture stream's own scratch exists before the capture
            fn()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=side):
            for _ in range(args.reps):
                fn()
        gr.replay()
        graphs[name] = gr
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name in variants:
            times[name].append(timed(graphs[name].replay))
    pixels = n * h * w
    bpp = {"partial/unweighted": 9, "partial/weighted": 13, "partial/parent_unweighted": 9, "finish/unweighted": 13,
           "finish/weighted": 17, "finish/parent_unweighted": 13, "finish_slope/unweighted": 13, "finish_slope/weighted": 17,
           "finish_slope/parent_unweighted": 13}
    tile_bytes = {"tiles/weights_f32": 8.0 * 32 * T * T, "tiles/weights_class_u8": 5.0 * 32 * T * T,
                  "tiles/patches": (8.0 * 4 + 1.0) * 32 * T * T + 4.0 * 3 * 32 * T * T}
    result = {"device": torch.cuda.get_device_name(0), "rd_version": _lib.load().rd_version(), "reps": args.reps,
              "rounds": args.rounds, "loss_shape": "x".join(map(str, shape)), "tiles": "32 x 256 x 256 from 2048 x 2048",
              "parent_lib": bool(args.parent_lib), "us": {}, "gb_per_s": {}, "ratio_weighted_over_unweighted": {}}
    for name, v in times.items():
        med = statistics.median(v)
        result["us"][name] = {"median": med, "min": min(v), "max": max(v)}
        nbytes = bpp[name] * pixels if name in bpp else tile_bytes[name]
        result["gb_per_s"][name] = nbytes / (med * 1e-6) / 1e9
    for k, (a, b) in {"partial": (13, 9), "finish": (17, 13), "finish_slope": (17, 13)}.items():
        result["ratio_weighted_over_unweighted"][k] = {
            "time": result["us"][f"{k}/weighted"]["median"] / result["us"][f"{k}/unweighted"]["median"], "bytes": a / b}
    result["ratio_weight_tiles_over_patches"] = {
        k: result["us"][f"tiles/weights_{k}"]["median"] / result["us"]["tiles/patches"]["median"] for k in ("f32", "class_u8")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if os.path.exists(args.out):                            # the step rates of bench.py are recorded beside the kernel times by hand
        kept = json.load(open(args.out)).get("bench_tiles_per_s")
        if kept is not None:
            result["bench_tiles_per_s"] = kept
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
