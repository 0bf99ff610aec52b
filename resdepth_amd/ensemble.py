"""All image pairs of a raster in ONE tiled sweep, fused per pixel on the GPU.

The reference predicts a raster once per image pair (test.py:136-189: a loader and a `predict_linear_blend` per entry of
`dataset.image_pairs`) and pools the residuals of all pairs afterwards (test.py:288-313).  Here a
GpuGridTiles(..., 'test', image_pairs=[P pairs], sweep_pairs=True) repeats every tile once per pair, tile-major and pair-minor,
and `predict_pairs_linear_blend` blends the prediction of pair p into plane p of a [P, rows, cols] device raster
(rd_blend_accumulate_planes), reduces the planes per pixel on the device (rd_fuse_planes: mean or median, and the range or
standard deviation over the pairs) and brings back the fused surface, the spread and -- if asked -- the P planes.

Eval-mode inference keeps one magnitude slot per image, so a tile's prediction depends on that tile alone, and the blend adds
per pixel in sample order within a plane: plane p equals, bit for bit, today's single-pair sweep of pair p, whatever the batch
size and wherever a batch cuts a tile's P samples."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops
from .inference import _raster_shape, _sweep_batch
from .trainer import DevicePrefetcher


class PairSweep:
    """What predict_pairs_linear_blend returns: `fused` np.float64 [rows, cols]; `spread` [rows, cols] or None; `pairs`
    np.float64 [P, rows, cols] (plane p = the sweep of image_pairs[p]) or None; `image_pairs`.  The arrays are views of pinned
    host memory the object keeps alive (`host`: with host="reuse" the next call of the same shape overwrites them).
    `device_pairs` / `device_fused`: None, or with keep_device=True the device tensors the sweep produced."""

    def __init__(self, fused, spread, pairs, image_pairs, host, device_pairs=None, device_fused=None):
        self.fused, self.spread, self.pairs, self.image_pairs, self.host = fused, spread, pairs, image_pairs, host
        # with keep_device=True: the sweep's own device tensors ([P, rows, cols] and [rows, cols] fp64), not copies --
        # evaluation.evaluate_pairs_statistics scores them where they are
        self.device_pairs, self.device_fused = device_pairs, device_fused


class _PairHost:
    """Pinned host memory of one call: P + 2 planes of rows x cols doubles at most (fused, spread, the P planes)."""

    def __init__(self, planes, rows, cols):
        self.key = (int(planes), int(rows), int(cols))
        self.t = torch.empty(self.key, dtype=torch.float64, pin_memory=True)


_host_cache = {}


def predict_pairs_linear_blend(dataloader, model, fuse: str = "median", spread=None, return_pairs: bool = True, host=None,
                               keep_device: bool = False):
    """One sweep over a loader that carries the "pair" column (GpuGridTiles(..., sweep_pairs=True)) -> PairSweep.
    fuse: "mean" | "median"; spread: None | "range" | "std" (ops.fuse_planes); return_pairs=False leaves the P planes on the
    device and returns only the fused surface (and the spread): 8 or 16 bytes per raster pixel cross to the host instead of
    8 (P + 1) or 8 (P + 2).  host: None = fresh pinned arrays per call; "reuse" = one cached block per (planes, rows, cols).
    keep_device=True: the PairSweep also carries the device tensors `device_pairs` [P, rows, cols] and `device_fused` (what the
    sweep holds, no copy) for evaluation.evaluate_pairs_statistics; the host results are the same either way."""
    if not torch.cuda.is_available():
        raise RuntimeError("resdepth_amd.predict_pairs_linear_blend runs on a HIP device only (no CPU fallback)")
    if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
        raise RuntimeError("predict_pairs_linear_blend: a process group of world > 1 is not supported (the banded multi-GPU "
                           "delivery holds one plane); sweep in one process")
    if fuse not in ops.FUSE_MODES:
        raise ValueError(f"predict_pairs_linear_blend: fuse must be one of {sorted(ops.FUSE_MODES)} (got {fuse!r})")
    if spread not in ops.SPREAD_MODES:
        raise ValueError(f"predict_pairs_linear_blend: spread must be None, 'range' or 'std' (got {spread!r})")
    ds = dataloader.dataset
    n_pairs = getattr(ds, "n_pairs", None)
    if not n_pairs:
        raise ValueError("predict_pairs_linear_blend needs a loader that sweeps its image pairs: dataset.n_pairs and the "
                         "'pair' batch column (GpuGridTiles(..., image_pairs=[...], sweep_pairs=True))")
    n_pairs = int(n_pairs)
    first = next(model.parameters(), None)
    device = first.device if first is not None and first.is_cuda else torch.device("cuda", torch.cuda.current_device())
    model.eval()
    model.to(device)
    rows, cols = _raster_shape(ds)
    tile_size, stride = int(ds.tile_size), int(ds.stride)
    raster = torch.zeros(n_pairs, rows, cols, dtype=torch.float64, device=device)
    with torch.no_grad():
        for batch in DevicePrefetcher(dataloader, device, 1):
            if "pair" not in batch:
                raise ValueError("predict_pairs_linear_blend: the batch has no 'pair' column (GpuGridTiles(..., sweep_pairs=True))")
            x = batch["input"].to(device, non_blocking=True)
            n = x.shape[0]
            y_pred = model(x)
            mean, std, pos, reg, aug, log2_variants = _sweep_batch(batch, ds, device, n)
            plane = torch.as_tensor(batch["pair"]).flatten().to(device=device, dtype=torch.int32).contiguous()
            if plane.numel() != n:
                raise ValueError("batch dict fields must hold one value per tile")
            with _lib.device_of(raster):
                ops.blend_accumulate(y_pred.contiguous(), mean.contiguous(), std.contiguous(), pos.contiguous(),
                                     reg.contiguous(), tile_size, stride, raster, aug=aug, log2_variants=log2_variants,
                                     plane=plane, n_planes=n_pairs)
    want_spread = ops.SPREAD_MODES[spread] != 0
    planes_out = 1 + int(want_spread) + (n_pairs if return_pairs else 0)
    reuse = isinstance(host, str) and host == "reuse"
    if reuse:
        host = _host_cache.get((planes_out, rows, cols))
    if not isinstance(host, _PairHost) or host.key != (planes_out, rows, cols):
        host = _PairHost(planes_out, rows, cols)
        if reuse:
            _host_cache[host.key] = host
    with _lib.device_of(raster):
        # the fuse runs once, after the last blend: per pixel, so no order of the sweep can show in its bits
        fused, spr = ops.fuse_planes(raster, fuse, spread)
        dst = host.t
        dst[0].copy_(fused, non_blocking=True)
        if want_spread:
            dst[1].copy_(spr, non_blocking=True)
        if return_pairs:
            dst[1 + int(want_spread):].copy_(raster, non_blocking=True)
        torch.cuda.current_stream(device).synchronize()
    out = host.t.numpy()
    return PairSweep(out[0], out[1] if want_spread else None, out[1 + int(want_spread):] if return_pairs else None,
                     getattr(ds, "image_pairs", None), host, raster if keep_device else None, fused if keep_device else None)
