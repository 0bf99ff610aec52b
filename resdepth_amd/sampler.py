"""Training-sample assembly on the GPU: the per-sample work of the reference's
`DsmOrthoDataset.__getitem__` (lib/DsmOrthoDataset.py:161-291) -- patch extraction, masked per-patch mean centring and
division by the global DSM std, ortho-image normalisation, loss mask, rot90 / flip augmentation
(lib/torch_transforms.py) -- as two kernels over rasters that stay resident in HBM (288 GB holds any city raster),
producing the collated batch dict directly on the device.  The reference does this per sample on the CPU with
per-channel numpy loops and cannot feed more than a few hundred tiles/s.

Raster I/O (GeoTIFF via GDAL) and the choice of valid patch positions stay with the caller (out of scope)."""
from __future__ import annotations

import warnings

import numpy as np
import torch

from . import _lib, ops, tiling
from ._lib import check, load, ptr, stream_ptr

# the per-tile metadata columns of a batch dict, in the column order of the loaders' tables ([pos (y, x) | box])
_META = ("patch_offset_y", "patch_offset_x", "patch_valid_pixels_uly", "patch_valid_pixels_ulx", "patch_valid_pixels_lry",
         "patch_valid_pixels_lrx")
_VIEW_CHANNELS = ("geom-mono", "geom-stereo", "geom-multiview", "stereo")


def _transform_mode(enabled, mean):
    """(mode, mean) of a DSM / ortho transform as the assembly kernels take it: 0 raw, 1 the given mean, 2 each tile's own mean
    (`not mean`, None or 0.0: the reference's test)."""
    mode = 0 if not enabled else (2 if not mean else 1)
    return mode, (float(mean) if mode == 1 else 0.0)


def _aug_code(aug, n=-1):
    """int [n, 3] (k, flip_v, flip_h), a tensor or anything numpy reads -> int32 [n] orientation codes k | flip_v << 2 |
    flip_h << 3 of the same kind (tiling.tta_codes: the one encoding of every loader and kernel)."""
    a = aug.to(torch.int32) if torch.is_tensor(aug) else np.asarray(aug, dtype=np.int32)
    a = a.reshape(n, 3)
    return a[:, 0] | (a[:, 1] << 2) | (a[:, 2] << 3)


def _draw_aug(n, generator):
    """The reference's augmentation draws for n samples -> int64 [n, 3]: k in {0..3}, then flip_v, then flip_h (each with
    probability 1/2).  This order of the three draws is what makes a seeded generator reproduce a run."""
    return torch.stack([torch.randint(0, 4, (n,), generator=generator), torch.randint(0, 2, (n,), generator=generator),
                        torch.randint(0, 2, (n,), generator=generator)], 1)


def _queued(jobs, produce, depth):
    """The loaders' queue: `produce(job)` runs max(0, depth) jobs ahead of the item handed out, in job order; the queue is
    drained at the end.  min(n_jobs, k + depth + 1) jobs are produced when item k is yielded."""
    queue = []
    for job in jobs:
        queue.append(produce(job))
        if len(queue) > max(0, int(depth)):
            yield queue.pop(0)
    while queue:
        yield queue.pop(0)


def _prefetched(device, jobs, assemble, depth, side=None):
    """Generator of `assemble(job)` (a batch dict) for every job, assembled `depth` batches AHEAD on a side stream (`side`, or a
    fresh one) and handed to the consumer's stream in job order (_hand_over): the prefetch of every loader of this module."""
    if side is None:
        with torch.cuda.device(device):
            side = torch.cuda.Stream(device=device)

    def produce(job):
        with torch.cuda.device(device), torch.cuda.stream(side):
            b = assemble(job)
            ev = torch.cuda.Event()
            ev.record(side)
        return b, ev

    for item in _queued(jobs, produce, depth):
        yield _hand_over(device, item)


def _hand_over(device, item):
    """(batch, event recorded behind its assembly) -> the batch, safe to use on `device`'s current stream: that stream waits
    on the one event, and every device tensor of the dict is pinned to it with `record_stream`."""
    b, ev = item
    cur = torch.cuda.current_stream(device)
    cur.wait_event(ev)
    for v in b.values():
        if torch.is_tensor(v) and v.is_cuda:
            v.record_stream(cur)
    return b


class GpuPatchSampler:
    def __init__(self, dsm_input, dsm_target=None, orthos=None, tile_size: int = 256, nodata: float = -9999.0,
                 dsm_std: float = 1.0, ortho_mean=None, ortho_std: float = 1.0, device="cuda", weight_raster=None,
                 class_weights=None):
        """dsm_input / dsm_target: [H, W] float32; orthos: [V_total, H, W] float32 (planar).  ortho_mean=None => per-patch
        mean over the views of the sample (lib/DsmOrthoDataset.py:231-233).

        weight_raster: per-pixel loss weights for the batches of GpuTrainSet / GpuValSet (`batch["loss_weight"]`), kept in HBM
        beside the rasters: an [H, W] float32 raster of finite weights >= 0 (checked once, on the device), or -- with
        class_weights, a table of at most 256 finite weights >= 0 (checked on the host) -- an [H, W] uint8 class raster whose
        weights are looked up when a tile is cut (1 byte per pixel instead of 4)."""
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("resdepth_amd.GpuPatchSampler needs a HIP device (no CPU fallback)")
        f = lambda t: None if t is None else torch.as_tensor(t, dtype=torch.float32).to(dev).contiguous()
        self.dsm_in, self.dsm_gt, self.orthos = f(dsm_input), f(dsm_target), f(orthos)
        self.h, self.w = self.dsm_in.shape
        self.tile, self.nodata = int(tile_size), float(nodata)
        self.dsm_std, self.ortho_mean, self.ortho_std = float(dsm_std), ortho_mean, float(ortho_std)
        self.device = dev
        self.weight, self.weight_table, self.weight_kind = self._check_weights(weight_raster, class_weights)

    def _check_weights(self, raster, table):
        """-> (device raster | None, device table of _lib.WEIGHT_TABLE floats | None, kind code | None)"""
        if raster is None:
            if table is not None:
                raise ValueError("GpuPatchSampler: class_weights needs the uint8 class raster as weight_raster")
            return None, None, None
        dev = self.device
        if table is None:
            w = torch.as_tensor(raster)
            if not w.dtype.is_floating_point:
                raise ValueError(f"GpuPatchSampler: weight_raster of dtype {w.dtype} needs class_weights (a float raster holds "
                                 "the weights themselves)")
            w = w.to(torch.float32).to(dev).contiguous()
            if tuple(w.shape) != (self.h, self.w):
                raise ValueError(f"GpuPatchSampler: weight_raster of shape {tuple(w.shape)}, the rasters are {self.h} x {self.w}")
            if not bool((torch.isfinite(w) & (w >= 0)).all()):
                raise ValueError("GpuPatchSampler: weight_raster must be finite and >= 0 everywhere")
            return w, None, _lib.WEIGHT_KINDS["f32"]
        tab = np.asarray(table, dtype=np.float64).reshape(-1)
        if not 1 <= tab.size <= _lib.WEIGHT_TABLE:
            raise ValueError(f"GpuPatchSampler: class_weights holds {tab.size} weights (1..{_lib.WEIGHT_TABLE})")
        if not bool((np.isfinite(tab) & (tab >= 0)).all()):
            raise ValueError("GpuPatchSampler: class_weights must be finite and >= 0")
        c = torch.as_tensor(raster)
        if c.dtype != torch.uint8:
            raise ValueError(f"GpuPatchSampler: with class_weights the weight_raster holds uint8 classes (got {c.dtype})")
        c = c.to(dev).contiguous()
        if tuple(c.shape) != (self.h, self.w):
            raise ValueError(f"GpuPatchSampler: weight_raster of shape {tuple(c.shape)}, the rasters are {self.h} x {self.w}")
        if int(c.max()) >= tab.size:
            raise ValueError(f"GpuPatchSampler: class {int(c.max())} in weight_raster, class_weights holds {tab.size} weights")
        full = np.zeros(_lib.WEIGHT_TABLE, dtype=np.float32)
        full[:tab.size] = tab.astype(np.float32)
        return c, torch.from_numpy(full).to(dev), _lib.WEIGHT_KINDS["class_u8"]

    def sample(self, positions, pairs=None, aug=None):
        """positions: int [n,2] (y, x); pairs: int [n,V] plane indices into `orthos`; aug: int [n,3] (k, flip_v, flip_h)
        or None.  Returns the DataLoader-shaped batch dict with device tensors."""
        with torch.cuda.device(self.device):       # raw launches go to the current device's stream
            return self._sample(positions, pairs, aug)

    def _sample(self, positions, pairs, aug):
        dev, t = self.device, self.tile
        pos = torch.as_tensor(positions, dtype=torch.int32).reshape(-1, 2)
        if not pos.is_cuda:          # validate on the host (no device->host sync in the training loop)
            if int(pos[:, 0].max()) + t > self.h or int(pos[:, 1].max()) + t > self.w or int(pos.min()) < 0:
                raise ValueError("patch position outside the raster")
        pos = pos.to(dev).contiguous()
        n = pos.shape[0]
        v = 0
        pair_t = omean = None
        if self.orthos is not None and pairs is not None:
            pair_t = torch.as_tensor(pairs, dtype=torch.int32).reshape(n, -1).to(dev).contiguous()
            v = pair_t.shape[1]
        zero = torch.zeros(n, dtype=torch.int32, device=dev)
        sums = torch.empty(n, 2, dtype=torch.float64, device=dev)
        check(load().rd_patch_sums(ptr(self.dsm_in), self.h * self.w, ptr(zero), 1, ptr(pos), n, t, self.w, self.nodata, 1,
                                   ptr(sums), stream_ptr()), "patch_sums")
        dsm_mean = (sums[:, 0] / sums[:, 1]).to(torch.float32)
        if v:
            if self.ortho_mean is None:
                osum = torch.empty(n, 2, dtype=torch.float64, device=dev)
                check(load().rd_patch_sums(ptr(self.orthos), self.h * self.w, ptr(pair_t), v, ptr(pos), n, t, self.w, 0.0, 0,
                                           ptr(osum), stream_ptr()), "patch_sums")
                omean = (osum[:, 0] / osum[:, 1]).to(torch.float32)
            else:
                omean = torch.full((n,), float(self.ortho_mean), dtype=torch.float32, device=dev)
        aug_t = None
        if aug is not None:
            aug_t = _aug_code(torch.as_tensor(aug, dtype=torch.int32), n).to(dev).contiguous()
        inp = torch.empty(n, 1 + v, t, t, dtype=torch.float32, device=dev)
        tgt = msk = None
        if self.dsm_gt is not None:
            tgt = torch.empty(n, 1, t, t, dtype=torch.float32, device=dev)
            msk = torch.empty(n, 1, t, t, dtype=torch.uint8, device=dev)
        check(load().rd_assemble_patches(ptr(self.dsm_in), ptr(self.dsm_gt), ptr(self.orthos) if v else None,
                                         self.h * self.w, ptr(pair_t), v, ptr(pos), ptr(aug_t), ptr(dsm_mean), self.dsm_std,
                                         ptr(omean), self.ortho_std, self.nodata, n, t, self.w, ptr(inp), ptr(tgt), ptr(msk),
                                         stream_ptr()), "assemble_patches")
        batch = {"input": inp, "dsm_mean": dsm_mean, "dsm_std": torch.full((n,), self.dsm_std, device=dev),
                 "patch_offset_x": pos[:, 1], "patch_offset_y": pos[:, 0],
                 "nodata": torch.full((n,), self.nodata, device=dev)}
        if tgt is not None:
            batch["target"], batch["loss_mask"] = tgt, msk.view(torch.bool)
        return batch

    def random_batch(self, n: int, pairs, generator=None, augment: bool = True):
        """n random patch positions (uniform over the raster) + the reference's augmentation draws
        (k in {0..3}, flips with probability 1/2)."""
        g = generator
        ys = torch.randint(0, self.h - self.tile + 1, (n,), generator=g)
        xs = torch.randint(0, self.w - self.tile + 1, (n,), generator=g)
        aug = _draw_aug(n, g) if augment else None
        pair = torch.as_tensor(pairs, dtype=torch.int32)
        if pair.dim() == 1:
            pair = pair.unsqueeze(0).expand(n, -1)
        return self.sample(torch.stack([ys, xs], 1), pair, aug)

    def stream_batches(self, n_batches: int, batch_size: int, pairs, generator=None, augment: bool = True, prefetch: int = 1):
        """Generator of `n_batches` random training batches (the dict of `random_batch`) assembled `prefetch` batches AHEAD on a
        side stream, so that the two assembly kernels of batch k + 1 (0.26 ms for 32 tiles of 256 x 256 x 3) run under batch k's
        forward / backward instead of in front of its own: the consumer's stream waits on one event per batch and the tensors
        are pinned to it with `record_stream`.  The positions / augmentation draws come from `generator` in the same order as
        consecutive `random_batch` calls, so the stream of batches is the same with or without prefetch."""
        return _prefetched(self.device, range(n_batches),
                           lambda k: self.random_batch(batch_size, pairs, generator=generator, augment=augment), prefetch)


class SamplerLoader:
    """A `trainloader` for resdepth_amd.Trainer (lib/Trainer.py:61-64,165: anything with `len()` that yields batch dicts) fed by a
    GpuPatchSampler: `n_batches` random augmented batches per epoch, assembled on the GPU one batch ahead (`stream_batches`).
    Takes the place of DataLoader(DsmOrthoDataset(...)) when the rasters fit in HBM (lib/DsmOrthoDataset.py:161-291 does the same
    per-sample work on the CPU).  `generator`: a CPU torch.Generator for the positions / augmentation draws (its state advances
    from epoch to epoch, as a shuffling DataLoader's does)."""

    def __init__(self, sampler: GpuPatchSampler, n_batches: int, batch_size: int, pairs, generator=None, augment: bool = True,
                 prefetch: int = 1):
        self.sampler, self.n_batches, self.batch_size = sampler, int(n_batches), int(batch_size)
        self.pairs, self.generator, self.augment, self.prefetch = pairs, generator, augment, prefetch
        self.dataset = range(self.n_batches * self.batch_size)       # len(loader.dataset), as the Trainer's shard checks read it
        self.drop_last = True

    def __len__(self):
        return self.n_batches

    def __iter__(self):
        return self.sampler.stream_batches(self.n_batches, self.batch_size, self.pairs, generator=self.generator,
                                           augment=self.augment, prefetch=self.prefetch)


def _check_channels(who, input_channels):
    """-> does the input carry image views?"""
    if input_channels not in ("geom",) + _VIEW_CHANNELS:
        raise ValueError(f"{who}: unknown input_channels {input_channels!r}")
    return input_channels in _VIEW_CHANNELS


def _check_shard(who, shard):
    rank, world = int(shard[0]), int(shard[1])
    if not 0 <= rank < world:
        raise ValueError(f"{who}: bad shard {shard!r}")
    return rank, world


def _check_image_pairs(who, sampler, image_pairs, where=""):
    """image_pairs as int lists: all of one length >= 1, every entry a plane of the sampler's orthos."""
    pairs = [[int(p) for p in pr] for pr in image_pairs]
    if len({len(p) for p in pairs}) != 1 or not pairs[0]:
        raise ValueError(f"{who}: every image pair must have the same number of views")
    n_planes = sampler.orthos.shape[0]
    if any(p < 0 or p >= n_planes for pr in pairs for p in pr):
        raise ValueError(f"{who}: an image index is outside the {n_planes} ortho planes{where}")
    return pairs


class GridTileSet:
    """`loader.dataset` of a GpuGridTiles: what predict_linear_blend and the Trainer read from a dataset (tile_size, stride,
    raster_shape, len(), `pos` in loader order, `shard` / `shard_plan`), plus the per-sample boxes and pair indices."""

    def __init__(self, tile_size, stride, raster_shape, pos, reg, pair_idx, shard, shard_plan, tta=None, tta_code=None,
                 tta_swap=None, n_pairs=None, image_pairs=None):
        self.tile_size, self.stride, self.raster_shape = int(tile_size), int(stride), tuple(raster_shape)
        self.pos, self.reg, self.pair_idx = pos, reg, pair_idx
        self.shard, self.shard_plan = shard, shard_plan
        # test-time augmentation (GpuGridTiles(tta=...)): `tta` = the variant codes -- every tile is len(tta) consecutive
        # samples --, tta_code / tta_swap = orientation code and view-swap flag of every sample.  All None without it.
        self.tta, self.tta_code, self.tta_swap = tta, tta_code, tta_swap
        # all pairs in one sweep (GpuGridTiles(sweep_pairs=True)): n_pairs = len(image_pairs), and pair_idx[i] is the plane of
        # sample i.  Both None without it (pair_idx is then all 0: a 'test' sweep reads pair 0).
        self.n_pairs, self.image_pairs = n_pairs, image_pairs

    def __len__(self):
        return len(self.pos)


class GpuGridTiles:
    """Validation / inference tiles (sampling_strategy 'val' / 'test' of the reference's DsmOrthoDataset, lib/DsmOrthoDataset.py:
    161-291 and 373-431) assembled on the GPU from the rasters a GpuPatchSampler keeps in HBM: the regular grid of
    `area_defn` (lib/rasterutils.py:100-191), per-tile DSM centring, ortho normalisation, target and the loss mask cut to each
    tile's non-overlap box, collated into device-resident batch dicts in the order and batching of
    DataLoader(dataset, batch_size, shuffle=False).  Takes the place of `utils.get_dataloader([dataset], sampling_strategy=
    'test' | 'val', ...)` for predict_linear_blend (test.py:170-189) and the Trainer's valloader (train.py:155-161); both take
    its batches as they are.  Batch k + 1 is assembled on a side stream while batch k is consumed (`prefetch`, as
    GpuPatchSampler.stream_batches).

    dsm_mean: None (or 0.0, the reference's `if not self.dsm_mean`) = each tile's mean over its input pixels != nodata; a
    tile whose input is all nodata gets NaN (0 / 0, as GpuPatchSampler).  The ortho mean / std and the DSM std are the
    sampler's.  shard=(rank, world): this rank's row band of a 'test' sweep (tiling.band_shards, as SyntheticRasterTiles).

    tta / tta_swap_views (strategy 'test' only): test-time augmentation of the sweep.  tta = "none", "flips", "d4" or a sequence
    of orientation codes (tiling.tta_codes: k | flip_v << 2 | flip_h << 3, the training loaders' transforms); tta_swap_views
    doubles the variants by showing the pair's views in reverse order (the reference's permute_images_within_pair; needs two
    or more views).  With a per-tile ortho mean (ortho_mean None) a swapped sample's mean is summed with the views in
    reverse order: fp64 sums of fp32 pixels, exact -- and so the plain tile's mean whatever the order -- as long as every non-zero
    pixel is at least 2^-29 of the tile's sum in magnitude (its last fp32 bit is then no finer than the sum's fp64 ulp); below
    that the two orders may differ by roundings of the fp64 sum, far under the fp32 rounding of the mean.  The sample list is this rank's plain list with every tile repeated once per variant, tile-major and
    variant-minor; `dataset` (pos, reg, pair_idx, len(), plus tta / tta_code / tta_swap) describes that list.  Batches carry the
    int32 device column "tta" (the orientation code of every sample), `input` in that orientation with the PLAIN tile's
    dsm_mean, and NO target / loss_mask: the variants are for prediction.  predict_linear_blend turns every prediction back
    and averages a tile's variants with the exact weight 1 / variants (rd_blend_accumulate_tta); the sweep costs variants x
    tiles forwards.  tta=None and tta_swap_views=False: the loader is what it was (rd_assemble_grid_tiles, no "tta" column).

    sweep_pairs (strategy 'test' only, an input with image views): every tile is repeated once per entry of `image_pairs`
    (1..16 of them), tile-major and pair-minor (tiling.pair_expand; with tta: tile, then pair, then variant), so ONE sweep
    predicts the raster from every pair -- ensemble.predict_pairs_linear_blend blends pair p into plane p and fuses the
    planes on the device.  Batches carry the int32 device column "pair" (the index into image_pairs = the plane of every
    sample) and, as under tta, NO target / loss_mask; `dataset` gains n_pairs and image_pairs, and its pair_idx is the
    column.  Not with shard of world > 1: the banded multi-GPU delivery is written for one plane.  False: the loader is what
    it was (pair 0 at every position, no "pair" column)."""

    def __init__(self, sampler: GpuPatchSampler, strategy: str, area_defn, input_channels: str = "geom-stereo",
                 image_pairs=None, stride=None, dsm_mean=None, transform_dsm: bool = True, transform_orthos: bool = True,
                 batch_size: int = 32, shard=(0, 1), prefetch: int = 1, augment: bool = False,
                 permute_images_within_pair: bool = False, tta=None, tta_swap_views: bool = False, sweep_pairs: bool = False):
        if augment:
            raise ValueError("GpuGridTiles: augment=True is not supported (the reference augments 'train' samples only)")
        if permute_images_within_pair:
            raise ValueError("GpuGridTiles: permute_images_within_pair=True is not supported")
        if not isinstance(sampler, GpuPatchSampler):
            raise ValueError("GpuGridTiles takes one GpuPatchSampler (multi-dataset ConcatDatasets are not supported)")
        views = _check_channels("GpuGridTiles", input_channels)
        rank, world = _check_shard("GpuGridTiles", shard)
        if strategy == "val" and world > 1:
            raise ValueError("GpuGridTiles: a sharded validation set is not supported")
        if strategy not in ("val", "test"):
            raise ValueError(f"GpuGridTiles: strategy must be 'val' or 'test' (got {strategy!r}); 'train' is SamplerLoader")
        if strategy == "val" and sampler.dsm_gt is None:
            raise ValueError("GpuGridTiles: strategy='val' needs the sampler's ground-truth raster")
        self.sweep_pairs = bool(sweep_pairs)
        if self.sweep_pairs:
            if strategy != "test":
                raise ValueError("GpuGridTiles: sweep_pairs is for strategy='test' (prediction); 'val' already reads every pair")
            if not views:
                raise ValueError(f"GpuGridTiles: sweep_pairs needs an input with image views (got input_channels={input_channels!r})")
            if image_pairs is not None and len(image_pairs) > tiling.MAX_SWEEP_PAIRS:
                raise ValueError(f"GpuGridTiles: sweep_pairs takes up to {tiling.MAX_SWEEP_PAIRS} image pairs (got {len(image_pairs)})")
            if world > 1:
                raise ValueError("GpuGridTiles: sweep_pairs with a shard of world > 1 is not supported (the banded multi-GPU "
                                 "delivery holds one plane)")
        self.source = sampler                 # not `.sampler`: predict_linear_blend reads that name as a torch sampler
        t = sampler.tile
        if t % 8:
            raise ValueError(f"GpuGridTiles: tile_size must be a multiple of 8 (got {t})")
        pairs = None
        if views:
            if sampler.orthos is None or not image_pairs:
                raise ValueError(f"GpuGridTiles: input_channels={input_channels!r} needs the sampler's orthos and image_pairs")
            pairs = _check_image_pairs("GpuGridTiles", sampler, image_pairs)
        self.strategy, self.input_channels = strategy, input_channels
        self.views = len(pairs[0]) if views else 0
        self.dsm_channel = 0 if input_channels == "stereo" else 1
        self.batch_size, self.prefetch = int(batch_size), int(prefetch)
        xe, ye = area_defn["x_extent"], area_defn["y_extent"]
        if len(xe) != len(ye):
            raise ValueError("GpuGridTiles: area_defn x_extent / y_extent differ in length")
        for (x0, x1), (y0, y1) in zip(xe, ye):
            if x0 < 0 or y0 < 0 or x1 >= sampler.w or y1 >= sampler.h or x1 - x0 + 1 < t or y1 - y0 + 1 < t:
                raise ValueError(f"GpuGridTiles: area x {x0}..{x1}, y {y0}..{y1} does not hold a {t} x {t} tile inside the "
                                 f"{sampler.h} x {sampler.w} raster")
        stride, pos, reg, pair_idx = tiling.grid_samples(xe, ye, t, strategy, stride, len(pairs) if views else 1, views)
        if not 0 < stride <= t:
            raise ValueError(f"GpuGridTiles: stride must be in 1..{t} (got {stride})")
        pos, reg, pair_idx, plan = tiling.grid_shard(strategy, pos, reg, pair_idx, t, sampler.h, (rank, world))
        extra = {}
        if self.sweep_pairs:
            pos, reg, pair_idx = tiling.pair_expand(pos, reg, len(pairs))
            extra = dict(n_pairs=len(pairs), image_pairs=[list(pr) for pr in pairs])
            if sampler.dsm_gt is not None and tta is None and not tta_swap_views:
                warnings.warn("GpuGridTiles: with sweep_pairs the batches carry no target / loss_mask (the sampler's ground "
                              "truth is not read); use a loader without it where a loss or a per-tile metric is needed",
                              stacklevel=2)
        self.tta = tta is not None or bool(tta_swap_views)
        if self.tta:
            if strategy != "test":
                raise ValueError("GpuGridTiles: tta is for strategy='test' (prediction); validation tiles keep one orientation")
            codes = tiling.tta_codes(tta, bool(tta_swap_views))
            if tta_swap_views and self.views < 2:
                raise ValueError("GpuGridTiles: tta_swap_views needs an image pair of two or more views")
            if sampler.dsm_gt is not None:
                warnings.warn("GpuGridTiles: with tta the batches carry no target / loss_mask (the sampler's ground truth is "
                              "not read); use a loader without tta where a loss or a per-tile metric is needed", stacklevel=2)
            pos, reg, pair_idx, code, swap, variants = tiling.tta_expand(pos, reg, pair_idx, codes, bool(tta_swap_views))
            rows6 = pair_idx
            if tta_swap_views:      # rows n_pairs .. 2 n_pairs - 1 of the pair -> plane table: the pairs with their views reversed
                rows6 = [p + len(pairs) * sw for p, sw in zip(pair_idx, swap)]
                pairs = pairs + [pr[::-1] for pr in pairs]
            self.dataset = GridTileSet(t, stride, (sampler.h, sampler.w), pos, reg, pair_idx, (rank, world), plan, variants,
                                       code, swap, **extra)
        else:
            rows6 = pair_idx
            self.dataset = GridTileSet(t, stride, (sampler.h, sampler.w), pos, reg, pair_idx, (rank, world), plan, **extra)
        # transform modes of rd_assemble_grid_tiles: 0 raw, 1 the given mean, 2 the tile's mean (`not mean`: the reference's test)
        self.dsm_mode, self.dsm_mean = _transform_mode(transform_dsm, dsm_mean)
        self.ortho_mode, self.ortho_mean = _transform_mode(transform_orthos, sampler.ortho_mean)
        dev = sampler.device
        n = len(pos)
        tab = torch.zeros(max(n, 1), 8, dtype=torch.int32)
        if n:
            tab[:n, 0:2] = torch.tensor(pos, dtype=torch.int32)
            tab[:n, 2:6] = torch.tensor(reg, dtype=torch.int32)
            tab[:n, 6] = torch.tensor(rows6, dtype=torch.int32)
        # uploaded once per loader: the kernels' sample table, the pair -> plane table and the int64 metadata columns
        self._table = tab.to(dev)
        self._pair_planes = torch.tensor(pairs, dtype=torch.int32).to(dev) if views else None
        self._aug = torch.tensor(self.dataset.tta_code, dtype=torch.int32).reshape(-1).to(dev) if self.tta else None
        self._pair = torch.tensor(pair_idx, dtype=torch.int32).reshape(-1).to(dev) if self.sweep_pairs else None
        self._meta = {k: tab[:n, c].to(torch.int64).to(dev) for c, k in enumerate(_META)}
        self.drop_last = False

    def __len__(self):
        return -(-len(self.dataset) // self.batch_size)

    def assemble(self, k0: int, k1: int, ws=None):
        """Samples [k0, k1) of this loader as one batch dict (device tensors), on the current stream."""
        with torch.cuda.device(self.source.device):      # raw launches go to the current device's stream
            return self._assemble(int(k0), int(k1), ws)

    def _assemble(self, k0, k1, ws):
        src, t, dev = self.source, self.source.tile, self.source.device
        if not 0 <= k0 < k1 <= len(self.dataset):
            raise ValueError(f"GpuGridTiles: sample range [{k0}, {k1}) outside 0..{len(self.dataset)}")
        n, v = k1 - k0, self.views
        c = self.dsm_channel + v
        inp = torch.empty(n, c, t, t, dtype=torch.float32, device=dev)
        mean = torch.empty(n, dtype=torch.float32, device=dev)
        tgt = msk = None
        # oriented samples and the samples of a pair sweep are for prediction: no target / loss_mask
        if src.dsm_gt is not None and not self.tta and not self.sweep_pairs:
            tgt = torch.empty(n, 1, t, t, dtype=torch.float32, device=dev)
            msk = torch.empty(n, 1, t, t, dtype=torch.uint8, device=dev)
        lib = load()
        need = lib.rd_assemble_grid_tiles_ws_bytes(n, t)
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
        head = (ptr(src.dsm_in), ptr(src.dsm_gt) if tgt is not None else None, ptr(src.orthos) if v else None,
                src.orthos.shape[0] if v else 0, src.h, src.w, self._table.data_ptr() + k0 * 8 * 4,
                ptr(self._pair_planes) if v else None, self._pair_planes.shape[0] if v else 0, v, self.dsm_channel, n, t,
                src.nodata, self.dsm_mode, self.dsm_mean, src.dsm_std, self.ortho_mode, self.ortho_mean, src.ortho_std)
        tail = (ptr(inp), ptr(tgt), ptr(msk), ptr(mean), ptr(ws), ws.numel(), stream_ptr())
        batch = {"input": inp, "dsm_mean": mean, "dsm_std": torch.full((n,), src.dsm_std, device=dev),
                 "nodata": torch.full((n,), src.nodata, device=dev)}
        if self.tta:        # the same arguments plus the orientation code of every sample
            batch["tta"] = self._aug[k0:k1]
            check(lib.rd_assemble_grid_tiles_aug(*head, ptr(batch["tta"]), *tail), "assemble_grid_tiles_aug")
        else:
            check(lib.rd_assemble_grid_tiles(*head, *tail), "assemble_grid_tiles")
        if self.sweep_pairs:
            batch["pair"] = self._pair[k0:k1]
        for key, col in self._meta.items():
            batch[key] = col[k0:k1]
        if tgt is not None:
            batch["target"], batch["loss_mask"] = tgt, msk.view(torch.bool)
        return batch

    def __iter__(self):
        src = self.source
        with torch.cuda.device(src.device):
            side = torch.cuda.Stream(device=src.device)
            with torch.cuda.stream(side):
                ws = torch.empty(load().rd_assemble_grid_tiles_ws_bytes(self.batch_size, src.tile), dtype=torch.uint8,
                                 device=src.device)
        yield from _prefetched(src.device, tiling.batch_bounds(len(self.dataset), self.batch_size),
                               lambda k: self._assemble(k[0], k[1], ws), self.prefetch, side)


_RASTER_DESC = [("dsm_in", "<u8"), ("dsm_gt", "<u8"), ("ortho", "<u8"), ("height", "<i4"), ("width", "<i4"), ("n_planes", "<i4"),
                ("nodata", "<f4"), ("dsm_std", "<f4"), ("ortho_mode", "<i4"), ("ortho_mean", "<f4"), ("ortho_std", "<f4"),
                ("reserved", "<i4", (2,))]          # rd_train_raster (include/resdepth_hip.h), 64 bytes
_SAMPLE_INTS = 8                                    # RD_TRAIN_SAMPLE_INTS
_TRAIN_AUG_BOX = 16                                 # RD_TRAIN_AUG_BOX


def _f32bits(v):
    return int(np.array(v, dtype=np.float32).view(np.int32))


def _check_loader_args(who, datasets, input_channels, batch_size, shard):
    """The checks GpuTrainSet and GpuValSet share -> datasets (a list), their samplers, views (does the input carry image
    views?), (rank, world)."""
    if isinstance(datasets, dict):
        datasets = [datasets]
    if not datasets:
        raise ValueError(f"{who}: no datasets")
    views = _check_channels(who, input_channels)
    if int(batch_size) < 1:
        raise ValueError(f"{who}: batch_size must be positive (got {batch_size})")
    shard = _check_shard(who, shard)
    samplers = [d.get("sampler") for d in datasets]
    if not all(isinstance(s, GpuPatchSampler) for s in samplers):
        raise ValueError(f"{who}: every dataset needs a GpuPatchSampler under 'sampler'")
    s0 = samplers[0]
    if s0.tile % 4 or s0.tile < 4:
        raise ValueError(f"{who}: tile_size must be a multiple of 4 (got {s0.tile})")
    if any(s.tile != s0.tile or s.device != s0.device for s in samplers):
        raise ValueError(f"{who}: the samplers must share tile size and device")
    if len({s.dsm_gt is None for s in samplers}) != 1:
        raise ValueError(f"{who}: either every sampler or none has a ground-truth raster")
    if len({s.weight is None for s in samplers}) != 1:
        raise ValueError(f"{who}: either every sampler or none has a weight raster")
    return datasets, samplers, views, shard


def _dataset_pairs(who, d, s, di, input_channels, n_views):
    """int32 [P, V] plane table of the image pairs of dataset di (an input with image views); V = n_views unless that is None."""
    if s.orthos is None or not d.get("image_pairs"):
        raise ValueError(f"{who}: input_channels={input_channels!r} needs orthos and image_pairs (dataset {di})")
    pairs = np.array(_check_image_pairs(who, s, d["image_pairs"], f" (dataset {di})"), dtype=np.int32)
    if n_views not in (None, pairs.shape[1]):
        raise ValueError(f"{who}: the datasets must share the number of views per sample")
    return pairs


def _raster_desc(samplers, views, transform_orthos, with_gt):
    """The rd_train_raster table of rd_assemble_train_patches, one row per sampler, as a numpy record array."""
    desc = np.zeros(len(samplers), dtype=_RASTER_DESC)
    for r, s in zip(desc, samplers):
        r["dsm_in"], r["dsm_gt"] = s.dsm_in.data_ptr(), (s.dsm_gt.data_ptr() if with_gt else 0)
        r["ortho"] = s.orthos.data_ptr() if views else 0
        r["height"], r["width"], r["n_planes"] = s.h, s.w, (s.orthos.shape[0] if views else 0)
        r["nodata"], r["dsm_std"], r["ortho_std"] = s.nodata, s.dsm_std, s.ortho_std
        r["ortho_mode"], r["ortho_mean"] = _transform_mode(transform_orthos, s.ortho_mean)
    return desc


_WEIGHT_DESC = [("plane", "<u8"), ("table", "<u8"), ("kind", "<i4"), ("height", "<i4"), ("width", "<i4"), ("reserved", "<i4")]
# rd_weight_raster (include/resdepth_hip_wloss.h), 32 bytes


def _weight_desc(samplers):
    """The rd_weight_raster table of rd_assemble_train_weights, one row per sampler in the order of _raster_desc, as a uint8
    device tensor; None when the samplers carry no weights."""
    s0 = samplers[0]
    if s0.weight is None:
        return None
    desc = np.zeros(len(samplers), dtype=_WEIGHT_DESC)
    for r, s in zip(desc, samplers):
        r["plane"], r["table"] = s.weight.data_ptr(), (s.weight_table.data_ptr() if s.weight_table is not None else 0)
        r["kind"], r["height"], r["width"] = s.weight_kind, s.h, s.w
    with torch.cuda.device(s0.device):
        return torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to(s0.device)


def _assemble_train(desc, n_rasters, tab, v, dsm_channel, t, with_gt, meta, wdesc=None):
    """One rd_assemble_train_patches launch on the current stream for the n samples of the device table `tab` (int32
    [rows, n]) -> the batch dict of GpuTrainSet and GpuValSet: dsm_std / nodata are views of the table, `meta` holds the
    caller's _META columns.  wdesc (the samplers' _weight_desc): one rd_assemble_train_weights launch over the same table adds
    `loss_weight` [n, 1, t, t]."""
    n, dev = tab.shape[1], tab.device
    inp = torch.empty(n, dsm_channel + v, t, t, dtype=torch.float32, device=dev)
    mean = torch.empty(n, dtype=torch.float32, device=dev)
    sums = torch.empty(n, 4, dtype=torch.float64, device=dev)
    tgt = msk = None
    if with_gt:
        tgt = torch.empty(n, 1, t, t, dtype=torch.float32, device=dev)
        msk = torch.empty(n, 1, t, t, dtype=torch.uint8, device=dev)
    check(load().rd_assemble_train_patches(ptr(desc), n_rasters, ptr(tab), n, v, dsm_channel, t, ptr(inp), ptr(tgt),
                                           ptr(msk), ptr(mean), ptr(sums), stream_ptr()), "assemble_train_patches")
    batch = {"input": inp, "dsm_mean": mean, "dsm_std": tab[6].view(torch.float32), "nodata": tab[7].view(torch.float32), **meta}
    if with_gt:
        batch["target"], batch["loss_mask"] = tgt, msk.view(torch.bool)
    if wdesc is not None:
        batch["loss_weight"] = ops.assemble_train_weights(wdesc, n_rasters, tab, v, t)
    return batch


class TrainSampleSet:
    """`loader.dataset` of a GpuTrainSet: len() = the samples this rank sees per epoch (what the Trainer's shard checks read),
    plus the whole sample list (dataset id, positions, pair indices) and the tile size."""

    def __init__(self, tile_size, dataset_id, pos, pair_idx, per_epoch):
        self.tile_size, self.dataset_id, self.pos, self.pair_idx = int(tile_size), dataset_id, pos, pair_idx
        self._per_epoch = int(per_epoch)

    def __len__(self):
        return self._per_epoch


class GpuTrainSet:
    """The training set of the reference (`utils.get_dataloader(cfg_traindata, sampling_strategy='train', ...)`, lib/utils.py:
    203-272, train.py:146-153) assembled on the GPU from rasters GpuPatchSamplers keep in HBM: per dataset a FIXED list of
    n_samples patch positions drawn once from its training areas, each bound to an image pair (lib/DsmOrthoDataset.py:316-371,
    tiling.draw_train_samples: the reference's rule and draw order from `rng`), the lists of several datasets concatenated
    (ConcatDataset), reshuffled every epoch (tiling.epoch_order), augmented per sample (rot90 / flips, lib/torch_transforms.py)
    and collated into device-resident batch dicts with the keys of the reference's 'train' sample (:281-291).  A batch may mix
    rasters: one rd_assemble_train_patches call per batch.  A `trainloader` for resdepth_amd.Trainer: len() = batches per epoch,
    `.dataset` has a len(), drop_last = False (a ragged last batch, as DataLoader), `batch_size`.

    datasets: [dict(sampler=GpuPatchSampler, area_defn=..., n_samples=..., image_pairs=...)] -- the samplers share tile size,
    device, view count and either all or none have a ground-truth raster; the DSM std, ortho mean / std and nodata are each
    sampler's own.  dsm_mean: None (or 0.0) = every patch's own mean.  generator: CPU torch.Generator of the epoch order, the
    augmentation draws (k, flip_v, flip_h) and the within-pair permutations (lib/DsmOrthoDataset.py:224-227); all of an epoch's
    draws are made when the epoch starts, so its batches do not depend on batch size or prefetch depth.  shard=(rank, world):
    this rank's samples of every epoch (equally many per rank).  Batch k + 1 is assembled on a side stream while batch k is
    consumed (`prefetch`, the hand-over of GpuPatchSampler.stream_batches)."""

    def __init__(self, datasets, input_channels: str, batch_size: int, use_all_stereo_pairs: bool = False,
                 permute_images_within_pair: bool = False, augment: bool = True, transform_dsm: bool = True,
                 transform_orthos: bool = True, dsm_mean=None, shuffle: bool = True, generator=None, rng=None, shard=(0, 1),
                 prefetch: int = 1):
        datasets, samplers, views, (rank, world) = _check_loader_args("GpuTrainSet", datasets, input_channels, batch_size, shard)
        s0 = samplers[0]
        t = s0.tile
        self.samplers, self.device, self.tile = samplers, s0.device, t
        self.has_gt = s0.dsm_gt is not None
        self.input_channels, self.batch_size, self.prefetch = input_channels, int(batch_size), int(prefetch)
        self.augment, self.permute, self.shuffle = bool(augment), bool(permute_images_within_pair), bool(shuffle)
        self.generator, self.shard = generator, (rank, world)
        self.dsm_channel = 0 if input_channels == "stereo" else 1
        dsm_mode, dsm_mean = _transform_mode(transform_dsm, dsm_mean)
        ids, poss, pidx, cols, planes = [], [], [], [], []
        n_views = None
        for di, (d, s) in enumerate(zip(datasets, samplers)):
            area = d["area_defn"]
            for (x0, x1), (y0, y1) in zip(area["x_extent"], area["y_extent"]):
                if x0 < 0 or y0 < 0 or x1 >= s.w or y1 >= s.h:
                    raise ValueError(f"GpuTrainSet: area x {x0}..{x1}, y {y0}..{y1} of dataset {di} is not inside the "
                                     f"{s.h} x {s.w} raster")
            if views:
                pairs = _dataset_pairs("GpuTrainSet", d, s, di, input_channels, n_views)
                n_views = pairs.shape[1]
            # the reference's draws, dataset after dataset (each DsmOrthoDataset constructor calls _determine_patches)
            pos, pi = tiling.draw_train_samples(area, t, d["n_samples"], input_channels, d.get("image_pairs"), use_all_stereo_pairs,
                                                rng)
            m = len(pos)
            ids.append(np.full(m, di, dtype=np.int64))
            poss.append(pos)
            pidx.append(pi)
            c = np.zeros((_SAMPLE_INTS, m), dtype=np.int32)
            c[0], c[1], c[2], c[4] = di, pos[:, 0], pos[:, 1], dsm_mode
            c[5] = _f32bits(dsm_mean)                                   # 0.0 (all bits 0) unless the mode is 1
            c[6], c[7] = _f32bits(s.dsm_std), _f32bits(s.nodata)        # the batch dict's per-sample dsm_std / nodata columns
            cols.append(c)
            if views:
                planes.append(pairs[pi])
        desc = _raster_desc(samplers, views, transform_orthos, self.has_gt)
        self._wdesc = _weight_desc(samplers)
        self.views = n_views or 0
        self._cols = np.concatenate(cols, axis=1)                                        # [8, m], static columns
        self._planes = np.concatenate(planes, axis=0) if views else np.zeros((self._cols.shape[1], 0), dtype=np.int32)
        self._ids, self._pos, self._pidx = np.concatenate(ids), np.concatenate(poss), np.concatenate(pidx)
        m = self._cols.shape[1]
        self.dataset = TrainSampleSet(t, self._ids, self._pos, self._pidx, (m // world) if world > 1 else m)
        self.drop_last = False
        with torch.cuda.device(self.device):
            self._desc = torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to(self.device)
        self._nan = {}

    def __len__(self):
        return -(-len(self.dataset) // self.batch_size)

    def sample_list(self):
        """(dataset id int64 [m], positions int64 [m, 2] (y, x), pair indices int64 [m]) of the whole set, in ConcatDataset order."""
        return self._ids, self._pos, self._pidx

    def table(self, index, aug=None, views=None):
        """Host sample table (int32 [8 + V, n], the column layout of rd_assemble_train_patches) for the samples `index` of the
        list; aug: int [n, 3] (k, flip_v, flip_h) or None; views: int [n, V] plane indices replacing the pairs' own order."""
        idx = np.asarray(index, dtype=np.int64).reshape(-1)
        tab = np.empty((_SAMPLE_INTS + self.views, idx.size), dtype=np.int32)
        tab[:_SAMPLE_INTS] = self._cols[:, idx]
        if self.views:
            tab[_SAMPLE_INTS:] = (self._planes[idx] if views is None else np.asarray(views, dtype=np.int32).reshape(idx.size, -1)).T
        if aug is not None:
            tab[3] = _aug_code(np.asarray(aug), idx.size)
        return tab

    def assemble(self, index, aug=None, views=None):
        """The samples `index` of the list as one batch dict (device tensors), on the current stream."""
        with torch.cuda.device(self.device):
            return self._assemble(torch.from_numpy(self.table(index, aug, views)))

    def _assemble(self, tab_host):
        n = tab_host.shape[1]
        tab = tab_host.to(self.device, non_blocking=True)
        nan = self._nan.get(n)
        if nan is None:
            nan = self._nan[n] = torch.full((n,), float("nan"), dtype=torch.float64, device=self.device)
        meta = dict(zip(_META, (tab[1].to(torch.int64), tab[2].to(torch.int64), nan, nan, nan, nan)))
        return _assemble_train(self._desc, len(self.samplers), tab, self.views, self.dsm_channel, self.tile, self.has_gt, meta,
                               self._wdesc)

    def epoch_tables(self):
        """One epoch's draws from `generator` -> [host sample table per batch] (pinned int32 [8 + V, n] each): the order
        (tiling.epoch_order), then the within-pair permutations, then k, flip_v, flip_h for every sample of the epoch."""
        g = self.generator
        order = tiling.epoch_order(self._cols.shape[1], g, self.shard, self.shuffle).numpy()
        n_e, v = order.size, self.views
        views = aug = None
        if self.permute and v > 1:
            perm = torch.argsort(torch.rand(n_e, v, generator=g), dim=1).numpy()
            views = np.take_along_axis(self._planes[order], perm, axis=1)
        if self.augment:
            aug = _draw_aug(n_e, g).numpy()
        tab = self.table(order, aug, views)
        rows = tab.shape[0]
        flat = torch.empty(max(tab.size, 1), dtype=torch.int32).pin_memory()
        out = []
        for k0, k1 in tiling.batch_bounds(n_e, self.batch_size):
            piece = flat[k0 * rows:k1 * rows].view(rows, k1 - k0)
            piece.copy_(torch.from_numpy(np.ascontiguousarray(tab[:, k0:k1])))
            out.append(piece)
        return out

    def __iter__(self):
        yield from _prefetched(self.device, self.epoch_tables(), self._assemble, self.prefetch)


class ValSampleSet:
    """`loader.dataset` of a GpuValSet: len() = the samples this rank reads per epoch (a replicated tail counted on every
    rank), and per such sample, in loader order, its dataset id, position, non-overlap box, pair index and its `index` in the
    ConcatDataset; `n_total` = the length of the whole list."""

    def __init__(self, tile_size, stride, index, dataset_id, pos, reg, pair_idx, n_total, shard):
        self.tile_size, self.stride, self.index = int(tile_size), int(stride), index
        self.dataset_id, self.pos, self.reg, self.pair_idx = dataset_id, pos, reg, pair_idx
        self.n_total, self.shard = int(n_total), shard

    def __len__(self):
        return len(self.index)


class GpuValSet:
    """The validation set of the reference (`utils.get_dataloader(cfg_valdata, 'val', ...)`, lib/utils.py:203-272, train.py:
    155-161: a ConcatDataset of one 'val' DsmOrthoDataset per entry, read with shuffle=False) assembled on the GPU from rasters
    GpuPatchSamplers keep in HBM: per dataset the regular grid of its areas with every image pair at every position
    (tiling.grid_samples), the lists concatenated (tiling.concat_val_samples), each tile's loss mask cut to its non-overlap box
    (lib/DsmOrthoDataset.py:434-470), collated into device-resident batch dicts with the keys and dtypes of GpuGridTiles in the
    order and batching of DataLoader(ConcatDataset, batch_size, shuffle=False), ragged last batch included.  A batch may
    straddle two rasters: one rd_assemble_train_patches call per batch (samples flagged RD_TRAIN_AUG_BOX).  A `valloader` for
    resdepth_amd.Trainer: len() = batches, `.dataset` has a len(), drop_last = False.

    datasets: [dict(sampler=GpuPatchSampler, area_defn=..., image_pairs=..., dsm_mean=None)] -- the samplers share tile size,
    device, view count and all have a ground-truth raster; the DSM std, ortho mean / std and nodata are each sampler's own.
    dsm_mean (per dataset): None (or 0.0) = every tile's own mean over its input pixels != nodata, an fp64 sum rounded once
    (the bits GpuTrainSet / GpuPatchSampler give the same tile).  shard=(rank, world): `batch_size` is the per-rank size and
    rank r reads its run of every global batch of batch_size * world samples (tiling.val_shard_batches); a last batch that
    world does not divide is read whole by every rank, which leaves the globally normalised loss the single-process one.
    The sample tables are uploaded once; batch k + 1 is assembled on a side stream while batch k is consumed (`prefetch`, the
    hand-over of GpuPatchSampler.stream_batches)."""

    def __init__(self, datasets, input_channels: str, batch_size: int, shard=(0, 1), prefetch: int = 1,
                 transform_dsm: bool = True, transform_orthos: bool = True, stride=None, augment: bool = False,
                 permute_images_within_pair: bool = False):
        if augment:
            raise ValueError("GpuValSet: augment=True is not supported (the reference augments 'train' samples only)")
        if permute_images_within_pair:
            raise ValueError("GpuValSet: permute_images_within_pair=True is not supported")
        datasets, samplers, views, self.shard = _check_loader_args("GpuValSet", datasets, input_channels, batch_size, shard)
        s0 = samplers[0]
        t = s0.tile
        if s0.dsm_gt is None:
            raise ValueError("GpuValSet: a validation set needs the samplers' ground-truth rasters")
        if stride is not None and not 0 < int(stride) <= t:
            raise ValueError(f"GpuValSet: stride must be in 1..{t} (got {stride})")
        self.samplers, self.device, self.tile = samplers, s0.device, t
        self.input_channels, self.batch_size, self.prefetch = input_channels, int(batch_size), int(prefetch)
        self.dsm_channel = 0 if input_channels == "stereo" else 1
        areas, pair_tabs = [], []
        n_views = None
        for di, (d, s) in enumerate(zip(datasets, samplers)):
            area = d["area_defn"]
            xe, ye = area["x_extent"], area["y_extent"]
            if len(xe) != len(ye):
                raise ValueError(f"GpuValSet: area_defn x_extent / y_extent differ in length (dataset {di})")
            for (x0, x1), (y0, y1) in zip(xe, ye):
                if x0 < 0 or y0 < 0 or x1 >= s.w or y1 >= s.h or x1 - x0 + 1 < t or y1 - y0 + 1 < t:
                    raise ValueError(f"GpuValSet: area x {x0}..{x1}, y {y0}..{y1} of dataset {di} does not hold a {t} x {t} "
                                     f"tile inside the {s.h} x {s.w} raster")
            pairs = None
            if views:
                pairs = _dataset_pairs("GpuValSet", d, s, di, input_channels, n_views)
                n_views = pairs.shape[1]
            areas.append((xe, ye, len(pairs) if views else 1))
            pair_tabs.append(pairs)
        desc = _raster_desc(samplers, views, transform_orthos, True)
        self._wdesc = _weight_desc(samplers)
        self.views = v = n_views or 0
        used_stride, ids, pos, reg, pidx = tiling.concat_val_samples(areas, t, stride, views)
        ids, pidx = np.array(ids, dtype=np.int64), np.array(pidx, dtype=np.int64)
        pos, reg = np.array(pos, dtype=np.int64).reshape(-1, 2), np.array(reg, dtype=np.int64).reshape(-1, 4)
        m = len(ids)
        # the whole list as the column table of rd_assemble_train_patches: 8 + V + 4 rows (box columns after the view planes)
        rows = _SAMPLE_INTS + v + 4
        cols = np.zeros((rows, m), dtype=np.int32)
        cols[0], cols[1], cols[2], cols[3] = ids, pos[:, 0], pos[:, 1], _TRAIN_AUG_BOX
        for di, (d, s) in enumerate(zip(datasets, samplers)):
            sel = ids == di
            mode, mean = _transform_mode(transform_dsm, d.get("dsm_mean"))
            cols[4, sel] = mode
            cols[5, sel] = _f32bits(mean)                               # 0.0 (all bits 0) unless the mode is 1
            cols[6, sel], cols[7, sel] = _f32bits(s.dsm_std), _f32bits(s.nodata)
            if views:
                cols[_SAMPLE_INTS:_SAMPLE_INTS + v, sel] = pair_tabs[di][pidx[sel]].T
        cols[_SAMPLE_INTS + v:] = reg.T
        # this rank's batches, each a contiguous [rows, n] piece of one flat device table (uploaded once)
        self._bounds = tiling.val_shard_batches(m, self.batch_size, self.shard)
        index = np.concatenate([np.arange(k0, k1) for k0, k1 in self._bounds]) if self._bounds else np.zeros(0, dtype=np.int64)
        flat = np.concatenate([np.ascontiguousarray(cols[:, k0:k1]).reshape(-1) for k0, k1 in self._bounds]) \
            if self._bounds else np.zeros(1, dtype=np.int32)
        self._rows = rows
        self._first = np.concatenate([[0], np.cumsum([k1 - k0 for k0, k1 in self._bounds])]).astype(np.int64)
        self.dataset = ValSampleSet(t, used_stride, index, ids[index], pos[index], reg[index], pidx[index], m, self.shard)
        self.drop_last = False
        meta = np.concatenate([pos[index], reg[index]], axis=1)                         # int64 [n_rank, 6]
        with torch.cuda.device(self.device):
            self._desc = torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to(self.device)
            self._table = torch.from_numpy(flat).to(self.device)
            self._meta = {k: torch.from_numpy(np.ascontiguousarray(meta[:, c])).to(self.device) for c, k in enumerate(_META)}

    def __len__(self):
        return len(self._bounds)

    def sample_list(self):
        """(dataset id int64 [n], positions int64 [n, 2] (y, x), boxes int64 [n, 4], pair indices int64 [n]) of this rank's
        samples in loader order."""
        ds = self.dataset
        return ds.dataset_id, ds.pos, ds.reg, ds.pair_idx

    def assemble(self, k: int):
        """Batch k of this loader as one batch dict (device tensors), on the current stream."""
        with torch.cuda.device(self.device):
            return self._assemble(int(k))

    def _assemble(self, k):
        if not 0 <= k < len(self._bounds):
            raise ValueError(f"GpuValSet: batch {k} outside 0..{len(self._bounds) - 1}")
        j0, j1 = int(self._first[k]), int(self._first[k + 1])
        tab = self._table[j0 * self._rows:j1 * self._rows].view(self._rows, j1 - j0)
        meta = {key: col[j0:j1] for key, col in self._meta.items()}
        return _assemble_train(self._desc, len(self.samplers), tab, self.views, self.dsm_channel, self.tile, True, meta,
                               self._wdesc)

    def __iter__(self):
        yield from _prefetched(self.device, range(len(self._bounds)), self._assemble, self.prefetch)
