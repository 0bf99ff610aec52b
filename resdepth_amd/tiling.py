"""Regular (overlapping) tile grids for tiled inference -- the index arithmetic of the reference's
`create_regular_grid` (lib/rasterutils.py:100-191): stride T/2 by default for inference
(lib/DsmOrthoDataset.py:99-100), last row / column shifted inwards to end on the region border, plus the
per-tile "region without overlap" box that drives the linear blend weights."""
from __future__ import annotations

from typing import List, Sequence, Tuple


def _axis(lo: int, hi: int, tile: int, stride: int):
    """1-D sweep over the inclusive range [lo, hi] -> [(start, border_lo, border_hi)]."""
    out = []
    start, end = lo, lo
    b_lo, b_hi = 0, stride - 1
    while end < hi:
        end = start + tile - 1
        s, bl, bh = start, b_lo, b_hi
        if end >= hi:                       # shift the last tile inwards
            bl = b_lo + (end - hi)
            end = hi
            s = hi - tile + 1
            bh = tile - 1
        out.append((s, bl, bh))
        start = s + stride if s == start else start + stride
        b_lo = tile - stride
    return out


def regular_grid(x_extent: Sequence[Tuple[int, int]], y_extent: Sequence[Tuple[int, int]], tile_size: int,
                 stride: int | None = None):
    """-> (positions [(uly, ulx)], regions [(border_uly, border_ulx, border_lry, border_lrx)]), row-major per stripe."""
    stride = tile_size if stride is None else stride
    pos: List[Tuple[int, int]] = []
    reg: List[Tuple[int, int, int, int]] = []
    for (x0, x1), (y0, y1) in zip(x_extent, y_extent):
        cols = _axis(int(x0), int(x1), tile_size, stride)
        for (uly, b_uly, b_lry) in _axis(int(y0), int(y1), tile_size, stride):
            for (ulx, b_ulx, b_lrx) in cols:
                pos.append((uly, ulx))
                reg.append((b_uly, b_ulx, b_lry, b_lrx))
    return pos, reg


def band_shards(pos: Sequence[Tuple[int, int]], tile_size: int, rows: int, world: int):
    """Shard a sweep's tile list (in sweep order, `regular_grid`) over `world` ranks by ROW BANDS: contiguous
    chunks cut at tile-row boundaries, balanced by tile count.  A rank's tiles then touch only the raster rows
    [y0, y1) of its band (+ the T - stride rows it shares with each neighbour), so its private raster is band-sized, the
    exchange is the shared rows only, and every rank reads ITS rows back to the host.

    -> list of `world` dicts: tiles [i0, i1) of `pos`; extent [y0, y1) = raster rows the rank's tiles touch; owned [c0, c1) =
    the rows the rank delivers (the cuts c partition [0, rows): c_r = y0 of rank r's first tile, c_0 = 0, c_world = rows);
    lo / hi = the rows its private raster covers = [min(c0, y0), max(c1, y1)).  Ranks beyond the number of tile rows get an
    empty range.  `monotonic` (same on every entry) says whether the cuts are non-decreasing -- false for tile lists whose
    areas go back up the raster, which the caller then sweeps with full-size rasters + a reduce instead."""
    n = len(pos)
    starts = [i for i in range(n) if i == 0 or pos[i][0] != pos[i - 1][0]] + [n]       # first tile of every tile row
    groups = len(starts) - 1
    cuts_i = [0]
    for r in range(1, world):
        # boundary (a tile-row start) whose tile count is closest to the r-th equal share, at least one tile row per rank
        target = n * r / world
        lo_g = min(groups, r)                               # rank r-1 keeps at least one row
        cand = range(max(lo_g, 0), groups + 1)
        best = min(cand, key=lambda g: (abs(starts[g] - target), g)) if groups else 0
        best = max(best, starts.index(cuts_i[-1]) + (1 if cuts_i[-1] < n else 0)) if groups else 0
        cuts_i.append(starts[min(best, groups)])
    cuts_i.append(n)
    out = []
    for r in range(world):
        i0, i1 = cuts_i[r], cuts_i[r + 1]
        ys = [pos[i][0] for i in range(i0, i1)]
        out.append({"i0": i0, "i1": i1, "y0": min(ys) if ys else None, "y1": (max(ys) + tile_size) if ys else None})
    # ownership cuts: rank r starts owning at its first tile's row; empty ranks own nothing (cut = the next non-empty one's)
    c = [0] * (world + 1)
    c[world] = rows
    for r in range(world - 1, 0, -1):
        c[r] = out[r]["y0"] if out[r]["y0"] is not None else c[r + 1]
    mono = all(c[r] <= c[r + 1] for r in range(world))
    for r in range(world):
        e = out[r]
        e["c0"], e["c1"] = c[r], c[r + 1]
        e["lo"] = min(e["c0"], e["y0"]) if e["y0"] is not None else e["c0"]
        e["hi"] = max(e["c1"], e["y1"]) if e["y1"] is not None else e["c1"]
        e["monotonic"] = mono
    return out


def grid_samples(x_extent: Sequence[Tuple[int, int]], y_extent: Sequence[Tuple[int, int]], tile_size: int, strategy: str,
                 stride: int | None = None, n_pairs: int = 1, views: bool = True):
    """Sample order of the reference's `_determine_patches` for sampling_strategy 'val' / 'test' (lib/DsmOrthoDataset.py:373-431)
    -> (stride, positions [(uly, ulx)], boxes [(b_uly, b_ulx, b_lry, b_lrx)], pair indices), one entry per sample.
    stride None: T/2 for 'test', T for 'val' (:99-104).  'val' with image views (`views`, every input_channels but 'geom')
    evaluates every pair at every position, pair-major: sample k = (position k % P, pair k // P) for P grid positions.
    'val' without views and 'test' take the positions once, with pair 0."""
    if strategy not in ("val", "test"):
        raise ValueError(f"strategy must be 'val' or 'test' (got {strategy!r})")
    if stride is None:
        stride = int(tile_size * 0.5) if strategy == "test" else int(tile_size)
    pos, reg = regular_grid(x_extent, y_extent, tile_size, stride)
    if strategy == "val" and views:
        n = int(n_pairs)
        return stride, pos * n, reg * n, [k for k in range(n) for _ in pos]
    return stride, pos, reg, [0] * len(pos)


def batch_bounds(n: int, batch_size: int):
    """[(k0, k1)] of a DataLoader(batch_size=..., drop_last=False) over n samples in order (the last batch may be ragged)."""
    return [(k, min(k + int(batch_size), n)) for k in range(0, n, int(batch_size))]


def concat_val_samples(areas, tile_size: int, stride: int | None = None, views: bool = True):
    """Sample list of ConcatDataset([DsmOrthoDataset(d, sampling_strategy='val') ...]) (lib/utils.py:256-270): the
    `grid_samples(..., 'val', ...)` lists of the datasets one after the other.  areas: [(x_extent, y_extent, n_pairs)] per
    dataset -> (stride, dataset ids, positions, boxes, pair indices), one entry per sample; a pair index counts within its own
    dataset's pair list."""
    ids, pos, reg, pair_idx = [], [], [], []
    used = int(tile_size) if stride is None else int(stride)
    for di, (xe, ye, n_pairs) in enumerate(areas):
        used, p, r, pi = grid_samples(xe, ye, tile_size, "val", stride, n_pairs, views)
        ids += [di] * len(p)
        pos += p
        reg += r
        pair_idx += pi
    return used, ids, pos, reg, pair_idx


def val_shard_batches(n: int, batch_size: int, shard=(0, 1)):
    """[(k0, k1)] of rank `shard[0]` of `shard[1]` over a validation list of n samples read in order (shuffle=False,
    drop_last=False), one entry per batch.  `batch_size` is the PER-RANK size b: a global batch is B = b * world consecutive
    samples and every rank has ceil(n / B) batches.  Of a full global batch k, rank r takes the contiguous run
    [k B + r b, k B + (r + 1) b).  A last batch of R = n mod B samples is split evenly (R / world each, in rank order) when
    world divides R; otherwise EVERY rank takes the whole last batch.

    Why replicate: under the global loss normaliser (GradSync.allreduce_loss_sums, which also assumes equal per-rank batch
    sizes through numel * world) a replicated batch has both sum |d| and sum mask multiplied by world, so its loss is the
    single-process one.  The batch grouping of the reference's meter (one loss per global batch, averaged over batches) is
    kept, no rank idles and no collective is skipped.  world = 1 gives `batch_bounds`."""
    rank, world = int(shard[0]), int(shard[1])
    if not 0 <= rank < world:
        raise ValueError(f"bad shard {tuple(shard)!r}")
    n, b = int(n), int(batch_size)
    if b < 1:
        raise ValueError(f"batch_size must be positive (got {batch_size})")
    big = b * world
    out = [(k + rank * b, k + (rank + 1) * b) for k in range(0, n - n % big, big)]
    rest = n % big
    if rest:
        k = n - rest
        if rest % world == 0:
            out.append((k + rank * (rest // world), k + (rank + 1) * (rest // world)))
        else:
            out.append((k, n))
    return out


def grid_shard(strategy: str, pos, reg, pair_idx, tile_size: int, rows: int, shard=(0, 1)):
    """This rank's samples of a `grid_samples` list -> (pos, reg, pair_idx, shard_plan).  'test' sweeps are cut into row bands
    (`band_shards`, the plan SyntheticRasterTiles keeps); a sharded 'val' set is refused."""
    rank, world = int(shard[0]), int(shard[1])
    if not 0 <= rank < world:
        raise ValueError(f"bad shard {tuple(shard)!r}")
    if strategy != "test":
        if world > 1:
            raise ValueError("a sharded validation set is not supported")
        return list(pos), list(reg), list(pair_idx), None
    plan = band_shards(pos, tile_size, rows, world)
    i0, i1 = plan[rank]["i0"], plan[rank]["i1"]
    return list(pos[i0:i1]), list(reg[i0:i1]), list(pair_idx[i0:i1]), plan


# ---- test-time augmentation: variants of a tile under the square's symmetry group ----------------------------------------
# A code is the training loaders' aug = k | flip_v << 2 | flip_h << 3: rot90(k) -> flipud -> fliplr (lib/torch_transforms.py).
TTA_SETS = {"none": (0,), "flips": (0, 4, 8, 12), "d4": tuple(k | (h << 3) for k in range(4) for h in (0, 1))}


def tta_codes(spec, swap_views: bool = False):
    """Variant codes of a test-time-augmentation set -> tuple of ints in 0..15.  spec: None / "none" = (0,); "flips" = identity,
    flipud, fliplr, both; "d4" = the eight elements of the square's symmetry group (k = 0..3, each without and with fliplr, in
    that order); or an explicit sequence of codes.  The number of variants (doubled by `swap_views`) must be 1, 2, 4, 8 or 16:
    the blend weighs every variant by 1 / variants, which is exact -- and commutes with every rounding -- for powers of two only."""
    if spec is None:
        codes = TTA_SETS["none"]
    elif isinstance(spec, str):
        if spec not in TTA_SETS:
            raise ValueError(f"tta must be one of {sorted(TTA_SETS)} or a sequence of codes (got {spec!r})")
        codes = TTA_SETS[spec]
    else:
        try:
            codes = tuple(spec)
        except TypeError:
            raise ValueError(f"tta must be one of {sorted(TTA_SETS)} or a sequence of codes (got {spec!r})") from None
        for c in codes:
            if isinstance(c, bool) or int(c) != c or not 0 <= int(c) <= 15:
                raise ValueError(f"tta codes are integers in 0..15 (k | flip_v << 2 | flip_h << 3), got {c!r}")
        codes = tuple(int(c) for c in codes)
    n = len(codes) * (2 if swap_views else 1)
    if n not in (1, 2, 4, 8, 16):
        raise ValueError(f"the number of tta variants must be 1, 2, 4, 8 or 16 (got {n})")
    return codes


def tta_apply(x, code: int):
    """The oriented form of a numpy array [..., T, T] under `code`: rot90(k) -> flipud -> fliplr on the last two axes."""
    import numpy as np
    code = int(code)
    y = np.rot90(x, code & 3, axes=(-2, -1))
    if code & 4:
        y = np.flip(y, -2)
    if code & 8:
        y = np.flip(y, -1)
    return np.ascontiguousarray(y)


def tta_undo(y, code: int):
    """Inverse of `tta_apply`: fliplr -> flipud -> rot90(-k)."""
    import numpy as np
    code = int(code)
    x = y
    if code & 8:
        x = np.flip(x, -1)
    if code & 4:
        x = np.flip(x, -2)
    return np.ascontiguousarray(np.rot90(x, -(code & 3), axes=(-2, -1)))


def tta_expand(pos, reg, pair_idx, codes, swap_views: bool = False):
    """A sample list with every tile repeated once per variant, tile-major and variant-minor -> (pos, reg, pair_idx, code per
    sample, view-swap flag per sample, the variant codes).  The variants are `codes`, then (swap_views) `codes` again with the
    pair's views in reverse order.  Applied AFTER grid_shard: a tile's variants stay on the tile's rank and next to each other,
    so the band plan, the frontier bookkeeping of predict_linear_blend and the per-pixel blend order see G samples where they
    saw one."""
    variants = [(c, 0) for c in codes] + ([(c, 1) for c in codes] if swap_views else [])
    g = len(variants)
    rep = lambda xs: [x for x in xs for _ in range(g)]
    n = len(pos)
    return (rep(pos), rep(reg), rep(pair_idx), [c for c, _ in variants] * n, [s for _, s in variants] * n,
            tuple(c for c, _ in variants))


# ---- all image pairs of a raster in one sweep ---------------------------------------------------------------------------
MAX_SWEEP_PAIRS = 16        # rd_fuse_planes reduces up to 16 planes per pixel


def pair_expand(pos, reg, n_pairs: int):
    """A 'test' sample list with every tile repeated once per image pair, tile-major and pair-minor -> (pos, reg, pair index
    per sample).  The idea of `tta_expand`: a tile's n_pairs samples are neighbours, so its DSM tile is hot in cache when the
    next pair reads it, and the band plan and the frontier bookkeeping of the sweep see n_pairs samples where they saw one.
    Applied AFTER grid_shard and BEFORE tta_expand: with test-time augmentation the order is tile-major, then pair, then
    variant-minor.  The pair index is the plane of the sample in a one-pass sweep (ensemble.predict_pairs_linear_blend)."""
    n_pairs = int(n_pairs)
    if n_pairs < 1:
        raise ValueError(f"pair_expand: n_pairs must be positive (got {n_pairs})")
    rep = lambda xs: [x for x in xs for _ in range(n_pairs)]
    return rep(pos), rep(reg), list(range(n_pairs)) * len(pos)


# ---- the training set: sampling_strategy 'train' of the reference's `_determine_patches` (lib/DsmOrthoDataset.py:316-371) ----
def _train_regions(area_defn, tile_size: int):
    """[(y_start, x_start, n_y, n_x)] per region of `area_defn`: the valid upper-left positions of
    data_allocation.indices_from_area_defn (lib/data_allocation.py:332-378) -- inclusive extents, every position keeps the
    tile inside its region."""
    xe, ye = area_defn["x_extent"], area_defn["y_extent"]
    if len(xe) != len(ye):
        raise ValueError("area_defn x_extent / y_extent differ in length")
    out = []
    for (x0, x1), (y0, y1) in zip(xe, ye):
        nx, ny = int(x1) - int(tile_size) + 1 - int(x0) + 1, int(y1) - int(tile_size) + 1 - int(y0) + 1
        if nx <= 0 or ny <= 0:
            raise ValueError(f"area x {x0}..{x1}, y {y0}..{y1} does not hold a {tile_size} x {tile_size} tile")
        out.append((int(y0), int(x0), ny, nx))
    return out


def train_position_count(area_defn, tile_size: int) -> int:
    """len(indices_from_area_defn(area_defn, tile_size)) without building the list (6e7 entries for an 8192^2 raster)."""
    return sum(ny * nx for _, _, ny, nx in _train_regions(area_defn, tile_size))


def train_position(area_defn, tile_size: int, index):
    """indices_from_area_defn(area_defn, tile_size)[index] for an int or an integer array `index` -> (y, x) or int64 [m, 2]:
    regions in order, then y outer, x inner."""
    import numpy as np
    regions = _train_regions(area_defn, tile_size)
    idx = np.asarray(index, dtype=np.int64)
    flat = idx.reshape(-1)
    total = sum(ny * nx for _, _, ny, nx in regions)
    if flat.size and (flat.min() < 0 or flat.max() >= total):
        raise IndexError(f"train position index outside 0..{total - 1}")
    out = np.zeros((flat.size, 2), dtype=np.int64)
    first = 0
    for y0, x0, ny, nx in regions:
        sel = (flat >= first) & (flat < first + ny * nx)
        k = flat[sel] - first
        out[sel, 0] = y0 + k // nx
        out[sel, 1] = x0 + k % nx
        first += ny * nx
    return (int(out[0, 0]), int(out[0, 1])) if idx.ndim == 0 else out


def draw_train_samples(area_defn, tile_size: int, n_samples: int, input_channels: str, image_pairs=None,
                       use_all_stereo_pairs: bool = False, rng=None):
    """The sample list of a 'train' DsmOrthoDataset (lib/DsmOrthoDataset.py:316-371) -> (positions int64 [m, 2] (y, x), pair
    indices int64 [m]) with the reference's rule AND draw order: `rng.choice(count, n_samples, replace=False)` for the
    positions; only for 'geom-stereo' with more than one pair either every position repeated per pair (use_all_stereo_pairs:
    m = n_samples * pairs, pair indices 0..P-1 tiled) or `rng.choice(P, n_samples, replace=True)`; every other channel mode
    gets pair 0 throughout, even with several pairs listed (as the reference).  rng: np.random (default) or a RandomState --
    after the same np.random.seed the list is the reference's."""
    import numpy as np
    rng = np.random if rng is None else rng
    count = train_position_count(area_defn, tile_size)
    n_samples = int(n_samples)
    if not 0 < n_samples <= count:
        raise ValueError(f"n_samples must be in 1..{count} (the valid patch positions of the area), got {n_samples}")
    indices = rng.choice(count, n_samples, replace=False)
    n_pairs = len(image_pairs) if image_pairs else 0
    if input_channels == "geom-stereo" and n_pairs > 1:
        if use_all_stereo_pairs:
            indices = np.repeat(indices, n_pairs)
            pair_idx = np.tile(np.arange(n_pairs, dtype=np.int64), n_samples)
        else:
            pair_idx = np.asarray(rng.choice(n_pairs, n_samples, replace=True), dtype=np.int64)
    else:
        pair_idx = np.zeros(n_samples, dtype=np.int64)
    return train_position(area_defn, tile_size, indices), pair_idx


def epoch_order(n: int, generator=None, shard=(0, 1), shuffle: bool = True):
    """Sample order of one epoch for rank `shard[0]` of `shard[1]`: torch.randperm(n, generator) (the DataLoader's
    RandomSampler; shuffle=False: 0..n-1), for world > 1 cut to a multiple of world, rank r taking order[r::world] -- every
    rank gets equally many samples (the Trainer's ragged-batch check needs equal last batches)."""
    import torch
    rank, world = int(shard[0]), int(shard[1])
    if not 0 <= rank < world:
        raise ValueError(f"bad shard {tuple(shard)!r}")
    order = torch.randperm(int(n), generator=generator) if shuffle else torch.arange(int(n))
    if world > 1:
        order = order[:(int(n) // world) * world][rank::world]
    return order
