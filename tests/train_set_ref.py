"""numpy stand-in for the reference's training set and its two normalisation statistics (TEST INFRASTRUCTURE ONLY): the
'train' sample list of DsmOrthoDataset._determine_patches (lib/DsmOrthoDataset.py:316-371, positions enumerated as
data_allocation.indices_from_area_defn does, lib/data_allocation.py:332-378), the 'train' sample dict of __getitem__
(:161-291; tests/grid_tiles_ref.py with the whole tile as the non-overlap box, plus view permutation and rot90 / flip
augmentation), compute_local_dsm_std_per_centered_patch (lib/utils.py:111-158) and compute_satellite_image_normalization
(lib/utils.py:161-200), both as fp64 two-pass reductions.  Pinned by tests/golden/g20_train.npz (the reference's own code);
the GPU tests use it on rasters too large for a fixture."""
import itertools

import numpy as np

import grid_tiles_ref as G


def position_list(area_defn, tile):
    """indices_from_area_defn by brute force: the list itself."""
    out = []
    for (x0, x1), (y0, y1) in zip(area_defn["x_extent"], area_defn["y_extent"]):
        for y in range(y0, y1 - tile + 2):
            for x in range(x0, x1 - tile + 2):
                out.append((y, x))
    return out


def sample_list(area_defn, tile, n_samples, channels, pairs, use_all, rng=np.random):
    """-> (positions [m, 2], pair indices [m]) with the reference's draws, from the explicit position list."""
    valid = position_list(area_defn, tile)
    indices = rng.choice(len(valid), n_samples, replace=False)
    if channels == "geom-stereo" and pairs is not None and len(pairs) > 1:
        if use_all:
            n = len(pairs)
            return (np.array([valid[i] for i in np.repeat(indices, n)], dtype=np.int64).reshape(-1, 2),
                    np.tile(np.arange(n, dtype=np.int64), n_samples))
        pos = np.array([valid[i] for i in indices], dtype=np.int64).reshape(-1, 2)
        return pos, np.asarray(rng.choice(len(pairs), n_samples, replace=True), dtype=np.int64)
    return np.array([valid[i] for i in indices], dtype=np.int64).reshape(-1, 2), np.zeros(n_samples, dtype=np.int64)


def augment(a, k, flip_v, flip_h):
    """rot90(k) -> flipud -> fliplr over the last two axes (lib/torch_transforms.py)."""
    a = np.rot90(a, int(k), axes=(-2, -1))
    if flip_v:
        a = a[..., ::-1, :]
    if flip_h:
        a = a[..., :, ::-1]
    return np.ascontiguousarray(a)


def train_sample(dsm_in, dsm_gt, orthos_hwv, pos, views, tile, nodata, dsm_std, ortho_mean, ortho_std, channels, dsm_mean=None,
                 transform_dsm=True, transform_orthos=True, aug=None):
    """One 'train' sample: {"input", "target", "loss_mask", "dsm_mean"}; views = the plane indices in the order used."""
    s = G.grid_sample(dsm_in, dsm_gt, orthos_hwv, pos, (0, 0, tile - 1, tile - 1), views, tile, nodata, dsm_std, ortho_mean,
                      ortho_std, channels, dsm_mean=dsm_mean, transform_dsm=transform_dsm, transform_orthos=transform_orthos)
    if aug is not None:
        for k in ("input", "target", "loss_mask"):
            if s[k] is not None:
                s[k] = augment(s[k], *aug)
    return s


def patch_moments(plane, positions, tile, nodata=None):
    """fp64 two-pass (count, mean, M2) per patch over the pixels != nodata (all pixels for nodata None) -> [n, 3]."""
    out = np.zeros((len(positions), 3))
    for i, (y, x) in enumerate(np.asarray(positions).reshape(-1, 2)):
        v = plane[y:y + tile, x:x + tile]
        v = (v[v != np.float32(nodata)] if nodata is not None else v.reshape(-1)).astype(np.float64)
        mean = v.sum() / v.size if v.size else np.nan
        out[i] = v.size, mean, ((v - mean) ** 2).sum() if v.size else np.nan
    return out


def patch_stds(plane, positions, tile, nodata):
    m = patch_moments(plane, positions, tile, nodata)
    return np.sqrt(m[:, 2] / (m[:, 0] - 1.0))


def patch_stds_naive(plane, positions, tile, nodata):
    """The formulation the kernels must NOT use: sqrt((sum x^2 - (sum x)^2 / n) / (n - 1)) in fp64."""
    out = np.zeros(len(positions))
    for i, (y, x) in enumerate(np.asarray(positions).reshape(-1, 2)):
        v = plane[y:y + tile, x:x + tile]
        v = v[v != np.float32(nodata)].astype(np.float64)
        out[i] = np.sqrt(((v * v).sum() - v.sum() ** 2 / v.size) / (v.size - 1))
    return out


def trimmed_mean(stds):
    """lib/utils.py:152-156."""
    stds = np.asarray(stds, dtype=np.float64)
    p95, p5 = np.percentile(stds, 95), np.percentile(stds, 5)
    return stds[np.logical_and(stds >= p5, stds <= p95)].mean().item()


def local_dsm_std(groups, tile, nodata):
    """groups = [(plane, positions)] -> (trimmed mean, per-sample stds in group order)."""
    stds = np.concatenate([patch_stds(p, pos, tile, nodata) for p, pos in groups])
    return trimmed_mean(stds), stds


def image_normalization(groups):
    """groups = [(orthos [H, W, V], image_pairs, area_defn)] -> (mean, population std), fp64 two-pass over the concatenation."""
    data = []
    for orthos, pairs, area in groups:
        for idx in sorted(set(itertools.chain(*pairs))):
            for (x0, x1), (y0, y1) in zip(area["x_extent"], area["y_extent"]):
                data.append(orthos[y0:y1 + 1, x0:x1 + 1, idx].reshape(-1).astype(np.float64))
    data = np.concatenate(data)
    mean = data.sum() / data.size
    return float(mean), float(np.sqrt(((data - mean) ** 2).sum() / data.size))
