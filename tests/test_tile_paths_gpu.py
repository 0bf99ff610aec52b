"""The tile data path's assemblers against each other at ragged cell edges (-m gpu): rd_assemble_patches,
rd_assemble_train_patches, rd_assemble_grid_tiles and rd_assemble_grid_tiles_aug cut the same pixels through one orientation
map and one normalise / mask block (csrc/rd_tile_dev.h), so for the same position, code and means their planes are the same
bits -- for all sixteen codes, at T = 8 (the smallest grid tile), T = 40 (a full 32-cell of the oriented blend plus a ragged 8)
and T = 72 (a full 64-cell of the oriented grid tiles plus a ragged 8, two row blocks of the training assembler), at a
position with x % 4 == 0 (16-byte loads) and one with x odd (4-byte loads).  Everything is bit for bit: no tolerance."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NODATA = -9999.0
PLANES = (2, 0)                            # the two views of every sample: planes of the three-plane ortho stack
POS = ((1, 4), (3, 7))                     # (y, x): 16-byte aligned rows, and rows that are not
DSM_MEAN, DSM_STD, ORTHO_MEAN, ORTHO_STD = 3.25, 1.7, 101.5, 37.0
CODES = list(range(16))


def _t_apply(x, code):
    y = torch.rot90(x, code & 3, (-2, -1))
    if code & 4:
        y = torch.flip(y, (-2,))
    if code & 8:
        y = torch.flip(y, (-1,))
    return y.contiguous()


def _t_undo(y, code):
    if code & 8:
        y = torch.flip(y, (-1,))
    if code & 4:
        y = torch.flip(y, (-2,))
    return torch.rot90(y, -(code & 3), (-2, -1)).contiguous()


def _same(a, b):
    """bit for bit (NaN payloads included)"""
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def _sampler(T, ortho_mean):
    """a raster a few pixels larger than the tile (W a multiple of 4), zeros and nodata planted in both DSMs"""
    from resdepth_amd import GpuPatchSampler
    g = torch.Generator().manual_seed(100 + T)
    H, W = T + 5, T + 12
    dsm_in = torch.randn(H, W, generator=g) * 4 + 3
    dsm_gt = torch.randn(H, W, generator=g) * 4 + 3
    orthos = torch.rand(3, H, W, generator=g) * 255
    for r, k in ((dsm_in, 0), (dsm_gt, 1)):
        flat = r.view(-1)
        flat[torch.randperm(H * W, generator=g)[:H * W // 7]] = NODATA
        flat[torch.randperm(H * W, generator=g)[:H * W // 9]] = 0.0
        r[k + 2, :] = NODATA                        # a whole row, and the tile's corner pixels
        r[POS[0][0], POS[0][1]] = 0.0
        r[POS[1][0] + T - 1, POS[1][1] + T - 1] = NODATA
    return GpuPatchSampler(dsm_in, dsm_gt, orthos, tile_size=T, nodata=NODATA, dsm_std=DSM_STD, ortho_mean=ortho_mean,
                           ortho_std=ORTHO_STD, device=DEV)


def _samples():
    """every code at both positions -> positions [n, 2], codes [n]"""
    pos = [p for p in POS for _ in CODES]
    return pos, CODES * len(POS)


def _train(s, T, pos, codes, dsm_mode, box=None):
    """rd_assemble_train_patches on one raster: the column table of GpuTrainSet (box: flagged samples with that box)"""
    from resdepth_amd import sampler as S
    n, v = len(pos), len(PLANES)
    tab = np.zeros((S._SAMPLE_INTS + v + (4 if box else 0), n), dtype=np.int32)
    tab[1], tab[2] = [p[0] for p in pos], [p[1] for p in pos]
    tab[3] = [c | (S._TRAIN_AUG_BOX if box else 0) for c in codes]
    tab[4], tab[5], tab[6], tab[7] = dsm_mode, S._f32bits(DSM_MEAN), S._f32bits(DSM_STD), S._f32bits(NODATA)
    for j, p in enumerate(PLANES):
        tab[S._SAMPLE_INTS + j] = p
    if box:
        for j, b in enumerate(box):
            tab[S._SAMPLE_INTS + v + j] = b
    desc = S._raster_desc([s], True, True, True)
    desc = torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to(DEV)
    return S._assemble_train(desc, 1, torch.from_numpy(tab).to(DEV), v, 1, T, True, {})


def _patches(s, T, pos, codes):
    """rd_assemble_patches with the fixed means"""
    from resdepth_amd._lib import check, load, ptr, stream_ptr
    n, v = len(pos), len(PLANES)
    pos_t = torch.tensor(pos, dtype=torch.int32, device=DEV)
    aug = torch.tensor(codes, dtype=torch.int32, device=DEV)
    pair = torch.tensor([PLANES] * n, dtype=torch.int32, device=DEV)
    dmean, omean = torch.full((n,), DSM_MEAN, device=DEV), torch.full((n,), ORTHO_MEAN, device=DEV)
    inp = torch.empty(n, 1 + v, T, T, device=DEV)
    tgt, msk = torch.empty(n, 1, T, T, device=DEV), torch.empty(n, 1, T, T, dtype=torch.uint8, device=DEV)
    check(load().rd_assemble_patches(ptr(s.dsm_in), ptr(s.dsm_gt), ptr(s.orthos), s.h * s.w, ptr(pair), v, ptr(pos_t), ptr(aug),
                                     ptr(dmean), DSM_STD, ptr(omean), ORTHO_STD, NODATA, n, T, s.w, ptr(inp), ptr(tgt), ptr(msk),
                                     stream_ptr()), "assemble_patches")
    return inp, tgt, msk


def _grid(s, T, pos, codes=None, box=None):
    """rd_assemble_grid_tiles (codes None: with target and mask) / rd_assemble_grid_tiles_aug, fixed means"""
    from resdepth_amd._lib import check, load, ptr, stream_ptr
    n, v = len(pos), len(PLANES)
    tab = torch.tensor([[y, x, *(box or (0, 0, T - 1, T - 1)), 0, 0] for y, x in pos], dtype=torch.int32, device=DEV)
    pair_planes = torch.tensor([PLANES], dtype=torch.int32, device=DEV)
    inp, mean = torch.empty(n, 1 + v, T, T, device=DEV), torch.empty(n, device=DEV)
    lib = load()
    ws = torch.empty(max(lib.rd_assemble_grid_tiles_ws_bytes(n, T), 16), dtype=torch.uint8, device=DEV)
    head = (ptr(s.dsm_in), ptr(s.dsm_gt) if codes is None else None, ptr(s.orthos), 3, s.h, s.w, ptr(tab), ptr(pair_planes), 1, v, 1,
            n, T, NODATA, 1, DSM_MEAN, DSM_STD, 1, ORTHO_MEAN, ORTHO_STD)
    if codes is None:
        tgt, msk = torch.empty(n, 1, T, T, device=DEV), torch.empty(n, 1, T, T, dtype=torch.uint8, device=DEV)
        check(lib.rd_assemble_grid_tiles(*head, ptr(inp), ptr(tgt), ptr(msk), ptr(mean), ptr(ws), ws.numel(), stream_ptr()),
              "assemble_grid_tiles")
        return inp, tgt, msk
    aug = torch.tensor(codes, dtype=torch.int32, device=DEV)
    check(lib.rd_assemble_grid_tiles_aug(*head, ptr(aug), ptr(inp), None, None, ptr(mean), ptr(ws), ws.numel(), stream_ptr()),
          "assemble_grid_tiles_aug")
    return inp, None, None


@pytest.mark.parametrize("T", [8, 40, 72])
def test_three_assemblers_and_torch_agree_for_every_code(T):
    s = _sampler(T, ORTHO_MEAN)
    pos, codes = _samples()
    plain, _, _ = _grid(s, T, list(POS))                       # code 0 of both positions
    want = torch.stack([_t_apply(plain[i // 16], c) for i, c in enumerate(codes)])
    assert not torch.isnan(want).any()
    a, a_tgt, a_msk = _patches(s, T, pos, codes)
    b = _train(s, T, pos, codes, dsm_mode=1)
    c, _, _ = _grid(s, T, pos, codes)
    for i, code in enumerate(codes):
        assert _same(a[i], want[i]), ("rd_assemble_patches", pos[i], code)
        assert _same(b["input"][i], want[i]), ("rd_assemble_train_patches", pos[i], code)
        assert _same(c[i], want[i]), ("rd_assemble_grid_tiles_aug", pos[i], code)
    # the two training assemblers' target and mask, oriented as well
    assert _same(b["target"], a_tgt) and _same(b["loss_mask"].view(torch.uint8), a_msk)
    assert 0 < int(a_msk.sum()) < a_msk.numel()


@pytest.mark.parametrize("T", [8, 40, 72])
def test_target_and_mask_of_a_boxed_tile_agree(T):
    s = _sampler(T, ORTHO_MEAN)
    box = (2, 3, T - 3, T - 2)                                   # inclusive, no edge on a multiple of 4
    inp, tgt, msk = _grid(s, T, list(POS), box=box)
    b = _train(s, T, list(POS), [0, 0], dsm_mode=1, box=box)
    assert _same(b["input"], inp) and _same(b["target"], tgt) and _same(b["loss_mask"].view(torch.uint8), msk)
    m = msk[:, 0].bool()
    inside = torch.zeros(T, T, dtype=torch.bool, device=DEV)
    inside[box[0]:box[2] + 1, box[1]:box[3] + 1] = True
    gt = torch.stack([s.dsm_gt[y:y + T, x:x + T] for y, x in POS])
    assert torch.equal(m, inside & (gt != 0) & (gt != NODATA)) and m.any() and not m[:, inside].all()


@pytest.mark.parametrize("T", [8, 40, 72])
def test_computed_means_agree(T):
    """mode 2: rd_assemble_patches fed rd_patch_sums' sums (GpuPatchSampler.sample) and rd_assemble_train_patches"""
    s = _sampler(T, None)
    pos, codes = _samples()
    aug = [[c & 3, (c >> 2) & 1, (c >> 3) & 1] for c in codes]
    a = s.sample(pos, [PLANES] * len(pos), aug)
    b = _train(s, T, pos, codes, dsm_mode=2)
    assert torch.isfinite(a["dsm_mean"]).all() and _same(b["dsm_mean"], a["dsm_mean"])
    assert _same(b["input"], a["input"]) and _same(b["target"], a["target"])
    assert _same(b["loss_mask"].view(torch.uint8), a["loss_mask"].view(torch.uint8))


def test_oriented_blend_is_the_plain_blend_of_unrotated_predictions():
    from resdepth_amd import ops
    T, stride, codes = 40, 24, (0, 5, 11)
    g = torch.Generator().manual_seed(7)
    pred = torch.randn(3, T, T, generator=g)
    plain = torch.stack([_t_undo(pred[j], c) for j, c in enumerate(codes)]).to(DEV)
    mean, std = torch.tensor([1.5, -2.25, 0.75], device=DEV), torch.tensor([1.7, 0.9, 2.3], device=DEV)
    pos = torch.tensor([[0, 0], [8, 17], [20, 30]], dtype=torch.int32, device=DEV)        # all three overlap; the last is cut
    reg = torch.tensor([[0, 0, T - 1, T - 1], [16, 16, T - 1, T - 1], [16, 0, 23, 23]], dtype=torch.int32, device=DEV)
    base = torch.randn(57, 67, generator=g, dtype=torch.float64).to(DEV)
    want = ops.blend_accumulate(plain, mean, std, pos, reg, T, stride, base.clone())
    got = ops.blend_accumulate(pred.to(DEV), mean, std, pos, reg, T, stride, base.clone(),
                               aug=torch.tensor(codes, dtype=torch.int32, device=DEV))
    assert _same(got, want) and not torch.equal(want, base)
