/*
 * resdepth_hip_tta.h -- test-time augmentation entry points of libresdepth_hip.so (rd_version >= 111), included by
 * resdepth_hip.h; its conventions (device pointers, stream, return codes, memory contract, alignment) hold here.
 *
 * Kept apart from resdepth_hip.h so that the coverage ledger over that header (tests/test_memory_contract_gpu.py) keeps
 * describing exactly the entry points its case table drives; the guard-band cases of the two entry points below, and a ledger
 * over THIS header, are in tests/test_tta_contract_gpu.py.
 * TO FOLD BACK: this split follows from where the tests live, not from the interface.  The next change that may edit
 * tests/test_memory_contract_gpu.py moves the two declarations into resdepth_hip.h, _lib.SIGNATURES_TTA into _lib.SIGNATURES
 * and the two case builders of tests/test_tta_contract_gpu.py into that file's table, and deletes this header.  Add no further
 * entry point here: the main ledger does not see this file, and a consumer that parses resdepth_hip.h without following its
 * includes misses what is declared here.
 *
 * The reference trains under the symmetry group of the square (lib/torch_transforms.py: Rotate, RandomVerticalFlip,
 * RandomHorizontalFlip) and predicts every tile in one orientation (lib/evaluation.py:460-513).  These two entry points let
 * the sweep show the net each tile in several orientations and average the predictions: a code is
 * aug = k | flip_v << 2 | flip_h << 3 = rot90(k) -> flipud -> fliplr, as rd_assemble_patches.
 */
#ifndef RESDEPTH_HIP_TTA_H
#define RESDEPTH_HIP_TTA_H

#ifdef __cplusplus
extern "C" {
#endif

/* rd_blend_accumulate for predictions of oriented tiles, averaged over 2^log2_variants variants.  For every sample i, in
 * sample order per raster pixel (rd_blend_accumulate's order; no atomics; launches of up to 64 samples, in order):
 *   raster[y_i + r][x_i + c] = fma((double)(float)(P_i[r][c] * std[i] + mean[i]) * 2^-log2_variants, w_i(r, c), raster[..])
 * -- ONE rounding per sample and pixel, a fused multiply-add, which is how rd_blend_accumulate's `+= (double)den * w` compiles
 * (v_fmac_f64 under -ffp-contract=on; the blend tests compare the two entry points bit for bit and fail if either changes).
 * P_i = pred[i] with the inverse of aug[i] applied (fliplr -> flipud -> rot90(-k)): the prediction in the raster's
 * orientation.  aug: int32 [n], only the low four bits are read; NULL = all 0.  w_i, pos, reg, the float de-normalisation
 * and the bounds rule (pixels outside rows x cols are skipped) are rd_blend_accumulate's.  log2_variants in 0..4.  The extra
 * factor is a power of two, so it scales the product exactly and commutes with the rounding (no value here is near the
 * subnormal range):
 * aug all 0 and log2_variants 0 give rd_blend_accumulate's bits, and in general the result is 2^-log2_variants times what
 * rd_blend_accumulate adds for the un-oriented predictions, bit for bit.  Kernel: blend_tta_kernel (32 x 32 raster cells;
 * the matching rectangle of pred[i] goes through LDS, so prediction reads are 128-B runs in every orientation). */
int rd_blend_accumulate_tta(const float* pred, const float* mean, const float* std, const int* pos, const int* reg,
                            const int* aug, int n, int tile_size, int stride, int log2_variants, double* raster, int rows,
                            int cols, rd_stream_t s);

/* rd_assemble_grid_tiles with an orientation per sample, for prediction: input[i] = the tile rd_assemble_grid_tiles writes for
 * samples[i], oriented by aug[i] (int32 [n], device, low four bits; NULL = all 0).  The tile means are the same fixed-order
 * fp64 sums over the untransformed pixels and every pixel takes the same sub / div, so an oriented tile is the permutation of
 * the plain one bit for bit (NaN mean of an all-nodata tile, NaN tile of a sample outside the raster included);
 * dsm_mean_out[i] is the plain tile's.  target and mask must be NULL (RD_ERR_ARG otherwise); dsm_gt is not read.  Every
 * other argument, the workspace (rd_assemble_grid_tiles_ws_bytes) and the alignment are rd_assemble_grid_tiles'.  Kernels:
 * grid_tile_sums (mode 2 only), grid_tile_write_aug (64 x 64 cells of the output tile; the matching raster rectangle goes
 * through LDS, so raster reads and tile writes are 256-B runs in every orientation). */
int rd_assemble_grid_tiles_aug(const float* dsm_in, const float* dsm_gt, const float* ortho_planes, int n_planes, int height,
                               int width, const int* samples, const int* pair_planes, int n_pairs, int views, int dsm_channel,
                               int n, int tile, float nodata, int dsm_mode, float dsm_mean, float dsm_std, int ortho_mode,
                               float ortho_mean, float ortho_std, const int* aug, float* input, float* target, uint8_t* mask,
                               float* dsm_mean_out, void* ws, size_t ws_bytes, rd_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* RESDEPTH_HIP_TTA_H */
