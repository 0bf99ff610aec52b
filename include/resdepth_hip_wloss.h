/*
 * resdepth_hip_wloss.h -- per-pixel weights for the masked training losses, and the weight tiles of a training batch cut from
 * rasters resident in HBM: entry points of libresdepth_hip.so (detected by symbol; rd_version is unchanged), included by
 * resdepth_hip.h; its conventions (device pointers, stream, return codes, memory contract, alignment) hold here.
 *
 * Kept apart from resdepth_hip.h for the reason resdepth_hip_loss.h is: the coverage ledger over the main header
 * (tests/test_memory_contract_gpu.py) describes exactly the entry points its case table drives.  The guard-band cases of the
 * entry points below, and a ledger over THIS header, are in tests/test_wloss_contract_gpu.py.
 *
 * Arithmetic.  All notation is that of resdepth_hip_loss.h: r is the same three fp32 operations, m = (mask[e] != 0), everything
 * after r is fp64.  A weight plane w is [N][H][W] fp32; the caller guarantees it finite and >= 0, the kernels do not test it.
 * The batch sums, in the same eight-slot fp64 array (a data-parallel caller still all-reduces one array):
 *     sums[0]  A  = sum m |r|                          UNWEIGHTED
 *     sums[1]  C  = sum m
 *     sums[2]  D  = sum m w rho(r)                     (times scale, as rd_masked_loss_partial)
 *     sums[3]  S  = sum omega |fl(r_a - r_b)|          over the valid neighbour pairs (the rule of resdepth_hip_loss.h),
 *                                                      omega = ((double)w_a + (double)w_b) * 0.5 (exact in fp64)
 *     sums[4]  Q  = sum omega
 *     sums[5]  Wc = sum m w
 *     sums[6], sums[7] = 0
 *     loss = D / Wc + (lambda > 0 && Q > 0 ? lambda * S / Q : 0)          mae = A / C  (the plain masked MAE, on purpose: it is
 *       the logged and selected metric, and runs trained with different weights stay comparable)
 *     dyp[e] = gout * std_n * (m * w_e * rho'(r_e) / Wc + (lambda / Q) * K(e))
 *       K(e) = sum omega * sign(r_e - r_other) over the valid pairs that contain e, in fp64, added in the order left, right,
 *       upper, lower neighbour; the slope part is exactly 0 when lambda == 0 or Q == 0.
 * Tie rules as resdepth_hip_loss.h.  A masked pixel gets exactly 0; a pixel with w = 0 gets exactly 0 from the data term.
 * Wc == 0: loss is NaN (0 / 0) and dyp is all zeros, what C == 0 gives rd_masked_loss_finish; mae is NaN only when C == 0.
 *
 * With w == 1 everywhere the calls below give THE BITS of rd_masked_loss_partial / _finish for every kind and lambda: the
 * kernels are the same templates, every extra operation is a multiplication by 1.0 at the same place of the same summation
 * order, and Q, Wc are then sums of ones (exact).
 *
 * Schedule: that of resdepth_hip_loss.h (tiles of RD_LOSS_STRIP_ROWS x RD_LOSS_STRIP_COLS, at most RD_LOSS_MAX_BLOCKS blocks,
 * fixed-order reductions, no floating-point atomics: the same bits run to run); w is staged in LDS beside r and m, cells
 * outside the sample with w = 0.  Alignment rule: the vector path of resdepth_hip_loss.h needs `weight` 16-byte aligned as
 * well; otherwise every access is one element wide.  Both forms give the same bits.
 */
#ifndef RESDEPTH_HIP_WLOSS_H
#define RESDEPTH_HIP_WLOSS_H

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of scratch rd_weighted_loss_partial needs for an [n][h][w] batch (per-block sums, fp64: six per block) */
size_t rd_weighted_loss_ws_bytes(int n, int h, int w);

/* sums[0..7] (fp64, device) as above (all eight are written).  yp, y, weight: [n][h][w] fp32; mask: [n][h][w] uint8; mean, std:
 * [n] fp32.  kind: RD_LOSS_L1 / _L2 / _HUBER (RD_LOSS_L1 with lambda = 0 included: there is no weighted rd_masked_l1_*).  One
 * pass over yp, y, mask and weight (13 bytes per pixel), two launches: masked_loss_partial_kernel<vector?, true> and
 * masked_loss_reduce_kernel<6>.  A scratch smaller than rd_weighted_loss_ws_bytes(n, h, w) is refused (RD_ERR_WS) with nothing
 * launched.  Memory: reads the four planes, mean, std; writes the scratch and the eight doubles of sums, and nothing else. */
int rd_weighted_loss_partial(const float* yp, const float* y, const uint8_t* mask, const float* weight, const float* mean,
                             const float* std, double* sums, int n, int h, int w, int kind, double delta, double scale, void* ws,
                             size_t ws_bytes, rd_stream_t s);

/* From sums (after any all-reduce): loss[0], mae[0] (fp32, one rounding of the fp64 value) and dyp [n][h][w], each nullable.
 * gout_dev: the upstream gradient as a DEVICE scalar (NULL = 1).  numel_total > 0 is accepted as rd_masked_loss_finish accepts
 * it.  One launch: masked_loss_finish_kernel<vector?, slope?, true>; with lambda == 0 no halo is staged and the kernel streams
 * 17 bytes per pixel; with dyp == NULL one block runs.  No scratch.  Nothing outside loss[0], mae[0] and the n * h * w floats
 * of dyp is written. */
int rd_weighted_loss_finish(const float* yp, const float* y, const uint8_t* mask, const float* weight, const float* mean,
                            const float* std, const double* sums, double numel_total, int kind, double delta, double scale,
                            double lambda, const float* gout_dev, float* loss, float* mae, float* dyp, int n, int h, int w,
                            rd_stream_t s);

/* ---- weight tiles of a training batch ---------------------------------------------------------------------------------- */
/* One weight raster per rd_train_raster of the batch's rd_assemble_train_patches call, in the same order.
 * kind RD_WEIGHT_F32: plane = height x width fp32 weights, table unused.
 * kind RD_WEIGHT_CLASS_U8: plane = height x width uint8 classes, table = RD_WEIGHT_TABLE floats (the weight of class c at
 * table[c]; a shorter table is padded by the caller), looked up in the kernel: 1 byte per pixel of HBM instead of 4. */
#define RD_WEIGHT_F32 0
#define RD_WEIGHT_CLASS_U8 1
#define RD_WEIGHT_TABLE 256
typedef struct rd_weight_raster {
    const void* plane;
    const float* table;
    int kind, height, width;
    int reserved;
} rd_weight_raster; /* 32 bytes */

/* out [n][1][tile][tile] fp32 = the weight tile of every sample of the SAME device sample table rd_assemble_train_patches takes
 * (samples[col * n + i]; `views` is that call's, the table's further columns are not read): the tile x tile window at columns
 * 1-2 (y, x) of raster column 0, oriented by column 3 (k | flip_v << 2 | flip_h << 3) through rd::aug_src of rd_tile_dev.h --
 * the helper the target plane goes through, so weight and target cannot disagree.  RD_TRAIN_AUG_BOX does not alter weights (the
 * mask already carries the box).  A sample with a raster id outside 0..n_rasters-1, a window outside its raster, a null plane,
 * an unknown kind or (RD_WEIGHT_CLASS_U8) a null table yields NaN and reads nothing.  A row that is neither rotated nor mirrored
 * left-right is read with one 16-byte load per four pixels (4-byte for classes) when width % 4 == 0 and the window's first
 * element is so aligned -- the conditions of train_patch_write; otherwise element by element.  Same bits either way.
 * rasters: DEVICE table of n_rasters descriptors.  tile: a multiple of 4, at most 1024; out 16-byte aligned.  One launch:
 * train_weight_write.  No scratch.  Memory: reads the descriptors, columns 0-3 of the table and the windows; writes the
 * n * tile * tile floats of out, and nothing else. */
int rd_assemble_train_weights(const rd_weight_raster* rasters, int n_rasters, const int* samples, int n, int views, int tile,
                              float* out, rd_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* RESDEPTH_HIP_WLOSS_H */
