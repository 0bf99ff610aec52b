/*
 * resdepth_hip_loss.h -- masked, de-normalised training losses beyond L1: entry points of libresdepth_hip.so
 * (rd_version >= 114), included by resdepth_hip.h; its conventions (device pointers, stream, return codes, memory contract,
 * alignment) hold here.
 *
 * Kept apart from resdepth_hip.h for the reason resdepth_hip_pairs.h is: the coverage ledger over the main header
 * (tests/test_memory_contract_gpu.py) describes exactly the entry points its case table drives.  The guard-band cases of the
 * entry points below, and a ledger over THIS header, are in tests/test_loss_contract_gpu.py.
 *
 * The reference's Trainer._compute_denormalized_loss (lib/Trainer.py:87-100) zeroes the masked pixels of both de-normalised
 * tensors, applies whatever criterion it was given and rescales by numel / sum(mask).  rd_masked_l1_* (resdepth_hip.h) is that
 * chain for nn.L1Loss; the pair below is the chain for a quadratic or a Huber data term, with an optional term on the first
 * differences of the residual, and reports the masked mean absolute error next to the loss.
 *
 * Arithmetic.  For sample n and pixel e of an [N][H][W] batch (one channel):
 *     p = fl(fl(yp * std_n) + mean_n)      t = fl(fl(y * std_n) + mean_n)      r = fl(p - t)          (fp32, as rd_masked_l1_*)
 *     m = (mask[e] != 0)
 * Everything that follows r is fp64.  Five sums over the batch:
 *     C = sum m                                    A = sum m |r|
 *     D = sum m rho(r), rho by `kind`:
 *         RD_LOSS_L1     scale * |r|
 *         RD_LOSS_L2     scale * r^2
 *         RD_LOSS_HUBER  scale * (|r| <= delta ? r^2 / 2 : delta * (|r| - delta / 2))
 *       (scale = 1 for nn.L1Loss / nn.MSELoss / nn.HuberLoss(delta); scale = 1 / beta with delta = beta for nn.SmoothL1Loss)
 *     S = sum |fl(r_a - r_b)| over the valid neighbour pairs (the difference is ONE fp32 subtraction), Q = their number:
 *       a horizontal pair is (i, j), (i, j + 1), a vertical pair (i, j), (i + 1, j); both pixels lie in the same sample, both
 *       have m = 1; a pair never crosses a sample boundary and never wraps a row.
 *     loss = D / C + (lambda > 0 && Q > 0 ? lambda * S / Q : 0)          mae = A / C
 *     dyp[e] = gout * std_n * (m * rho'(r) / C + (lambda / Q) * k(e))
 *       k(e) = integer sum of sign(r_e - r_other) over the valid pairs that contain e (-4 .. 4), formed as an integer and
 *       multiplied once; the slope part is exactly 0 when lambda == 0 or Q == 0; a masked pixel gets exactly 0.
 * Tie rules: sign(0) = 0 everywhere -- rho'(0) = 0 for RD_LOSS_L1, a flat neighbour pair adds 0 to k; |r| == delta takes the
 * quadratic branch (both branches agree there in value and slope).  C == 0: loss and mae are NaN (0 / 0) and dyp is all zeros,
 * what rd_masked_l1_finish gives.
 *
 * Schedule.  A block owns tiles of RD_LOSS_STRIP_ROWS x RD_LOSS_STRIP_COLS pixels, each inside ONE sample, and stages r and m
 * of the tile plus a one-pixel halo in LDS once; neighbours are read from there.  At most RD_LOSS_MAX_BLOCKS blocks walk the
 * tiles in a fixed order, a block's threads add their pixels in a fixed order, one block adds the per-block sums in block
 * order: no floating-point atomics, the same bits run to run.  Q and C are counted in integers (exact).
 * Alignment rule: when W % 4 == 0 and yp, y (dyp) are 16-byte aligned and mask is 4-byte aligned, a tile's interior is read
 * as float4 / one 4-byte mask word per four pixels and dyp is written as float4; otherwise every access is one element wide.
 * Both forms give the same bits.  H * W and N * H * W must be below 2^31.
 */
#ifndef RESDEPTH_HIP_LOSS_H
#define RESDEPTH_HIP_LOSS_H

#ifdef __cplusplus
extern "C" {
#endif

#define RD_LOSS_L1 0
#define RD_LOSS_L2 1
#define RD_LOSS_HUBER 2

/* tile of one block and the cap of the grid (a block takes tiles b, b + grid, ...) */
#define RD_LOSS_STRIP_ROWS 32
#define RD_LOSS_STRIP_COLS 64
#define RD_LOSS_MAX_BLOCKS 1024

/* bytes of scratch rd_masked_loss_partial needs for an [n][h][w] batch (per-block sums, fp64) */
size_t rd_masked_loss_ws_bytes(int n, int h, int w);

/* sums[0..7] (fp64, device) = A, C, D, S, Q, 0, 0, 0 of the batch (all eight are written: a data-parallel caller all-reduces
 * the whole array).  yp, y: [n][h][w] fp32; mask: [n][h][w] uint8 (torch.bool); mean, std: [n] fp32.  One pass over yp, y and
 * mask (9 bytes per pixel), two launches: masked_loss_partial_kernel<vector?, false> and masked_loss_reduce_kernel<5>.  A scratch smaller
 * than rd_masked_loss_ws_bytes(n, h, w) is refused (RD_ERR_WS) with nothing launched.  delta > 0 is required for
 * RD_LOSS_HUBER only. */
int rd_masked_loss_partial(const float* yp, const float* y, const uint8_t* mask, const float* mean, const float* std,
                           double* sums, int n, int h, int w, int kind, double delta, double scale, void* ws,
                           size_t ws_bytes, rd_stream_t s);

/* From sums (after any all-reduce): loss[0] and mae[0] (fp32, one rounding of the fp64 value) and dyp [n][h][w], each
 * nullable.  gout_dev: the upstream gradient as a DEVICE scalar (NULL = 1).  numel_total is the global element count; the
 * data term divides by C directly, so it does not enter the result (it is accepted so that the call mirrors
 * rd_masked_l1_finish and a caller may check it: it must be > 0).  One launch: masked_loss_finish_kernel<vector?, slope?, false>;
 * with lambda == 0 no halo is staged and the kernel streams 13 bytes per pixel; with dyp == NULL one block runs.
 * Nothing outside loss[0], mae[0] and the n * h * w floats of dyp is written. */
int rd_masked_loss_finish(const float* yp, const float* y, const uint8_t* mask, const float* mean, const float* std,
                          const double* sums, double numel_total, int kind, double delta, double scale, double lambda,
                          const float* gout_dev, float* loss, float* mae, float* dyp, int n, int h, int w, rd_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* RESDEPTH_HIP_LOSS_H */
