/*
 * resdepth_hip_tail.h -- the skip term of the last convolution taken in level 0's BatchNorm / activation / max-pool pass: two
 * entry points of libresdepth_hip.so, included by resdepth_hip.h; its conventions (device pointers, stream, return codes, memory
 * contract, magnitude slots through rd_quant_next) hold here.
 *
 * A side header for the reason resdepth_hip_optim.h is: the coverage ledger over the main header
 * (tests/test_memory_contract_gpu.py) describes exactly the entry points its case table drives.  The guard-band cases of the
 * two entry points below and a ledger over THIS header are in tests/test_tail_fold_contract_gpu.py; bindings:
 * resdepth_amd/_lib.py SIGNATURES_TAIL; front end: resdepth_amd/ops.py bn_act_pool_fwd_tailskip, conv3x3_last_fwd_tail_pre;
 * user: UNet.fold_tail_skip (resdepth_amd/unet.py).
 *
 * What they replace.  In the forward of the composed tail (rd_conv3x3_last_fwd_tail in resdepth_hip.h), level 0's pre-BN tensor
 * z [N, H, W, C] -- the largest tensor of the step -- is read twice, and both readers evaluate the same act(BN(z)) per element:
 * rd_bn_act_pool_fwd right after the first convolution (lib/UNet.py:45,29-31,161: BatchNorm, activation, MaxPool2d(2)) and
 * rd_conv3x3_last_fwd_tail at the very end (lib/UNet.py:227-244: skip add, last convolution, outer residual).  The skip part of
 * the last convolution, conv_last(act(BN(z))), depends on z, the batch statistics and the last layer's weight only, and all
 * three exist when the first reader runs.  So the first reader emits it as a ONE-channel tensor skip9 [N, H, W] and the second
 * read of z is gone.  The pair gives the bits of that pair -- pooled, idx and zpool of the first, out of the second:
 * the arithmetic, its order and its association are those kernels'.
 */
#ifndef RESDEPTH_HIP_TAIL_H
#define RESDEPTH_HIP_TAIL_H

#ifdef __cplusplus
extern "C" {
#endif

/* rd_bn_act_pool_fwd in its pooled form without the full-resolution activation (a = NULL there), plus the skip term.
 *   y = fmaf(z, invstd * gamma, beta - mean * (invstd * gamma));  act = y > 0 ? y : y * slope   (slope_dev, nullable: a
 *   1-element device tensor that overrides `slope` -- nn.PReLU().weight)
 *   pooled / idx / zpool (nullable) [N, H/2, W/2, C]: the 2 x 2 maximum of act with torch's rule (the first maximum wins, a NaN
 *   wins), its position 0..3 (row-major in the window) and z at that position;
 *   skip9[n][y][x] = sum_tap sum_c act[n][y + tap / 3 - 1][x + tap % 3 - 1][c] * w_last[c][tap], act = 0 outside the image: per
 *   pixel and tap the products over a group of 8 consecutive channels as one fmaf chain, the C / 8 groups by a fixed pairwise
 *   tree, the taps in order 0..8 from 0.f.
 * w_last: the last convolution's weight [1, C, 3, 3].  The magnitude slot registered as out2 by rd_quant_next receives
 * max |pooled| -- one commit per 16 x 32 image tile instead of one per element range, so the slot's words hold the same
 * maximum, spread differently over its sixteen lines.
 * C in {16, 32, 64}; H and W even; H * W * C * 4 < 2^31.  Anything else is refused (RD_ERR_ARG) with nothing written.
 * Memory: reads z[0 .. N*H*W*C), the four BN vectors [C], w_last[0 .. 9*C), slope_dev[0]; writes pooled, idx (bytes) and zpool
 * [0 .. N*H/2*W/2*C), skip9[0 .. N*H*W), the words 0 and 1 of the sixteen lines of the out2 slot, and nothing else.  No scratch.
 * Kernel: bn_act_pool_tailskip_kernel<C / 8> (one 16 x 32 tile with its one-pixel ring per block, the tile layout of
 * conv_last_fwd_tail_kernel). */
int rd_bn_act_pool_fwd_tailskip(const float* z, const float* mean, const float* invstd, const float* gamma, const float* beta,
                                float slope, const float* slope_dev, const float* w_last, float* pooled, uint8_t* idx, float* zpool,
                                float* skip9, int n, int h, int w, int c, rd_stream_t s);

/* The rest of rd_conv3x3_last_fwd_tail once skip9 is there:
 *   out[q] = ((skip9[q] + sum_{p': d = q - 2p' in [-1,2]^2} T[p'][d]) + sum_{tap: q + off(tap) inside} B9[tap]) + bias
 *            (+ x[:, 0], the outer residual; x_nchw nullable, x_channels its channel count)
 * t16 = T [N, H/2, W/2, 16] and b9 [9] as there, bias [1] nullable, out [N, 1, H, W].  It takes no z and no channel count.
 * H and W even, N <= 65535, H <= 262140; anything else is refused (RD_ERR_ARG) with nothing written.
 * Memory: reads skip9[0 .. N*H*W), t16[0 .. N*H/2*W/2*16), b9[0 .. 9), bias[0], channel 0 of every image of x_nchw; writes
 * out[0 .. N*H*W) and nothing else.  No scratch.
 * Kernel: conv_last_fwd_pre_kernel (one thread per output pixel). */
int rd_conv3x3_last_fwd_tail_pre(const float* skip9, const float* t16, const float* b9, const float* bias, const float* x_nchw,
                                 int x_channels, float* out, int n, int h, int w, rd_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* RESDEPTH_HIP_TAIL_H */
