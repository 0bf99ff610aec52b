/*
 * resdepth_hip_pairs.h -- sweeping all image pairs of a raster in one pass: entry points of libresdepth_hip.so
 * (rd_version >= 112), included by resdepth_hip.h; its conventions (device pointers, stream, return codes, memory contract,
 * alignment) hold here.
 *
 * Kept apart from resdepth_hip.h for the reason resdepth_hip_tta.h is: the coverage ledger over the main header
 * (tests/test_memory_contract_gpu.py) describes exactly the entry points its case table drives, and the contents of
 * resdepth_hip_tta.h are pinned by tests/test_tta_cpu.py and tests/test_tta_contract_gpu.py.  The guard-band cases of the two
 * entry points below, and a ledger over THIS header, are in tests/test_pairs_contract_gpu.py.
 * TO FOLD BACK: this split follows from where the tests live, not from the interface.  The next change that may edit
 * tests/test_memory_contract_gpu.py moves the two declarations (and the mode constants) into resdepth_hip.h,
 * _lib.SIGNATURES_PAIRS into _lib.SIGNATURES and the case builders of tests/test_pairs_contract_gpu.py into that file's table,
 * and deletes this header -- together with resdepth_hip_tta.h.  Add no further entry point here: the main ledger does not see
 * this file, and a consumer that parses resdepth_hip.h without following its includes misses what is declared here.
 *
 * The reference predicts a raster once per image pair (test.py:136-189) and pools the residuals of all pairs
 * (test.py:288-313).  With these two entry points one sweep blends every pair's predictions into a plane of its own and a
 * streaming kernel reduces the planes per pixel (the fused surface and how far the pairs disagree).
 */
#ifndef RESDEPTH_HIP_PAIRS_H
#define RESDEPTH_HIP_PAIRS_H

#ifdef __cplusplus
extern "C" {
#endif

/* fuse_mode / spread_mode of rd_fuse_planes */
#define RD_FUSE_MEAN 0
#define RD_FUSE_MEDIAN 1
#define RD_SPREAD_NONE 0
#define RD_SPREAD_RANGE 1
#define RD_SPREAD_STD 2

/* rd_blend_accumulate_tta into one of n_planes rasters: sample i is added to raster + plane[i] * plane_stride (a rows x cols
 * fp64 raster; plane_stride in doubles, >= rows * cols; the planes hold (n_planes - 1) * plane_stride + rows * cols doubles).
 * plane: int32 [n], device; NULL = all 0.  aug: as rd_blend_accumulate_tta, NULL = all 0.  Every other argument, the
 * arithmetic (one fused multiply-add per sample and pixel), the launches (up to 64 samples, in order) and the bounds rule are
 * rd_blend_accumulate_tta's.
 * Order: samples of different planes never meet.  Within a launch a sample j < i takes a pixel from sample i only if
 * plane[j] == plane[i], and a pixel's owner adds only samples of its own plane, in sample order: every plane receives its own
 * samples in their order, as if the call held no others.  So plane p holds, bit for bit, what rd_blend_accumulate_tta gives for
 * the samples of plane p alone -- however the samples of the planes are interleaved and however a list is split into calls --
 * and plane == NULL with n_planes = 1 is rd_blend_accumulate_tta.
 * A plane index outside 0 .. n_planes - 1 is a caller error that the kernel does not write through: the sample is skipped
 * (nothing is added for it, no error is reported).  Kernel: blend_tta_kernel<true>. */
int rd_blend_accumulate_planes(const float* pred, const float* mean, const float* std, const int* pos, const int* reg,
                               const int* aug, const int* plane, int n, int tile_size, int stride, int log2_variants,
                               double* raster, int n_planes, long long plane_stride, int rows, int cols, rd_stream_t s);

/* Per-pixel reduction over n_planes (1..16, RD_ERR_ARG otherwise) fp64 planes of n pixels: v_p = planes[p * plane_stride + i],
 * plane_stride in doubles, any value >= n (odd ones included).  fused [n] and, unless spread_mode is RD_SPREAD_NONE (then it
 * may be NULL), spread [n] are written; they must not overlap the planes.
 *   RD_FUSE_MEAN     acc = v_0; acc = acc + v_p for p = 1 .. n_planes - 1 in plane order; fused = acc / n_planes (a division)
 *   RD_FUSE_MEDIAN   ascending order statistics: the middle value for odd n_planes, (a + b) * 0.5 of the two middle values
 *                    for even n_planes (what np.median computes)
 *   RD_SPREAD_RANGE  max - min, exact
 *   RD_SPREAD_STD    sqrt(sum_p (v_p - m)^2 / n_planes), m the RD_FUSE_MEAN value, summed in plane order from 0 (the compiler
 *                    may contract a square and its add: within (n_planes + 4) * 2^-53 relative of the uncontracted loop)
 * A NaN in any plane gives NaN in every output of that pixel.  mean, median and range are reproduced bit for bit by a float64
 * host loop.  A streaming kernel (fuse_planes_kernel): two pixels per thread, 16-byte non-temporal loads of every plane and
 * 16-byte stores, when planes, fused, spread are 16-byte aligned and plane_stride is even (or n_planes is 1); 8-byte accesses
 * otherwise, and for the last pixel of an odd n.  Nothing past element n - 1 of an output is written. */
int rd_fuse_planes(const double* planes, long long plane_stride, int n_planes, long long n, int fuse_mode, double* fused,
                   int spread_mode, double* spread, rd_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* RESDEPTH_HIP_PAIRS_H */
