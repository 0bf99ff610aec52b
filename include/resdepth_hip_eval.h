/*
 * resdepth_hip_eval.h -- scoring the planes of a pair sweep where the sweep left them: entry points of libresdepth_hip.so
 * (rd_version >= 113), included by resdepth_hip.h; its conventions (device pointers, stream, return codes, memory contract,
 * alignment) hold here.
 *
 * A side header for the reason resdepth_hip_tta.h and resdepth_hip_pairs.h are: the coverage ledger over the main header
 * (tests/test_memory_contract_gpu.py) describes exactly the entry points its case table drives, and the contents of the two
 * other side headers are pinned by their own tests.  The guard-band cases of the entry points below, and a ledger over THIS
 * header, are in tests/test_eval_planes_contract_gpu.py; bindings: resdepth_amd/_lib.py SIGNATURES_EVAL.
 *
 * The reference scores every pair's prediction with evaluate_performance (test.py:191-258) and then the pool of all pairs'
 * residuals class by class (test.py:288-357).  rd_eval_classify_planes is rd_eval_classify for P planes at once -- what does
 * not depend on the pair (area, ground-truth validity, the class bits) is worked out once per pixel --, and
 * rd_residual_stats_pooled is rd_residual_stats_sets for sets whose members come from several planes of one source.
 */
#ifndef RESDEPTH_HIP_EVAL_H
#define RESDEPTH_HIP_EVAL_H

#ifdef __cplusplus
extern "C" {
#endif

#define RD_EVAL_MAX_PLANES 16   /* one bit of the validity word per plane */
#define RD_CLS_VALID_EXTRA 64   /* class bit: gt valid and the extra surface != nodata (only set when `extra` is given) */

/* The plane form of rd_eval_classify: one pass over rows x cols pixels reads the n_planes (1..RD_EVAL_MAX_PLANES, RD_ERR_ARG
 * otherwise) fp64 planes planes[p * plane_stride + i] (plane_stride in doubles, any value >= rows * cols, odd ones included),
 * the initial DSM and the ground truth (f32 or f64 as flagged, never rounded), the 0/1 mask bytes and the area rectangles
 * (all as rd_eval_classify takes them) ONCE and writes
 *   r_before   [n]            initial - gt                                  (nullable: not written)
 *   residuals  n_planes planes, plane_stride apart: planes[p] - gt          (fp64, the subtraction of rd_eval_classify)
 *   cls        [n] bytes      the RD_CLS_* bits of rd_eval_classify with RD_CLS_VALID_AFTER clear
 *   valid      [n] 16-bit words: bit p = ground truth valid here (inside the area, != nodata, gt_mask) and planes[p] != nodata
 *                             -- validity is per prediction, as in the reference (lib/evaluation.py:31 compute_residuals)
 * and, for an optional further surface `extra` [n] (the fused one; NULL together with r_extra):
 *   r_extra    [n]            extra - gt;  RD_CLS_VALID_EXTRA in cls = ground truth valid and extra != nodata,
 * so that rd_residual_stats_sets scores it (and r_before) from the same class byte.
 * With n_planes = 1 residuals is, bit for bit, rd_eval_classify's r_after, and cls | ((valid & 1) << 1) its class byte.
 * Memory: nothing outside [0, n) of r_before, r_extra, cls, valid, and nothing outside [p * plane_stride, p * plane_stride + n)
 * of residuals for p < n_planes, is written: the padding between planes is untouched and the last plane ends at
 * (n_planes - 1) * plane_stride + n.  Nullable: r_before; extra and r_extra (both or neither); gt_mask, building,
 * building_nodata, water, forest; rects when n_rects <= 0.  Aliasing: residuals may BE planes (in place: same pointer, and
 * then the same stride by construction) and r_extra may be extra; any other overlap between an output and an input or
 * another output is a caller error.  Kernel: eval_classify_planes_kernel. */
int rd_eval_classify_planes(const double* planes, long long plane_stride, int n_planes, const double* extra,
                            const void* initial, int initial_f64, const void* gt, int gt_f64, const uint8_t* gt_mask,
                            const uint8_t* building, const uint8_t* building_nodata, const uint8_t* water,
                            const uint8_t* forest, const int* rects, int n_rects, int rows, int cols, double nodata,
                            double* r_before, double* residuals, double* r_extra, uint8_t* cls, uint16_t* valid,
                            rd_stream_t s);

/* The plane form of rd_residual_stats_sets.  All n_sets (1..RD_STATS_MAX_SETS) sets of a call pool the planes p0 .. p1 - 1
 * (0 <= p0 < p1 <= n_planes <= RD_EVAL_MAX_PLANES) of the source src[p * plane_stride + i], i < n (plane_stride >= n).  Set s
 * is the multiset of those values over the planes p of the range and the pixels i where bit p of valid[i] is set (valid
 * NULL: every plane counts), cls[i] holds all bits of set_need[s], and |r| <= set_thr[s] when set_thr[s] > 0.
 * p1 = p0 + 1 scores one pair, [0, n_planes) the pool of all pairs (test.py:288-313).
 * out[s * 8 .. s * 8 + 7] (device doubles) as rd_residual_stats_sets: count, max, min, MAE, RMSE, absolute median, median,
 * NMAD (centred on the set's own absolute median); count .. RMSE from fixed-order partials (two calls give the same bits),
 * the three medians exact (even counts average the two middle values, wherever in the planes they lie); an empty set gives
 * count 0 and NaN elsewhere.  set_need / set_thr are host arrays.
 * The histograms are 32-bit counters: (p1 - p0) * n >= 2^32 is refused with RD_ERR_ARG (split the range, or the raster).
 * Memory: reads src only inside the planes of the range, cls and valid inside [0, n); writes out[0 .. 8 * n_sets) and the
 * first rd_residual_stats_pooled_ws_bytes(n, n_sets) bytes of ws (a smaller ws_bytes: RD_ERR_WS, nothing launched).
 * Nullable: valid.  No output may overlap an input.  Kernels: pooled_moments_kernel, pooled_hist_kernel and the pick / finish
 * kernels of rd_residual_stats_sets. */
size_t rd_residual_stats_pooled_ws_bytes(long long n, int n_sets);
int rd_residual_stats_pooled(const double* src, long long plane_stride, int n_planes, int p0, int p1, const uint8_t* cls,
                             const uint16_t* valid, long long n, const int* set_need, const double* set_thr, int n_sets,
                             double* out, void* ws, size_t ws_bytes, rd_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* RESDEPTH_HIP_EVAL_H */
