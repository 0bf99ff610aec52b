/*
 * resdepth_hip_dist.h -- error quantiles (LE90 and its kin) and within-tolerance shares of the statistics sets: entry points of
 * libresdepth_hip.so (rd_version >= 116), included by resdepth_hip.h; its conventions (device pointers, stream, return codes,
 * memory contract, alignment) hold here.
 *
 * A side header for the reason resdepth_hip_eval.h is: the coverage ledger over the main header
 * (tests/test_memory_contract_gpu.py) describes exactly the entry points its case table drives.  The guard-band cases of the
 * entry points below, every refusal, and a ledger over THIS header are in tests/test_dist_contract_gpu.py; bindings:
 * resdepth_amd/_lib.py SIGNATURES_DIST.
 *
 * The reference has none of this: it reports eight numbers per set (rd_residual_stats_sets).  Accuracy specifications of
 * satellite DSMs are written as a linear error at a confidence level -- LE90 is the 90 % quantile of |residual| -- and as the
 * share of pixels within a tolerance.  Both come from the same sets, on the device, without a sort.
 *
 * A SET is what it is in rd_residual_stats_sets and rd_residual_stats_pooled: the multiset of the values r whose class byte
 * holds all bits of set_need[s], with |r| <= set_thr[s] when set_thr[s] > 0 (pooled form: and the plane's bit of the validity
 * word set).  c is its member count.
 *
 * QUANTILE j has a level q[j] in [0, 1] and a mode q_mode[j]: 0 ranks r, 1 ranks |r|.  With v_(0) <= ... <= v_(c-1) the ranked
 * values, in fp64:
 *     h  = fl((double)(c - 1) * q[j])                      one multiplication
 *     lo = floor(h)     g = h - lo  (exact)     hi = g > 0 ? lo + 1 : lo
 *     Q  = g == 0 ? v_(lo) : fl(v_(lo) + fl(g * fl(v_(hi) - v_(lo))))
 * three separately rounded operations, never contracted into a fused multiply-add.  This is numpy's default `linear` method up
 * to the form of the interpolation (numpy's lerp rounds in other places; either form rounds at most three times on magnitudes
 * <= 2 M, M = max(|v_(lo)|, |v_(hi)|), so the two differ by at most 16 * 2^-53 * M).  q = 0.5 is the median of
 * rd_residual_stats_sets to within that bound, NOT in bits: the median is 0.5 * (a + b).  c == 0 gives NaN.
 * The values are ranked by the radix select of rd_residual_stats_sets, i.e. in the order of its 64-bit keys: -0.0 ranks below
 * +0.0 (so Q may be either zero; mode 1 ranks fabs(r), which has no -0.0), a NaN with the sign bit clear ranks above +Inf and
 * one with the sign bit set below -Inf (mode 1: every NaN above +Inf).  A NaN is never a member of a set with set_thr > 0.
 *
 * SHARE k has a tolerance tau[k] >= 0:  W_k = (double)#{members : |r| <= tau[k]} / (double)c, both numbers counted in integers
 * (per-wave popcounts, 32-bit LDS counters per block, 64-bit global integer atomics): the same input gives the same bits on
 * every run.  A NaN member is within no tolerance.  c == 0 gives NaN.
 *
 * out[s * (1 + n_q + n_t) + ...] = c, Q_0 .. Q_{n_q - 1}, W_0 .. W_{n_t - 1} as device doubles.
 *
 * Schedule of a call: one launch clears the scratch's counters, one counting pass over the values (member counts and shares),
 * dist_prepare_kernel (shares; per quantile the ranks lo, hi and the weight g from the count, which exists only on the
 * device: no host synchronisation), then the n_sets * n_q selectors in groups of 20, each group eight histogram passes over the
 * values with a pick after each (sets_hist_kernel / pooled_hist_kernel and sets_pick_kernel, the medians' own) and
 * dist_finish_kernel.  n_q == 0: the counting pass alone.
 *
 * Refused with RD_ERR_ARG and nothing launched: n_q + n_t == 0; n_q > RD_DIST_MAX_Q or n_t > RD_DIST_MAX_T (or negative); a
 * level outside [0, 1] or not finite; a mode other than 0 or 1; a negative or non-finite tolerance; n_sets outside
 * 1..RD_STATS_MAX_SETS; n, or (p1 - p0) * n in the pooled form, >= 2^32 (32-bit histogram counters); what the eight-number
 * forms refuse of their shared arguments.  A scratch smaller than the _ws_bytes query: RD_ERR_WS, nothing launched.
 * q, q_mode, tau and the set_* arguments are host arrays.
 * Memory: reads what the eight-number form of the same name reads; writes out[0 .. n_sets * (1 + n_q + n_t)) and the first
 * _ws_bytes(...) bytes of ws, nothing else.  No output may overlap an input.
 */
#ifndef RESDEPTH_HIP_DIST_H
#define RESDEPTH_HIP_DIST_H

#ifdef __cplusplus
extern "C" {
#endif

#define RD_DIST_MAX_Q 8   /* quantiles of a call */
#define RD_DIST_MAX_T 8   /* tolerances of a call */

/* The sets of rd_residual_stats_sets (src0, src1 nullable, cls, n, set_src, set_need, set_thr, n_sets as there).  Kernels:
 * sets_dist_count_kernel, dist_prepare_kernel, sets_hist_kernel, sets_pick_kernel, dist_finish_kernel. */
size_t rd_residual_dist_sets_ws_bytes(long long n, int n_sets, int n_q, int n_t);
int rd_residual_dist_sets(const double* src0, const double* src1, const uint8_t* cls, long long n, const int* set_src,
                          const int* set_need, const double* set_thr, int n_sets, const double* q, const int* q_mode, int n_q,
                          const double* tau, int n_t, double* out, void* ws, size_t ws_bytes, rd_stream_t s);

/* The sets of rd_residual_stats_pooled (src, plane_stride, n_planes, p0, p1, cls, valid nullable, n, set_need, set_thr, n_sets
 * as there): p1 = p0 + 1 one pair, [0, n_planes) the pool of all pairs; the padding between planes is never read.  Kernels:
 * pooled_dist_count_kernel, dist_prepare_kernel, pooled_hist_kernel, sets_pick_kernel, dist_finish_kernel. */
size_t rd_residual_dist_pooled_ws_bytes(long long n, int n_sets, int n_q, int n_t);
int rd_residual_dist_pooled(const double* src, long long plane_stride, int n_planes, int p0, int p1, const uint8_t* cls,
                            const uint16_t* valid, long long n, const int* set_need, const double* set_thr, int n_sets,
                            const double* q, const int* q_mode, int n_q, const double* tau, int n_t, double* out, void* ws,
                            size_t ws_bytes, rd_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* RESDEPTH_HIP_DIST_H */
