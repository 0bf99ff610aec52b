/*
 * resdepth_hip_errmap.h -- where a refined DSM fails and on what ground: the statistics of every cell of a grid, Horn's slope
 * of a DSM, and the bins of a covariate as class bytes.  Entry points of libresdepth_hip.so (rd_version >= 116 with these
 * symbols exported), included by resdepth_hip.h; its conventions (device pointers, stream, return codes, memory contract,
 * alignment: none beyond the element's own) hold here.
 *
 * A side header for the reason resdepth_hip_eval.h is: the coverage ledger over the main header
 * (tests/test_memory_contract_gpu.py) describes exactly the entry points its case table drives.  The guard-band cases of the
 * entry points below, every refusal, and a ledger over THIS header are in tests/test_errmap_contract_gpu.py; bindings:
 * resdepth_amd/_lib.py SIGNATURES_ERRMAP; front end: resdepth_amd/evaluation.py error_map, dsm_slope, evaluate_binned.
 *
 * The reference has none of this: it exports the residual raster (test.py:216-246) and leaves the analysis to a GIS.
 *
 * Every pointer is a device pointer except `edges` (a host array).  No pointer may be null, no output may overlap an input, and
 * a refused call (RD_ERR_ARG, a message in rd_last_error_string) launches nothing and writes nothing.  None of the three takes
 * scratch.
 */
#ifndef RESDEPTH_HIP_ERRMAP_H
#define RESDEPTH_HIP_ERRMAP_H

#ifdef __cplusplus
extern "C" {
#endif

#define RD_CELL_MIN 4     /* smallest and largest side of a cell of rd_cell_stats, in pixels */
#define RD_CELL_MAX 256
#define RD_BIN_MAX 24     /* bins of rd_bin_classes: four planes of six bin bits */
#define RD_CELL_MAX_CELLS 16777216   /* a call of rd_cell_stats takes fewer cells than this (one 256-thread block each) */
#define RD_SLOPE_MAX_ROWS 1048560    /* rows of a raster of rd_dsm_slope: 65535 tiles of 16 rows */

/* The eight numbers of rd_residual_stats_sets for every cell of a grid over a rows x cols raster.
 * Cell (cy, cx) covers rows [cy * cell_h, min(rows, (cy + 1) * cell_h)) and columns [cx * cell_w, min(cols, (cx + 1) * cell_w)):
 * ncy = ceil(rows / cell_h) by ncx = ceil(cols / cell_w) cells, the ragged border cells included.  The MEMBERS of a cell are
 * the src values of its pixels whose class byte holds all bits of `need`, with |r| <= thr when thr > 0 (thr == 0: no
 * truncation): the set of rd_residual_stats_sets restricted to the cell.
 *     out[(cy * ncx + cx) * 8 + 0..7] = count, max, min, MAE, RMSE, absolute median, median, NMAD
 * with the meaning they have there: an even count averages the two middle values (0.5 * (a + b)), NMAD is 1.4826 * the median
 * of |r - absolute median|, an empty cell gives count 0 and NaN elsewhere.  The values are ranked in the order of the engine's
 * 64-bit keys: -0.0 ranks below +0.0, a NaN with the sign bit clear above +Inf and one with the sign bit set below -Inf.  A NaN
 * is never a member when thr > 0.
 * Count, max, min and the three medians are exact.  MAE and RMSE come from fixed-order partials: a pixel of the cell always
 * goes to the same thread, a thread adds its pixels in row-major order, the block adds its threads in one fixed tree; no
 * floating-point atomics.  The same input gives the same bits on every call, whatever the alignment of src.
 * One block of 256 threads per cell: a moments pass, then the radix select of the engine inside the block -- eight passes for
 * the median and the absolute median together, eight for the NMAD, histograms of integer counters in LDS -- each pass reading
 * the cell's src and cls again (a cell is at most 256 x 256 x 9 bytes).  One code path for every cell size.
 * Refused: rows or cols < 1; a cell side outside RD_CELL_MIN..RD_CELL_MAX; need outside 0..255; thr negative or not finite;
 * RD_CELL_MAX_CELLS cells or more (a 16384 x 16384 raster at cell 4).
 * Memory: reads src[0 .. rows * cols) and cls[0 .. rows * cols); writes out[0 .. 8 * ncy * ncx) and nothing else.
 * Kernel: cell_stats_kernel. */
int rd_cell_stats(const double* src, const uint8_t* cls, int rows, int cols, int cell_h, int cell_w, int need, double thr,
                  double* out, rd_stream_t s);

/* Horn's 3 x 3 slope of a DSM as rise over run (the tangent of the slope angle), in fp64.  dsm: rows x cols floats
 * (dsm_f64 == 0) or doubles (dsm_f64 != 0), read as given.  With the neighbours of pixel e laid out as
 *     a b c
 *     d e f          rows increasing downwards, columns to the right
 *     g h i
 *     p = ((c + 2f + i) - (a + 2d + g)) / (8 * gsd_x)
 *     q = ((g + 2h + i) - (a + 2b + c)) / (8 * gsd_y)
 *     slope = sqrt(fl(fl(p * p) + fl(q * q)))
 * the sums evaluated left to right as written, every operation a separately rounded fp64 operation, never contracted into a
 * fused multiply-add; 2f, 2d, 2h, 2b are exact, and 8 * gsd is one fp64 multiplication on the host.  The square root is the
 * device's fp64 square root: within one unit in the last place of the correctly rounded one (exact where p * p + q * q is a
 * perfect square of a representable number).
 * The result is NaN (0x7ff8000000000000) where any of the nine cells equals `nodata`, is NaN, or lies outside the raster: the
 * border ring is NaN, and so is every pixel of a raster with fewer than three rows or columns.  nodata NaN: no value is nodata.
 * Refused: rows or cols < 1; rows > RD_SLOPE_MAX_ROWS; gsd_x or gsd_y not positive or not finite.
 * Memory: reads dsm[0 .. rows * cols); writes slope[0 .. rows * cols) and nothing else.
 * Kernel: dsm_slope_kernel (one launch: a 64 x 16 tile staged in LDS with its one-pixel halo). */
int rd_dsm_slope(const void* dsm, int dsm_f64, int rows, int cols, double nodata, double gsd_x, double gsd_y, double* slope,
                 rd_stream_t s);

/* The bins of a covariate as class bytes the statistics engine can score.  by: n floats (by_f64 == 0) or doubles; cls: n class
 * bytes of rd_eval_classify; edges: a HOST array of n_bins + 1 strictly increasing values, -Inf and +Inf allowed at the ends.
 * Bin b is the half-open interval [edges[b], edges[b + 1]); a NaN `by` value falls in no bin, and neither does a value outside
 * [edges[0], edges[n_bins]).  out holds G = ceil(n_bins / 6) planes of n bytes:
 *     out[g * n + i] = (cls[i] & 3) | (the pixel's bin b lies in group g, 6g <= b < 6g + 6 ? 1 << (2 + b - 6g) : 0)
 * the two validity bits (RD_CLS_VALID_BEFORE, RD_CLS_VALID_AFTER) with one bin bit.  The statistics of bin b are then the set
 * need = validity bit | 1 << (2 + b % 6) of rd_residual_stats_sets (or any call of the engine) on plane b / 6.
 * One pass over by and cls.
 * Refused: n < 1; n_bins outside 1..RD_BIN_MAX; a NaN edge; edges that do not increase strictly.
 * Memory: reads by[0 .. n), cls[0 .. n); writes out[0 .. G * n) and nothing else.
 * Kernel: bin_classes_kernel. */
int rd_bin_classes(const void* by, int by_f64, const uint8_t* cls, long long n, const double* edges, int n_bins, uint8_t* out,
                   rd_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* RESDEPTH_HIP_ERRMAP_H */
