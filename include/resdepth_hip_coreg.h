/*
 * resdepth_hip_coreg.h -- is a DSM aligned with its reference, and if not, by how much: the sums of the least-squares 3-D
 * translation between two gridded surfaces, and the sub-pixel resampler that applies one.  Entry points of libresdepth_hip.so
 * (rd_version >= 116 with these symbols exported), included by resdepth_hip.h; its conventions (device pointers, stream, return
 * codes, memory contract, alignment: none beyond the element's own) hold here.
 *
 * A side header for the reason resdepth_hip_errmap.h is: the coverage ledger over the main header
 * (tests/test_memory_contract_gpu.py) describes exactly the entry points its case table drives.  The guard-band cases of the
 * entry points below, every refusal, and a ledger over THIS header are in tests/test_coreg_contract_gpu.py; bindings:
 * resdepth_amd/_lib.py SIGNATURES_COREG; front end: resdepth_amd/coregistration.py estimate_shift, coregister, translate.
 *
 * The reference has none of this: it requires co-registered rasters of its user (README lines 65-71, lib/DsmOrthoDataset.py:167).
 *
 * The method.  S is the raster to move, G the reference, p = dS/dx and q = dS/dy Horn's gradient of S per metre (columns to the
 * right, rows downwards), d = G - S.  Moving the content of S by (tx, ty) metres and lifting it by tz gives S - tx p - ty q + tz
 * to first order, so d ~ a p + b q + c over the member pixels, solved by the 3 x 3 normal equations out of the ten sums of
 * rd_shift_sums: tx = -a, ty = -b, tz = c.  The caller iterates: rd_translate_bilinear of the ORIGINAL raster by the shift so far,
 * the sums again, the increment added.
 *
 * Every pointer is a device pointer.  Only `cls` may be null (exactly when need == 0); no output may overlap an input, and a
 * refused call (RD_ERR_ARG, a message in rd_last_error_string) launches nothing and writes nothing.
 */
#ifndef RESDEPTH_HIP_COREG_H
#define RESDEPTH_HIP_COREG_H

#ifdef __cplusplus
extern "C" {
#endif

#define RD_SHIFT_NSUMS 10            /* N, Sp, Sq, Sd, Spp, Spq, Sqq, Spd, Sqd, Sdd */
#define RD_SHIFT_MAX_BLOCKS 2048     /* blocks of shift_sums_kernel: a block walks ceil(tiles / RD_SHIFT_MAX_BLOCKS) tiles */
#define RD_SHIFT_MAX_TILES 1073741824 /* 64 x 16 tiles of a raster of rd_shift_sums: the tile index of the launch stays an int */

/* Scratch of rd_shift_sums for a rows x cols raster: RD_SHIFT_NSUMS doubles per block; 0 for a shape the call refuses. */
size_t rd_shift_sums_ws_bytes(int rows, int cols);

/* The ten sums of the translation fit in one pass over src, ref and cls.  src, ref: rows x cols floats (x_f64 == 0) or doubles,
 * read as given and widened exactly; cls: rows x cols class bytes or null.  With the neighbours of src pixel e = (y, x) laid
 * out as
 *     a b c
 *     d e f          rows increasing downwards, columns to the right
 *     g h i
 *     p = ((c + 2f + i) - (a + 2d + g)) / (8 * gsd_x)
 *     q = ((g + 2h + i) - (a + 2b + c)) / (8 * gsd_y)          the formulas and the rounding of rd_dsm_slope
 *     d = fl(ref(y, x) - e)
 * pixel (y, x) is a MEMBER when all of these hold:
 *     1 <= y <= rows - 2 and 1 <= x <= cols - 2;
 *     none of the nine src cells equals `nodata` or is NaN (nodata NaN: no value is nodata);
 *     ref(y, x) neither equals `nodata` nor is NaN;
 *     (cls[y * cols + x] & need) == need;
 *     p, q and d are finite;
 *     |d| <= thr when thr > 0;
 *     fl(fl(p * p) + fl(q * q)) <= fl(slope_max * slope_max) when slope_max > 0 -- the square taken once on the host, no square
 *     root anywhere.
 *     out[0..9] = N, sum p, sum q, sum d, sum p*p, sum p*q, sum q*q, sum p*d, sum q*d, sum d*d over the members
 * every term and every addition a separately rounded fp64 operation, never contracted into a fused multiply-add.  N is exact.
 * The sums are fixed-order: the raster is cut into 64 x 16 tiles in row-major order; with T tiles, W = ceil(T /
 * RD_SHIFT_MAX_BLOCKS) and B = ceil(T / W) blocks, block b walks the tiles b, b + B, b + 2B, ...; pixel (ty, tx) of a tile always
 * goes to thread (ty * 64 + tx) % 256, a thread adds its pixels tile by tile and within a tile from the top; the block adds its
 * threads in one fixed tree (a butterfly inside each wave, then wave 0 + 1 + 2 + 3) into ws[b * 10 + k]; a finish kernel of one
 * block adds the block partials (thread t the partials t, t + 256, ... in that order, then one fixed tree).  No floating-point
 * atomics.  The same input gives the same bits on every call, whatever the alignment of the pointers and whatever ws held; the
 * result depends on the inputs and the shape only.  With zero members out is ten zeros (+0.0).
 * Refused: rows or cols < 1; more than RD_SHIFT_MAX_TILES tiles; gsd_x or gsd_y not positive or not finite; thr or slope_max
 * negative or not finite; need outside 0..255; cls null with need != 0; src, ref, ws or out null; ws_bytes below
 * rd_shift_sums_ws_bytes(rows, cols).
 * Memory: reads src[0 .. rows * cols), ref[0 .. rows * cols) and, when not null, cls[0 .. rows * cols); writes
 * ws[0 .. rd_shift_sums_ws_bytes / 8) and out[0 .. RD_SHIFT_NSUMS) and nothing else.
 * Kernels: shift_sums_kernel (each tile staged in LDS with its one-pixel halo), shift_sums_finish_kernel. */
int rd_shift_sums(const void* src, int src_f64, const void* ref, int ref_f64, const uint8_t* cls, int need, int rows, int cols,
                  double nodata, double gsd_x, double gsd_y, double thr, double slope_max, void* ws, size_t ws_bytes, double* out,
                  rd_stream_t s);

/* The content of a raster moved by (tx, ty) PIXELS (columns to the right, rows downwards) and lifted by tz, resampled
 * bilinearly: out(y, x) = src(y - ty, x - tx) + tz.  src: rows x cols floats (src_f64 == 0) or doubles.  Per pixel, every
 * operation a separately rounded fp64 operation, never contracted:
 *     ys = fl(y - ty), y0 = floor(ys), fy = ys - y0;  xs = fl(x - tx), x0 = floor(xs), fx = xs - x0
 *     taps v00, v01, v10, v11 at (y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1)
 *     top = v00 + fx * (v01 - v00), bot = v10 + fx * (v11 - v10), val = top + fy * (bot - top), out = val + tz
 * Column x0 + 1 is NOT NEEDED when fx == 0 (top = v00 and bot = v10 then, without arithmetic), and row y0 + 1 is not needed
 * when fy == 0 (val = top): a shift by whole pixels is an exact copy, and the last row and column survive it.  Where a needed
 * tap lies outside the raster, equals `nodata` or is NaN (nodata NaN: no value is nodata), out = fill; a NaN -- a NaN fill, or
 * taps of opposite infinities -- is written as 0x7ff8000000000000.  y0 and x0 are compared against the raster as doubles before
 * any conversion to an integer, so |tx| = 1e300 gives a raster of `fill`.
 * Refused: rows or cols < 1; tx, ty or tz not finite; src or out null or the same pointer.
 * Memory: reads src[0 .. rows * cols); writes out[0 .. rows * cols) and nothing else.
 * Kernel: translate_bilinear_kernel (one launch: up to four taps read and one value written per pixel). */
int rd_translate_bilinear(const void* src, int src_f64, int rows, int cols, double nodata, double tx, double ty, double tz,
                          double fill, double* out, rd_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* RESDEPTH_HIP_COREG_H */
