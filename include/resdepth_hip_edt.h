/*
 * resdepth_hip_edt.h -- how far is every pixel from a mask, and which pixel of the mask is nearest: the exact squared Euclidean
 * distance transform of a byte mask with its feature transform, and the nearest-valid fill that reads it.  Entry points of
 * libresdepth_hip.so (rd_version >= 116 with these symbols exported), included by resdepth_hip.h; its conventions (device
 * pointers, stream, return codes, memory contract, alignment: none beyond the element's own) hold here.
 *
 * A side header for the reason resdepth_hip_errmap.h is: the coverage ledger over the main header
 * (tests/test_memory_contract_gpu.py) describes exactly the entry points its case table drives.  The guard-band cases of the
 * entry points below, every refusal, and a ledger over THIS header are in tests/test_edt_contract_gpu.py; bindings:
 * resdepth_amd/_lib.py SIGNATURES_EDT; front end: resdepth_amd/morphology.py distance_transform, edge_distance, buffer_mask,
 * fill_voids.
 *
 * The reference has none of this: distances to building outlines, metric buffers and void filling are left to GDAL and scipy on
 * the host.
 *
 * Integer arithmetic throughout: no floating point, no atomics on global memory.  The same input gives the same bits on every
 * call, whatever the alignment of the pointers and whatever ws and the outputs held.
 *
 * Every pointer is a device pointer.  Only `idx` of rd_edt_sq may be null; no output may overlap an input, and a refused call
 * (RD_ERR_ARG, a message in rd_last_error_string) launches nothing and writes nothing.
 */
#ifndef RESDEPTH_HIP_EDT_H
#define RESDEPTH_HIP_EDT_H

#ifdef __cplusplus
extern "C" {
#endif

#define RD_EDT_MAX_ROWS 32768        /* rows^2 + cols^2 < 2^31 and rows * cols < 2^31: d2 and idx stay int32 */
#define RD_EDT_MAX_COLS 16384        /* a row of int16 offsets is at most 32 KiB of LDS */
#define RD_EDT_NONE 2147483647       /* d2 where the mask has no set pixel; idx is -1 there */
#define RD_EDT_BAND_ROWS 128         /* rows of a band of the column pass: one thread scans one band of one column */

/* Scratch of rd_edt_sq for a rows x cols mask: two int32 per band and column (the first and the last set row of the band),
 * ceil(rows / RD_EDT_BAND_ROWS) * cols * 8 bytes; 0 for a shape the call refuses.  A function of the shape alone. */
size_t rd_edt_ws_bytes(int rows, int cols);

/* The exact squared Euclidean distance transform of a rows x cols byte mask, and its feature transform.  A pixel is SET when its
 * mask byte is non-zero (invert == 0) or zero (invert != 0); any non-zero byte counts, not only 1.
 *     d2[r * cols + c]  = min over the set pixels (y, x) of (y - r)^2 + (x - c)^2, in pixels^2: 0 on a set pixel
 *     idx[r * cols + c] = y * cols + x of the set pixel that attains it
 * THE TIE RULE: among the set pixels at the minimal d2 the one with the smallest |x - c| wins, then the smaller column x, then
 * the smaller row y.  With no set pixel at all d2 is RD_EDT_NONE everywhere and idx is -1 everywhere.  idx may be null: nothing
 * of it is computed or written then, and d2 has the same bits.
 * Two passes.  The column pass gives every pixel the signed row offset to the nearest set pixel of its own column, the upper one
 * on a tie: edt_band_kernel scans every band of RD_EDT_BAND_ROWS rows of every column once (one thread each, threads along the
 * columns), leaves the nearest set row above inside the band in d2's storage and the band's first and last set row in ws;
 * edt_column_kernel finds the nearest set rows beyond the band in ws, scans the band upwards and leaves the offset in d2's
 * storage.  The row pass, edt_row_kernel, takes one block per row: the row's offsets staged in LDS as int16 before anything is
 * written, then every pixel searches outward from its own column, dx = 0, 1, 2, ... while dx^2 is below the best so far, left
 * before right with a strict comparison, never past either end of the row.  The work per pixel grows with its distance.
 * Refused: rows or cols < 1; rows > RD_EDT_MAX_ROWS or cols > RD_EDT_MAX_COLS; ws_bytes below rd_edt_ws_bytes(rows, cols);
 * mask, d2 or ws null; d2 or idx overlapping mask, or each other.
 * Memory: reads mask[0 .. rows * cols); writes d2[0 .. rows * cols), when not null idx[0 .. rows * cols), and
 * ws[0 .. rd_edt_ws_bytes / 4) (an int32 array) and nothing else.
 * Kernels: edt_band_kernel, edt_column_kernel, edt_row_kernel. */
int rd_edt_sq(const uint8_t* mask, int invert, int rows, int cols, int32_t* d2, int32_t* idx, void* ws, size_t ws_bytes,
              rd_stream_t s);

/* The value of the nearest set pixel where it is near enough, the pixel's own value elsewhere.  dsm, out: n floats
 * (dsm_f64 == 0) or doubles, copied as bit patterns (a NaN keeps its payload); d2, idx: n values each, as rd_edt_sq wrote them.
 *     out[i] = (d2[i] > 0 && d2[i] <= max_d2 && 0 <= idx[i] < n) ? dsm[idx[i]] : dsm[i]
 * An idx[i] >= n is treated as -1: it is never dereferenced.  max_d2 = RD_EDT_NONE - 1 means no cap, max_d2 = 0 a plain copy.
 * Refused: n < 1; max_d2 < 0; dsm, d2, idx or out null; out overlapping dsm.
 * Memory: reads dsm[0 .. n), d2[0 .. n), idx[0 .. n); writes out[0 .. n) and nothing else.
 * Kernel: fill_nearest_kernel (one grid-stride launch). */
int rd_fill_nearest(const void* dsm, int dsm_f64, const int32_t* d2, const int32_t* idx, long long n, int max_d2, void* out,
                    rd_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* RESDEPTH_HIP_EDT_H */
