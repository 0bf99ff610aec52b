/*
 * resdepth_hip_ortho.h -- ortho-rectification of satellite views onto the grid of a DSM through their rational polynomial camera
 * models (RPC00B): the `orthos = [V, H, W]` planes that GpuPatchSampler and the tiled sweep take, made from raw scenes and the DSM
 * in HBM.  Entry point of libresdepth_hip.so (rd_version >= 116 with this symbol exported), included by resdepth_hip.h; its
 * conventions (device pointers, stream, return codes, memory contract, alignment: none beyond the element's own) hold here.
 *
 * A side header for the reason resdepth_hip_coreg.h is: the coverage ledger over the main header
 * (tests/test_memory_contract_gpu.py) describes exactly the entry points its case table drives.  The guard-band cases of the
 * entry point below, every refusal, and a ledger over THIS header are in tests/test_ortho_contract_gpu.py; bindings:
 * resdepth_amd/_lib.py SIGNATURES_ORTHO; front end: resdepth_amd/ortho.py RPC, orthorectify, project_grid.
 *
 * The reference has none of this: it assumes "that the images have already been ortho-rectified with the help of the initial
 * DSM" (README lines 56-58 and 68).
 *
 * Every pointer is a device pointer.  `valid` and `coords` may be null; no output may overlap an input or another output, and
 * a refused call (RD_ERR_ARG, a message in rd_last_error_string) launches nothing and writes nothing.
 */
#ifndef RESDEPTH_HIP_ORTHO_H
#define RESDEPTH_HIP_ORTHO_H

#ifdef __cplusplus
extern "C" {
#endif

#define RD_ORTHO_MAX_VIEWS 16

#define RD_ORTHO_U8 0 /* element type of an image */
#define RD_ORTHO_U16 1
#define RD_ORTHO_F32 2

#define RD_ORTHO_GEOGRAPHIC 0 /* crs: the grid's X is the longitude and Y the latitude, degrees on WGS84 */
#define RD_ORTHO_UTM 1        /* crs: X easting and Y northing, metres, transverse Mercator on WGS84 */

#define RD_ORTHO_NEAREST 0 /* resampling */
#define RD_ORTHO_BILINEAR 1
#define RD_ORTHO_BICUBIC 2

/* One image and its camera.  image: rows x cols elements of `dtype`, element (y, x) at image[y * pitch + x] (pitch in ELEMENTS,
 * 64-bit: rows need not be contiguous, and the offset is formed in 64 bits).  line0, samp0: the RPC line / sample coordinates of
 * the CENTRE of image[0, 0] -- 0 for a whole scene of a vendor whose model counts from pixel centres, 0.5 for a corner-based
 * model, row0 / col0 more for a crop.  image_nodata: taps that equal it are undefined; NaN: no value is.  The RPC00B model: the ten
 * offsets and scales, and the four 20-term coefficient vectors in RPC00B order. */
typedef struct rd_ortho_view {
    const void* image;
    long long pitch;
    int rows, cols;
    int dtype;
    int reserved;
    double line0, samp0;
    double image_nodata;
    double line_off, samp_off, lat_off, lon_off, height_off;
    double line_scale, samp_scale, lat_scale, lon_scale, height_scale;
    double line_num[20], line_den[20], samp_num[20], samp_den[20];
} rd_ortho_view; /* 776 bytes */

/* out[v] = image v seen from above on the grid of the DSM.  dsm: rows x cols floats; views: DEVICE array of n_views descriptors;
 * out [n_views, rows, cols] float; valid [n_views, rows, cols] uint8 or null; coords [n_views, rows, cols, 2] double or null.
 * For pixel (r, c), every step in fp64:
 *   1. ground point: X = x0 + (c + 0.5) * dx, Y = y0 + (r + 0.5) * dy (dy is usually negative);
 *   2. to degrees: crs RD_ORTHO_GEOGRAPHIC: lon = X, lat = Y.  crs RD_ORTHO_UTM: the inverse of the Krueger series to n^4 on
 *      WGS84 (a = 6378137, f = 1 / 298.257223563, k0 = 0.9996, false easting 500000, n = f / (2 - f),
 *      A = a / (1 + n) * (1 + n^2 / 4 + n^4 / 64)):
 *        xi = (Y - false_northing) / (k0 A), eta = (X - 500000) / (k0 A)
 *        xi' = xi - sum_j beta_j sin(2 j xi) cosh(2 j eta), eta' = eta - sum_j beta_j cos(2 j xi) sinh(2 j eta), j = 1..4
 *        beta_1 = n/2 - 2n^2/3 + 37n^3/96 - n^4/360, beta_2 = n^2/48 + n^3/15 - 437n^4/1440,
 *        beta_3 = 17n^3/480 - 37n^4/840, beta_4 = 4397n^4/161280
 *        lon = lon0_deg + atan2(sinh eta', cos xi') in degrees
 *        tau' = sin xi' / sqrt(sinh^2 eta' + cos^2 xi'), the tangent of the conformal latitude; tau = tan(lat) from it by THREE
 *        Newton steps started at tau' (each: sigma = sinh(e atanh(e tau / sqrt(1 + tau^2))), t = tau sqrt(1 + sigma^2) - sigma
 *        sqrt(1 + tau^2), tau += (tau' - t) / sqrt(1 + t^2) * (1 + (1 - e^2) tau^2) / ((1 - e^2) sqrt(1 + tau^2))); the first
 *        error is e^2 = 0.0067 relative and a step squares it.  sin / cos / sinh / cosh of the multiples 4, 6, 8 come from those
 *        of 2 xi and 2 eta by the addition theorems.  Accuracy: the truncation of the series, 1e-7 m inside a zone
 *        (tests/test_ortho_cpu.py holds the forward and inverse series to 1e-6 m against a quadrature of the meridian arc);
 *   3. h = dsm(r, c) + height_offset.  A DSM value that equals dsm_nodata or is NaN (dsm_nodata NaN: no value is nodata) makes
 *      the pixel undefined in every view;
 *   4. per view: P = (lat - lat_off) / lat_scale, L = (lon - lon_off) / lon_scale, H = (h - height_off) / height_scale;
 *      line = line_num(P, L, H) / line_den(P, L, H) * line_scale + line_off, samp likewise, each polynomial the sum over the
 *      monomials 1, L, P, H, LP, LH, PH, L^2, P^2, H^2, PLH, L^3, LP^2, LH^2, L^2P, P^3, PH^2, L^2H, P^2H, H^3 in that order;
 *      yi = line - line0, xi = samp - samp0: the position in the image, in elements from the centre of image[0, 0];
 *   5. resample at (yi, xi), weights and the sum in fp64, rounded ONCE to float:
 *      RD_ORTHO_NEAREST:  the element at (floor(yi + 0.5), floor(xi + 0.5));
 *      RD_ORTHO_BILINEAR: y0 = floor(yi), fy = yi - y0, x0 = floor(xi), fx = xi - x0; taps v00, v01, v10, v11 at (y0, x0),
 *        (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1); top = v00 + fx (v01 - v00), bot = v10 + fx (v11 - v10), val = top +
 *        fy (bot - top): the formulas of rd_translate_bilinear, and its rule: column x0 + 1 is NOT NEEDED when fx == 0 (top = v00,
 *        bot = v10) and row y0 + 1 is not needed when fy == 0 (val = top);
 *      RD_ORTHO_BICUBIC:  Catmull-Rom (a = -0.5) over the 4 x 4 taps at rows y0 - 1 .. y0 + 2 and columns x0 - 1 .. x0 + 2 with,
 *        for t = fx (and fy), w0 = ((-0.5 t + 1) t - 0.5) t, w1 = (1.5 t - 2.5) t^2 + 1, w2 = ((-1.5 t + 2) t + 0.5) t,
 *        w3 = (0.5 t - 0.5) t^2; val = sum_j wy_j (sum_i wx_i v_ji), rows from the top, columns from the left.  With fx == 0 the
 *        weights are exactly 0, 1, 0, 0: only column x0 is needed then (the row sum is v_j1), and only row y0 with fy == 0.
 *      The pixel is UNDEFINED in a view when a needed tap lies outside the image or equals image_nodata, when line or samp is
 *      not finite, or when the descriptor has a null image, rows or cols < 1 or an unknown dtype (the descriptors live in
 *      device memory: their content cannot be refused by the call).  Bounds are compared as doubles before any conversion to an
 *      integer; element offsets into the image are 64-bit.
 * out(v, r, c) = the value, `fill` where undefined; valid(v, r, c) = 1 / 0; coords(v, r, c) = (yi, xi) for every pixel whose DSM
 * value is defined (whatever the image says), two NaNs otherwise.  out and valid are the same bits with and without valid and
 * coords.  No atomics, no scratch buffer, no data-dependent loop: one thread per DSM pixel walks the n_views views, every other
 * iteration count is a compile-time constant; the same input gives the same bits on every call.
 * Refused: rows or cols < 1; rows * cols >= 2^31; n_views outside 1..RD_ORTHO_MAX_VIEWS; dx or dy zero or not finite; unknown
 * crs or resampling; lon0_deg or height_offset not finite; dsm, views or out null.
 * Memory: reads dsm[0 .. rows * cols), views[0 .. n_views) and the elements of the images that are needed taps; writes
 * out[0 .. n_views * rows * cols), when not null valid[0 .. n_views * rows * cols) and coords[0 .. 2 * n_views * rows * cols),
 * and nothing else.
 * Kernel: ortho_rpc_kernel (one launch, templated on the resampling; the tap load on the element type, chosen per view by a
 * wave-uniform branch: the type is the descriptor's).  A wave covers 64 x 1 pixels of the grid (DESIGN.md 3.6f has the
 * measurement); out, valid and coords leave through non-temporal stores, the taps are gathered through the cache, the model is
 * read through wave-uniform addresses. */
int rd_ortho_rpc(const float* dsm, int rows, int cols, double x0, double dx, double y0, double dy, int crs, double lon0_deg,
                 double false_northing, double dsm_nodata, double height_offset, const rd_ortho_view* views, int n_views,
                 int resampling, float fill, float* out, uint8_t* valid, double* coords, rd_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* RESDEPTH_HIP_ORTHO_H */
