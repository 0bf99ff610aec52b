// Co-registration of a DSM to its reference (include/resdepth_hip_coreg.h): the ten sums of the least-squares 3-D translation in
// one pass, and the bilinear resampler that applies a shift.
// shift_sums_kernel: Horn's gradient of the source from a 64 x 16 tile staged in LDS with its one-pixel halo, as dsm_slope_kernel
// forms it (rd_stats.hip), the residual against the reference, the membership test, and ten running sums per thread; every
// operation through the round-to-nearest intrinsics so that -ffp-contract=on fuses nothing.  A block walks the tiles b, b + B,
// ...; which pixel a thread gets and the order it adds them in depend on the shape alone, and so does the tree that follows:
// a butterfly inside each wave, the four waves in order, the block partials in shift_sums_finish_kernel.  No atomics.
// translate_bilinear_kernel: one thread per pixel, the source position and its floor compared against the raster as doubles.
#include "rd_common.h"

namespace rd {

constexpr int SHIFT_TW = 64, SHIFT_TH = 16, SHIFT_THREADS = 256;
constexpr int SHIFT_PER_THREAD = SHIFT_TW * SHIFT_TH / SHIFT_THREADS;      // pixels of a tile that go to one thread
constexpr double DBL_LARGEST = 1.7976931348623157e308;
static_assert(SHIFT_TW * SHIFT_TH % SHIFT_THREADS == 0 && SHIFT_THREADS % SHIFT_TW == 0, "a thread keeps its column in every tile");

__device__ __forceinline__ double coreg_load(const void* p, int f64, long i) {
    return f64 ? ((const double*)p)[i] : (double)((const float*)p)[i];
}

__device__ __forceinline__ double coreg_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// tiles along x and y, tiles a block walks, blocks: functions of the shape alone
struct ShiftGrid {
    long tiles_x, tiles_y, tiles;
    int walk, blocks;
};

static ShiftGrid shift_grid(int rows, int cols) {
    ShiftGrid g;
    g.tiles_x = ((long)cols + SHIFT_TW - 1) / SHIFT_TW;
    g.tiles_y = ((long)rows + SHIFT_TH - 1) / SHIFT_TH;
    g.tiles = g.tiles_x * g.tiles_y;
    g.walk = g.tiles <= RD_SHIFT_MAX_TILES ? (int)((g.tiles + RD_SHIFT_MAX_BLOCKS - 1) / RD_SHIFT_MAX_BLOCKS) : 0;
    g.blocks = g.walk ? (int)((g.tiles + g.walk - 1) / g.walk) : 0;
    return g;
}

// the butterfly of one wave: every lane ends with the same bits
__device__ __forceinline__ double coreg_wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v = __dadd_rn(v, __shfl_xor(v, o));
    return v;
}

__global__ __launch_bounds__(SHIFT_THREADS) void shift_sums_kernel(const void* __restrict__ src, int src_f64,
                                                                   const void* __restrict__ ref, int ref_f64,
                                                                   const uint8_t* __restrict__ cls, unsigned need, int rows,
                                                                   int cols, double nodata, double run_x, double run_y, double thr,
                                                                   int capped, double slope_sq, int tiles_x, int tiles,
                                                                   double* __restrict__ ws) {
    constexpr int PW = SHIFT_TW + 2, PH = SHIFT_TH + 2;
    __shared__ double tile[PH * PW];                   // NaN: nodata, NaN or outside the raster
    __shared__ double red[SHIFT_THREADS / 64][RD_SHIFT_NSUMS];
    const double nanv = coreg_nan();
    const int t = threadIdx.x, lx = t % SHIFT_TW, ly = t / SHIFT_TW;
    double acc[RD_SHIFT_NSUMS];
#pragma unroll
    for (int k = 0; k < RD_SHIFT_NSUMS; ++k) acc[k] = 0.0;

    for (int tl = blockIdx.x; tl < tiles; tl += gridDim.x) {        // tiles <= RD_SHIFT_MAX_TILES = 2^30: tl + gridDim.x fits
        const int tyi = tl / tiles_x, txi = tl - tyi * tiles_x;
        const int ox = txi * SHIFT_TW, oy = tyi * SHIFT_TH;
        // the reference and the class byte of this thread's pixels: asked for before the tile is staged
        double g[SHIFT_PER_THREAD];
        unsigned c[SHIFT_PER_THREAD];
#pragma unroll
        for (int j = 0; j < SHIFT_PER_THREAD; ++j) {
            const int y = oy + ly + j * (SHIFT_THREADS / SHIFT_TW), x = ox + lx;
            const bool in = y < rows && x < cols;
            const long i = (long)y * cols + x;
            g[j] = in ? coreg_load(ref, ref_f64, i) : nanv;
            c[j] = in && cls ? (unsigned)cls[i] : 0xffu;
        }
        __syncthreads();                               // the previous tile has been read by everyone
        for (int i = t; i < PH * PW; i += SHIFT_THREADS) {
            const int py = i / PW, px = i - py * PW;
            const int y = oy - 1 + py, x = ox - 1 + px;
            double v = nanv;
            if (y >= 0 && y < rows && x >= 0 && x < cols) {
                v = coreg_load(src, src_f64, (long)y * cols + x);
                if (v == nodata) v = nanv;
            }
            tile[i] = v;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < SHIFT_PER_THREAD; ++j) {
            const double* r0 = tile + (ly + j * (SHIFT_THREADS / SHIFT_TW)) * PW + lx;      // the row above, from the left neighbour
            const double a = r0[0], b = r0[1], cc = r0[2];
            const double d4 = r0[PW], e = r0[PW + 1], f = r0[PW + 2];
            const double g7 = r0[2 * PW], hh = r0[2 * PW + 1], ii = r0[2 * PW + 2];
            const bool bad = isnan(a) || isnan(b) || isnan(cc) || isnan(d4) || isnan(e) || isnan(f) || isnan(g7) || isnan(hh) ||
                             isnan(ii);
            const double east = __dadd_rn(__dadd_rn(cc, __dmul_rn(2.0, f)), ii);
            const double west = __dadd_rn(__dadd_rn(a, __dmul_rn(2.0, d4)), g7);
            const double south = __dadd_rn(__dadd_rn(g7, __dmul_rn(2.0, hh)), ii);
            const double north = __dadd_rn(__dadd_rn(a, __dmul_rn(2.0, b)), cc);
            const double p = __ddiv_rn(__dsub_rn(east, west), run_x);
            const double q = __ddiv_rn(__dsub_rn(south, north), run_y);
            const double gj = g[j];
            const double d = __dsub_rn(gj, e);
            const double pp = __dmul_rn(p, p), qq = __dmul_rn(q, q);
            bool member = !bad && !isnan(gj) && gj != nodata && (c[j] & need) == need;
            member = member && fabs(p) <= DBL_LARGEST && fabs(q) <= DBL_LARGEST && fabs(d) <= DBL_LARGEST;
            member = member && (!(thr > 0.0) || fabs(d) <= thr);
            member = member && (!capped || __dadd_rn(pp, qq) <= slope_sq);
            if (member) {
                acc[0] = __dadd_rn(acc[0], 1.0);
                acc[1] = __dadd_rn(acc[1], p);
                acc[2] = __dadd_rn(acc[2], q);
                acc[3] = __dadd_rn(acc[3], d);
                acc[4] = __dadd_rn(acc[4], pp);
                acc[5] = __dadd_rn(acc[5], __dmul_rn(p, q));
                acc[6] = __dadd_rn(acc[6], qq);
                acc[7] = __dadd_rn(acc[7], __dmul_rn(p, d));
                acc[8] = __dadd_rn(acc[8], __dmul_rn(q, d));
                acc[9] = __dadd_rn(acc[9], __dmul_rn(d, d));
            }
        }
    }
    const int lane = t & 63, w = t >> 6;
#pragma unroll
    for (int k = 0; k < RD_SHIFT_NSUMS; ++k) {
        const double v = coreg_wave_sum(acc[k]);
        if (lane == 0) red[w][k] = v;
    }
    __syncthreads();
    if (t < RD_SHIFT_NSUMS)
        ws[(long)blockIdx.x * RD_SHIFT_NSUMS + t] = __dadd_rn(__dadd_rn(__dadd_rn(red[0][t], red[1][t]), red[2][t]), red[3][t]);
}

// one block: thread t adds the partials of the blocks t, t + 256, ... in that order, then one fixed tree per sum
__global__ __launch_bounds__(SHIFT_THREADS) void shift_sums_finish_kernel(const double* __restrict__ ws, int nb,
                                                                          double* __restrict__ out) {
    __shared__ double red[RD_SHIFT_NSUMS][SHIFT_THREADS];
    const int t = threadIdx.x;
    double acc[RD_SHIFT_NSUMS];
#pragma unroll
    for (int k = 0; k < RD_SHIFT_NSUMS; ++k) acc[k] = 0.0;
    for (int b = t; b < nb; b += SHIFT_THREADS) {
#pragma unroll
        for (int k = 0; k < RD_SHIFT_NSUMS; ++k) acc[k] = __dadd_rn(acc[k], ws[(long)b * RD_SHIFT_NSUMS + k]);
    }
#pragma unroll
    for (int k = 0; k < RD_SHIFT_NSUMS; ++k) red[k][t] = acc[k];
    __syncthreads();
    for (int off = SHIFT_THREADS / 2; off > 0; off >>= 1) {
        if (t < off) {
#pragma unroll
            for (int k = 0; k < RD_SHIFT_NSUMS; ++k) red[k][t] = __dadd_rn(red[k][t], red[k][t + off]);
        }
        __syncthreads();
    }
    if (t < RD_SHIFT_NSUMS) out[t] = red[t][0];
}

__global__ __launch_bounds__(256) void translate_bilinear_kernel(const void* __restrict__ src, int f64, int rows, int cols,
                                                                 double nodata, double tx, double ty, double tz, double fill,
                                                                 double* __restrict__ out) {
    const double nanv = coreg_nan();
    const double fillv = isnan(fill) ? nanv : fill;
    const long n = (long)rows * cols;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int y = (int)(i / cols), x = (int)(i - (long)y * cols);
        const double ys = __dsub_rn((double)y, ty), xs = __dsub_rn((double)x, tx);
        const double y0 = floor(ys), x0 = floor(xs);
        const double fy = __dsub_rn(ys, y0), fx = __dsub_rn(xs, x0);
        const bool two_x = fx != 0.0, two_y = fy != 0.0;
        // as doubles: a position 1e300 pixels away is outside, not an overflowed integer
        bool ok = y0 >= 0.0 && x0 >= 0.0 && y0 <= (double)(rows - (two_y ? 2 : 1)) && x0 <= (double)(cols - (two_x ? 2 : 1));
        double val = fillv;
        if (ok) {
            const long at = (long)(int)y0 * cols + (int)x0;
            const double v00 = coreg_load(src, f64, at);
            const double v01 = two_x ? coreg_load(src, f64, at + 1) : v00;
            const double v10 = two_y ? coreg_load(src, f64, at + cols) : v00;
            const double v11 = two_x && two_y ? coreg_load(src, f64, at + cols + 1) : v00;
            ok = !(isnan(v00) || v00 == nodata || isnan(v01) || v01 == nodata || isnan(v10) || v10 == nodata || isnan(v11) ||
                   v11 == nodata);
            const double top = two_x ? __dadd_rn(v00, __dmul_rn(fx, __dsub_rn(v01, v00))) : v00;
            const double bot = two_x ? __dadd_rn(v10, __dmul_rn(fx, __dsub_rn(v11, v10))) : v10;
            const double mid = two_y ? __dadd_rn(top, __dmul_rn(fy, __dsub_rn(bot, top))) : top;
            const double lifted = __dadd_rn(mid, tz);
            val = ok ? (isnan(lifted) ? nanv : lifted) : fillv;
        }
        out[i] = val;
    }
}

}  // namespace rd

using namespace rd;

extern "C" {

size_t rd_shift_sums_ws_bytes(int rows, int cols) {
    if (rows < 1 || cols < 1) return 0;
    return (size_t)shift_grid(rows, cols).blocks * RD_SHIFT_NSUMS * sizeof(double);
}

int rd_shift_sums(const void* src, int src_f64, const void* ref, int ref_f64, const uint8_t* cls, int need, int rows, int cols,
                  double nodata, double gsd_x, double gsd_y, double thr, double slope_max, void* ws, size_t ws_bytes, double* out,
                  rd_stream_t s_) {
    RD_REQUIRE(src && ref && ws && out, "rd_shift_sums: null pointer");
    RD_REQUIRE(rows >= 1 && cols >= 1, "rd_shift_sums: bad shape (rows=%d cols=%d)", rows, cols);
    const ShiftGrid g = shift_grid(rows, cols);
    RD_REQUIRE(g.tiles <= RD_SHIFT_MAX_TILES, "rd_shift_sums: %ld x %ld tiles of %d x %d pixels (at most %d)", g.tiles_y,
               g.tiles_x, SHIFT_TH, SHIFT_TW, RD_SHIFT_MAX_TILES);
    RD_REQUIRE(gsd_x > 0.0 && gsd_x <= DBL_LARGEST && gsd_y > 0.0 && gsd_y <= DBL_LARGEST,
               "rd_shift_sums: GSD %g x %g must be positive and finite", gsd_x, gsd_y);
    RD_REQUIRE(thr >= 0.0 && thr <= DBL_LARGEST, "rd_shift_sums: threshold %g must be finite and >= 0", thr);
    RD_REQUIRE(slope_max >= 0.0 && slope_max <= DBL_LARGEST, "rd_shift_sums: slope_max %g must be finite and >= 0", slope_max);
    RD_REQUIRE(need >= 0 && need <= 255, "rd_shift_sums: need %d outside 0..255", need);
    RD_REQUIRE(cls || need == 0, "rd_shift_sums: need %d without class bytes", need);
    const size_t want = (size_t)g.blocks * RD_SHIFT_NSUMS * sizeof(double);
    RD_REQUIRE(ws_bytes >= want, "rd_shift_sums: workspace of %zu bytes, %zu needed", ws_bytes, want);
    hipStream_t s = (hipStream_t)s_;
    // algorithmic bytes: one read of the source, the reference and the class byte of every pixel
    ProfScope ps(s, "shift_sums", 0, (double)rows * cols * ((src_f64 ? 8.0 : 4.0) + (ref_f64 ? 8.0 : 4.0) + (cls ? 1.0 : 0.0)));
    RD_LAUNCH(shift_sums_kernel, dim3((unsigned)g.blocks), dim3(SHIFT_THREADS), 0, s, src, src_f64 ? 1 : 0, ref, ref_f64 ? 1 : 0,
              cls, (unsigned)need, rows, cols, nodata, 8.0 * gsd_x, 8.0 * gsd_y, thr, slope_max > 0.0 ? 1 : 0,
              slope_max * slope_max, (int)g.tiles_x, (int)g.tiles, (double*)ws);
    RD_LAUNCH_CHECK("shift_sums");
    RD_LAUNCH(shift_sums_finish_kernel, dim3(1), dim3(SHIFT_THREADS), 0, s, (const double*)ws, g.blocks, out);
    RD_LAUNCH_CHECK("shift_sums_finish");
    return RD_OK;
}

int rd_translate_bilinear(const void* src, int src_f64, int rows, int cols, double nodata, double tx, double ty, double tz,
                          double fill, double* out, rd_stream_t s_) {
    RD_REQUIRE(src && out && (const void*)out != src, "rd_translate_bilinear: null or aliased pointer");
    RD_REQUIRE(rows >= 1 && cols >= 1, "rd_translate_bilinear: bad shape (rows=%d cols=%d)", rows, cols);
    RD_REQUIRE(fabs(tx) <= DBL_LARGEST && fabs(ty) <= DBL_LARGEST && fabs(tz) <= DBL_LARGEST,
               "rd_translate_bilinear: shift (%g, %g, %g) must be finite", tx, ty, tz);
    hipStream_t s = (hipStream_t)s_;
    const long n = (long)rows * cols;
    ProfScope ps(s, "translate_bilinear", 0, (double)n * ((src_f64 ? 8.0 : 4.0) + 8.0));
    const long blocks = (n + 255) / 256;
    RD_LAUNCH(translate_bilinear_kernel, dim3((unsigned)(blocks < 1048576 ? blocks : 1048576)), dim3(256), 0, s, src,
              src_f64 ? 1 : 0, rows, cols, nodata, tx, ty, tz, fill, out);
    RD_LAUNCH_CHECK("translate_bilinear");
    return RD_OK;
}

}  // extern "C"
