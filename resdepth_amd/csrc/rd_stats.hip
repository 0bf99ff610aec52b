// Masked residual statistics of a refined DSM against the ground truth on the GPU (lib/evaluation.py:11-131:
// compute_residuals + get_statistics): count, max, min, MAE, RMSE and the three medians (absolute median, median,
// NMAD = 1.4826 * median|r - absolute_median|), optionally after truncating |r| > threshold.
//
// Medians are exact: an 8-pass radix select over the order-preserving 64-bit keys of the fp64 values, both middle
// ranks at once (even counts average the two middle values like np.ma.median).  Histograms are integer counters, so
// the result is independent of scheduling; sums go through fixed-order block partials.  No host synchronisation.
#include "rd_common.h"

namespace rd {

struct SelState {
    unsigned long long prefix[2];
    long long rank[2];
    long long count;
    double shift;
};

__device__ __forceinline__ unsigned long long key_of(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double unkey(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}
__device__ __forceinline__ double pick_value(double r, int mode, double shift) {
    return mode == 0 ? r : (mode == 1 ? fabs(r) : fabs(r - shift));
}

__global__ __launch_bounds__(256) void residual_kernel(const double* __restrict__ raster, const float* __restrict__ gt,
                                                       const uint8_t* __restrict__ mask, long n, double nodata,
                                                       double thr, double* __restrict__ r, uint8_t* __restrict__ valid,
                                                       double* __restrict__ partial) {
    __shared__ double red[5 * 256];
    double cnt = 0.0, sa = 0.0, sq = 0.0, mn = INFINITY, mx = -INFINITY;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const double a = raster[i], g = (double)gt[i];
        const double d = a - g;
        bool ok = (a != nodata) && (g != nodata) && (!mask || mask[i]);
        if (thr > 0.0) ok = ok && (fabs(d) <= thr);
        r[i] = d;
        valid[i] = ok ? 1 : 0;
        if (ok) {
            cnt += 1.0;
            sa += fabs(d);
            sq += d * d;
            mn = fmin(mn, d);
            mx = fmax(mx, d);
        }
    }
    const int t = threadIdx.x;
    red[t] = cnt; red[256 + t] = sa; red[512 + t] = sq; red[768 + t] = mn; red[1024 + t] = mx;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) {
            red[t] += red[t + off];
            red[256 + t] += red[256 + t + off];
            red[512 + t] += red[512 + t + off];
            red[768 + t] = fmin(red[768 + t], red[768 + t + off]);
            red[1024 + t] = fmax(red[1024 + t], red[1024 + t + off]);
        }
        __syncthreads();
    }
    if (t == 0)
        for (int q = 0; q < 5; ++q) partial[blockIdx.x * 5 + q] = red[q * 256];
}

__global__ void moments_finish_kernel(const double* __restrict__ partial, int nb, double* __restrict__ out,
                                      SelState* __restrict__ st) {
    if (threadIdx.x || blockIdx.x) return;
    double cnt = 0.0, sa = 0.0, sq = 0.0, mn = INFINITY, mx = -INFINITY;
    for (int b = 0; b < nb; ++b) {
        cnt += partial[b * 5];
        sa += partial[b * 5 + 1];
        sq += partial[b * 5 + 2];
        mn = fmin(mn, partial[b * 5 + 3]);
        mx = fmax(mx, partial[b * 5 + 4]);
    }
    const double nanv = __longlong_as_double(0x7ff8000000000000ll);
    out[0] = cnt;
    out[1] = cnt > 0 ? mx : nanv;
    out[2] = cnt > 0 ? mn : nanv;
    out[3] = cnt > 0 ? sa / cnt : nanv;
    out[4] = cnt > 0 ? sqrt(sq / cnt) : nanv;
    st->count = (long long)cnt;
}

__global__ void select_init_kernel(SelState* st, unsigned* hist, const double* shift_src) {
    const int t = threadIdx.x;
    for (int i = t; i < 512; i += blockDim.x) hist[i] = 0u;
    if (t == 0) {
        st->prefix[0] = st->prefix[1] = 0ull;
        st->rank[0] = (st->count - 1) / 2;
        st->rank[1] = st->count / 2;
        st->shift = shift_src ? *shift_src : 0.0;
    }
}

__global__ __launch_bounds__(256) void select_hist_kernel(const double* __restrict__ r, const uint8_t* __restrict__ valid,
                                                          long n, int mode, int pass, const SelState* __restrict__ st,
                                                          unsigned* __restrict__ hist) {
    __shared__ unsigned lh[512];
    for (int i = threadIdx.x; i < 512; i += 256) lh[i] = 0u;
    __syncthreads();
    const double shift = st->shift;
    const unsigned long long p0 = st->prefix[0], p1 = st->prefix[1];
    const int hs = 8 * (pass + 1);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        if (!valid[i]) continue;
        const unsigned long long k = key_of(pick_value(r[i], mode, shift));
        const unsigned long long hi = pass == 7 ? 0ull : (k >> hs);
        const unsigned b = (unsigned)((k >> (8 * pass)) & 255ull);
        if (hi == p0) atomicAdd(&lh[b], 1u);
        if (hi == p1) atomicAdd(&lh[256 + b], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 512; i += 256)
        if (lh[i]) atomicAdd(&hist[i], lh[i]);
}

__global__ void select_pick_kernel(SelState* st, unsigned* hist) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        for (int s = 0; s < 2; ++s) {
            long long rank = st->rank[s], below = 0;
            int bin = 255;
            for (int b = 0; b < 256; ++b) {
                const long long c = hist[s * 256 + b];
                if (rank < below + c) {
                    bin = b;
                    break;
                }
                below += c;
            }
            st->prefix[s] = (st->prefix[s] << 8) | (unsigned long long)bin;
            st->rank[s] = rank - below;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 512; i += blockDim.x) hist[i] = 0u;
}

__global__ void select_finish_kernel(const SelState* st, double* dst, double scale) {
    if (threadIdx.x || blockIdx.x) return;
    const double nanv = __longlong_as_double(0x7ff8000000000000ll);
    dst[0] = st->count > 0 ? scale * 0.5 * (unkey(st->prefix[0]) + unkey(st->prefix[1])) : nanv;
}

static int stats_grid(long n) {
    long g = (n + 255) / 256;
    if (g > 2048) g = 2048;
    if (g < 1) g = 1;
    return (int)g;
}

}  // namespace rd

using namespace rd;

extern "C" {

size_t rd_residual_stats_ws_bytes(long long n) {
    const size_t nn = (size_t)((n + 15) / 16 * 16);
    return nn * sizeof(double) + nn + (size_t)stats_grid(n) * 5 * sizeof(double) + 512 * sizeof(unsigned) + 256;
}

int rd_residual_stats(const double* raster, const float* gt, const uint8_t* mask, long long n, double nodata,
                      double threshold, double* out, void* ws, size_t ws_bytes, rd_stream_t s_) {
    RD_REQUIRE(raster && gt && out && n > 0, "rd_residual_stats: bad arguments");
    if (!ws || ws_bytes < rd_residual_stats_ws_bytes(n)) {
        set_error("rd_residual_stats: workspace too small (%zu < %zu)", ws_bytes, rd_residual_stats_ws_bytes(n));
        return RD_ERR_WS;
    }
    hipStream_t s = (hipStream_t)s_;
    const size_t nn = (size_t)((n + 15) / 16 * 16);
    const int nb = stats_grid(n);
    char* base = (char*)ws;
    double* r = (double*)base;
    uint8_t* valid = (uint8_t*)(base + nn * sizeof(double));
    double* partial = (double*)(base + nn * sizeof(double) + nn);
    unsigned* hist = (unsigned*)((char*)partial + (size_t)nb * 5 * sizeof(double));
    SelState* st = (SelState*)((char*)hist + 512 * sizeof(unsigned));
    ProfScope ps(s, "residual_stats", 0, 13.0 * n + 24.0 * 9.0 * n);
    RD_LAUNCH(residual_kernel, dim3(nb), dim3(256), 0, s, raster, gt, mask, (long)n, nodata, threshold, r, valid,
                       partial);
    RD_LAUNCH(moments_finish_kernel, dim3(1), dim3(64), 0, s, (const double*)partial, nb, out, st);
    // out: 0 count, 1 max, 2 min, 3 MAE, 4 RMSE, 5 absolute_median, 6 median, 7 NMAD
    const int modes[3] = {1, 0, 2};
    const int dst[3] = {5, 6, 7};
    for (int m = 0; m < 3; ++m) {
        RD_LAUNCH(select_init_kernel, dim3(1), dim3(256), 0, s, st, hist, m == 2 ? (const double*)(out + 5) : nullptr);
        for (int pass = 7; pass >= 0; --pass) {
            RD_LAUNCH(select_hist_kernel, dim3(nb), dim3(256), 0, s, (const double*)r, (const uint8_t*)valid,
                               (long)n, modes[m], pass, (const SelState*)st, hist);
            RD_LAUNCH(select_pick_kernel, dim3(1), dim3(256), 0, s, st, hist);
        }
        RD_LAUNCH(select_finish_kernel, dim3(1), dim3(64), 0, s, (const SelState*)st, out + dst[m],
                           m == 2 ? 1.4826 : 1.0);
    }
    RD_LAUNCH_CHECK("residual_stats");
    return RD_OK;
}

}  // extern "C"

// ---- class-partitioned evaluation (lib/evaluation.py:163-457 evaluate_performance; for the P planes of a pair sweep
// test.py:191-357, include/resdepth_hip_eval.h) ----------------------------------------------------------------------------
// rd_dilate_mask: the L1-ball dilation of lib/rasterutils.py:88 in one launch.  A 64 x 32 output tile is staged in LDS
// with a k-pixel halo; per haloed row and output column the distance to the nearest set pixel of that row (capped at
// k + 1), then out = OR over dy of (row distance at dy) <= k - |dy|, exactly the diamond of radius k.
//
// Classification, two forms of one pixel rule.  Shared (area_contains, gt_valid, class_bits): the area rectangles, the
// ground truth's validity and the building / terrain bits, worked out once per pixel.  eval_classify_kernel adds one
// prediction with its residual and RD_CLS_VALID_AFTER.  eval_classify_planes_kernel adds P planes and an optional extra
// surface (the fused one): per plane one load, one subtraction, one store and one bit of the validity word.  The planes are
// walked with a running pointer, one value live at a time: no array of P values, so nothing is indexed by a runtime number
// (scripts/check_isa.sh fails the build on scratch).  The residual planes may be the input planes: a thread reads plane p
// of its pixel before it writes it and no other thread touches that element, so neither pointer is __restrict__.
//
// Statistics sets, two forms of one engine.  Shared: every set's moments in one pass (SetMoments: per-set registers,
// fixed-order block partials), then the exact medians of all sets by the radix select of rd_residual_stats with the
// histograms of up to SEL_GROUP selectors (set x {median, absolute median} in one phase, NMAD in the next) filled by one
// read of the values per pass (hist_begin / hist_count / hist_flush); the finish, shift, pick and select-finish kernels, the
// workspace (StatsWs) and the launch schedule (make_select_plan, run_selection).  A form is the loop that produces
// (class, value): rd_residual_stats_sets reads two sources and a set picks one; rd_residual_stats_pooled draws a set's
// members from planes p0 .. p1 - 1 of one strided source under a per-pixel validity word.  There the class byte and the
// validity word are read once per round and serve every plane and every selector; the plane loop is the outer one, so a
// round holds HB values of ONE plane in registers (indexed by the unrolled u only).

namespace rd {

constexpr int DIL_TW = 64, DIL_TH = 32;
constexpr int SEL_GROUP = 20;        // selectors sharing one histogram pass: 20 x 2 ranks x 256 bins x 4 B = 40 KB of LDS
constexpr int HB = 8;                // pixels per thread and round of the histogram kernels

__global__ __launch_bounds__(256) void dilate_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int rows,
                                                     int cols, int k) {
    __shared__ uint8_t tile[(DIL_TH + 2 * RD_DILATE_MAX_ITER) * (DIL_TW + 2 * RD_DILATE_MAX_ITER)];
    __shared__ uint8_t hd[(DIL_TH + 2 * RD_DILATE_MAX_ITER) * DIL_TW];
    const int pw = DIL_TW + 2 * k, ph = DIL_TH + 2 * k;
    const int ox = blockIdx.x * DIL_TW, oy = blockIdx.y * DIL_TH;
    for (int i = threadIdx.x; i < pw * ph; i += blockDim.x) {
        const int ty = i / pw, tx = i - ty * pw;
        const int y = oy - k + ty, x = ox - k + tx;
        tile[i] = (y >= 0 && y < rows && x >= 0 && x < cols) ? (in[(long)y * cols + x] != 0) : 0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ph * DIL_TW; i += blockDim.x) {
        const int ty = i / DIL_TW, tx = i - ty * DIL_TW;
        const uint8_t* c = tile + ty * pw + tx + k;
        int d = k + 1;
        for (int dx = k; dx >= 0; --dx)
            if (c[dx] | c[-dx]) d = dx;
        hd[i] = (uint8_t)d;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < DIL_TH * DIL_TW; i += blockDim.x) {
        const int ty = i / DIL_TW, tx = i - ty * DIL_TW;
        const int y = oy + ty, x = ox + tx;
        if (y >= rows || x >= cols) continue;
        bool on = false;
        for (int dy = -k; dy <= k; ++dy) on |= hd[(ty + k + dy) * DIL_TW + tx] <= k - abs(dy);
        out[(long)y * cols + x] = on ? 1 : 0;
    }
}

struct EvalRects {
    int n;                               // < 0: the whole raster
    int r[RD_EVAL_MAX_RECTS][4];         // y0, y1, x0, x1 (half-open)
};

__device__ __forceinline__ double load_f(const void* p, int f64, long i) {
    return f64 ? ((const double*)p)[i] : (double)((const float*)p)[i];
}

__device__ __forceinline__ bool area_contains(const EvalRects& area, int y, int x) {
    bool in = area.n < 0;
    for (int q = 0; q < area.n; ++q)
        in |= y >= area.r[q][0] && y < area.r[q][1] && x >= area.r[q][2] && x < area.r[q][3];
    return in;
}

__device__ __forceinline__ bool gt_valid(bool in, double g, double nodata, const uint8_t* gt_mask, long i) {
    return in && g != nodata && (!gt_mask || gt_mask[i]);
}

// the building / terrain bits of pixel i (none without a building mask)
__device__ __forceinline__ unsigned class_bits(bool in, long i, const uint8_t* bdil, const uint8_t* bnod,
                                               const uint8_t* water, const uint8_t* forest) {
    unsigned c = 0;
    if (bdil) {
        const bool b = bdil[i] != 0;
        const bool t = in && !b && !(bnod && bnod[i]);
        const bool tw = t && !(water && water[i]);
        if (in && b) c |= RD_CLS_BUILDING;
        if (t) c |= RD_CLS_TERRAIN;
        if (tw) c |= RD_CLS_TERRAIN_NOWATER;
        if (tw && !(forest && forest[i])) c |= RD_CLS_TERRAIN_NOWATER_NOFOREST;
    }
    return c;
}

__global__ __launch_bounds__(256) void eval_classify_kernel(
    const double* __restrict__ pred, const void* __restrict__ init, int init_f64, const void* __restrict__ gt, int gt_f64,
    const uint8_t* __restrict__ gt_mask, const uint8_t* __restrict__ bdil, const uint8_t* __restrict__ bnod,
    const uint8_t* __restrict__ water, const uint8_t* __restrict__ forest, EvalRects area, int rows, int cols,
    double nodata, double* __restrict__ rb, double* __restrict__ ra, uint8_t* __restrict__ cls) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= cols) return;
    for (int y = blockIdx.y; y < rows; y += gridDim.y) {
        const long i = (long)y * cols + x;
        const bool in = area_contains(area, y, x);
        const double g = load_f(gt, gt_f64, i), a = load_f(init, init_f64, i), p = pred[i];
        const bool gok = gt_valid(in, g, nodata, gt_mask, i);
        unsigned c = 0;
        if (gok && a != nodata) c |= RD_CLS_VALID_BEFORE;
        if (gok && p != nodata) c |= RD_CLS_VALID_AFTER;
        c |= class_bits(in, i, bdil, bnod, water, forest);
        rb[i] = a - g;
        ra[i] = p - g;
        cls[i] = (uint8_t)c;
    }
}

__global__ __launch_bounds__(256) void eval_classify_planes_kernel(
    const double* planes, long plane_stride, int n_planes, const double* extra, const void* __restrict__ init, int init_f64,
    const void* __restrict__ gt, int gt_f64, const uint8_t* __restrict__ gt_mask, const uint8_t* __restrict__ bdil,
    const uint8_t* __restrict__ bnod, const uint8_t* __restrict__ water, const uint8_t* __restrict__ forest, EvalRects area,
    int rows, int cols, double nodata, double* __restrict__ rb, double* res, double* r_extra, uint8_t* __restrict__ cls,
    uint16_t* __restrict__ valid) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= cols) return;
    for (int y = blockIdx.y; y < rows; y += gridDim.y) {
        const long i = (long)y * cols + x;
        const bool in = area_contains(area, y, x);
        const double g = load_f(gt, gt_f64, i), a = load_f(init, init_f64, i);
        const bool gok = gt_valid(in, g, nodata, gt_mask, i);
        unsigned c = 0;
        if (gok && a != nodata) c |= RD_CLS_VALID_BEFORE;
        c |= class_bits(in, i, bdil, bnod, water, forest);
        if (extra) {
            const double e = extra[i];
            if (gok && e != nodata) c |= RD_CLS_VALID_EXTRA;
            r_extra[i] = e - g;
        }
        unsigned v = 0;
        const double* src = planes + i;
        double* dst = res + i;
        for (int p = 0; p < n_planes; ++p, src += plane_stride, dst += plane_stride) {
            const double pv = *src;
            if (gok && pv != nodata) v |= 1u << p;
            *dst = pv - g;
        }
        if (rb) rb[i] = a - g;
        cls[i] = (uint8_t)c;
        valid[i] = (uint16_t)v;
    }
}

struct SetSpecs {
    int n;
    int src[RD_STATS_MAX_SETS];
    unsigned need[RD_STATS_MAX_SETS];
    double thr[RD_STATS_MAX_SETS];
};

__device__ __forceinline__ bool in_set(const SetSpecs& sp, int s, unsigned c, double r) {
    return (c & sp.need[s]) == sp.need[s] && (sp.thr[s] <= 0.0 || fabs(r) <= sp.thr[s]);
}

__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wave_min(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// count, sum|r|, sum r^2, min, max of every set over a thread's values, in registers: the arrays are indexed by unrolled
// loops only (an array indexed by a runtime value goes to scratch)
struct SetMoments {
    double cnt[RD_STATS_MAX_SETS], sa[RD_STATS_MAX_SETS], sq[RD_STATS_MAX_SETS], mn[RD_STATS_MAX_SETS],
        mx[RD_STATS_MAX_SETS];

    __device__ __forceinline__ SetMoments() {
#pragma unroll
        for (int s = 0; s < RD_STATS_MAX_SETS; ++s) {
            cnt[s] = sa[s] = sq[s] = 0.0;
            mn[s] = INFINITY;
            mx[s] = -INFINITY;
        }
    }

    // one pixel (or pixel-plane) of class c: value_of(s) is what set s reads there
    template <class ValueOf>
    __device__ __forceinline__ void add(const SetSpecs& sp, unsigned c, ValueOf value_of) {
#pragma unroll
        for (int s = 0; s < RD_STATS_MAX_SETS; ++s) {
            const double d = value_of(s);
            if (s < sp.n && in_set(sp, s, c, d)) {
                cnt[s] += 1.0;
                sa[s] += fabs(d);
                sq[s] += d * d;
                mn[s] = fmin(mn[s], d);
                mx[s] = fmax(mx[s], d);
            }
        }
    }

    // store()'s tree for ONE set, left in LDS: o[0..4] = the block's count, sum|r|, sum r^2, min, max of set s, written by
    // thread 0 and visible to the block on return; every thread of the block is here (cell_stats_kernel)
    __device__ __forceinline__ void reduce(int s, double (*red)[5], double* o) const {
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        const double v0 = wave_sum(cnt[s]), v1 = wave_sum(sa[s]), v2 = wave_sum(sq[s]), v3 = wave_min(mn[s]),
                     v4 = wave_max(mx[s]);
        if (lane == 0) {
            red[w][0] = v0; red[w][1] = v1; red[w][2] = v2; red[w][3] = v3; red[w][4] = v4;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            o[0] = red[0][0] + red[1][0] + red[2][0] + red[3][0];
            o[1] = red[0][1] + red[1][1] + red[2][1] + red[3][1];
            o[2] = red[0][2] + red[1][2] + red[2][2] + red[3][2];
            o[3] = fmin(fmin(red[0][3], red[1][3]), fmin(red[2][3], red[3][3]));
            o[4] = fmax(fmax(red[0][4], red[1][4]), fmax(red[2][4], red[3][4]));
        }
        __syncthreads();
    }

    // partial[(block * n_sets + s) * 5 + q]: the block's moments of set s, waves added in a fixed order
    __device__ __forceinline__ void store(double* __restrict__ partial, const SetSpecs& sp, double (*red)[5]) const {
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
        for (int s = 0; s < RD_STATS_MAX_SETS; ++s) {
            if (s >= sp.n) continue;
            const double v0 = wave_sum(cnt[s]), v1 = wave_sum(sa[s]), v2 = wave_sum(sq[s]), v3 = wave_min(mn[s]),
                         v4 = wave_max(mx[s]);
            if (lane == 0) {
                red[w][0] = v0; red[w][1] = v1; red[w][2] = v2; red[w][3] = v3; red[w][4] = v4;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                double* o = partial + ((long)blockIdx.x * sp.n + s) * 5;
                o[0] = red[0][0] + red[1][0] + red[2][0] + red[3][0];
                o[1] = red[0][1] + red[1][1] + red[2][1] + red[3][1];
                o[2] = red[0][2] + red[1][2] + red[2][2] + red[3][2];
                o[3] = fmin(fmin(red[0][3], red[1][3]), fmin(red[2][3], red[3][3]));
                o[4] = fmax(fmax(red[0][4], red[1][4]), fmax(red[2][4], red[3][4]));
            }
            __syncthreads();
        }
    }
};

__global__ __launch_bounds__(256) void sets_moments_kernel(const double* __restrict__ src0, const double* __restrict__ src1,
                                                           const uint8_t* __restrict__ cls, long n, SetSpecs sp,
                                                           double* __restrict__ partial) {
    __shared__ double red[4][5];
    SetMoments m;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const double r0 = src0[i], r1 = src1[i];
        m.add(sp, cls[i], [&](int s) { return sp.src[s] ? r1 : r0; });      // a set reads one of two sources
    }
    m.store(partial, sp, red);
}

// a thread adds its pixels in pixel order and, per pixel, the planes p0 .. p1 - 1 in plane order
__global__ __launch_bounds__(256) void pooled_moments_kernel(const double* __restrict__ src, long plane_stride, int p0, int p1,
                                                             const uint8_t* __restrict__ cls,
                                                             const uint16_t* __restrict__ valid, long n, SetSpecs sp,
                                                             double* __restrict__ partial) {
    __shared__ double red[4][5];
    SetMoments m;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const unsigned c = cls[i];
        const unsigned v = valid ? (unsigned)valid[i] : 0xffffu;
        const double* q = src + (long)p0 * plane_stride + i;
        for (int p = p0; p < p1; ++p, q += plane_stride) {
            if (!((v >> p) & 1u)) continue;
            const double d = *q;
            m.add(sp, c, [&](int) { return d; });                           // every set reads the one value
        }
    }
    m.store(partial, sp, red);
}

// one block per set: fixed-order sum of the block partials (strided per thread, then a fixed tree) -> out[s*8 + 0..4];
// the selection states of the set's three medians (selectors s*3 + mode of the table: mode 0 median, 1 absolute median,
// 2 NMAD) start from its count
__global__ __launch_bounds__(256) void sets_moments_finish_kernel(const double* __restrict__ partial, int nb, int n_sets,
                                                                  double* __restrict__ out, SelState* __restrict__ st) {
    __shared__ double red[5][256];
    const int s = blockIdx.x, t = threadIdx.x;
    double cnt = 0.0, sa = 0.0, sq = 0.0, mn = INFINITY, mx = -INFINITY;
    for (int b = t; b < nb; b += 256) {
        const double* p = partial + ((long)b * n_sets + s) * 5;
        cnt += p[0];
        sa += p[1];
        sq += p[2];
        mn = fmin(mn, p[3]);
        mx = fmax(mx, p[4]);
    }
    red[0][t] = cnt; red[1][t] = sa; red[2][t] = sq; red[3][t] = mn; red[4][t] = mx;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) {
            red[0][t] += red[0][t + off];
            red[1][t] += red[1][t + off];
            red[2][t] += red[2][t + off];
            red[3][t] = fmin(red[3][t], red[3][t + off]);
            red[4][t] = fmax(red[4][t], red[4][t + off]);
        }
        __syncthreads();
    }
    if (t) return;
    cnt = red[0][0];
    const double nanv = __longlong_as_double(0x7ff8000000000000ll);
    double* o = out + s * 8;
    o[0] = cnt;
    o[1] = cnt > 0 ? red[4][0] : nanv;
    o[2] = cnt > 0 ? red[3][0] : nanv;
    o[3] = cnt > 0 ? red[1][0] / cnt : nanv;
    o[4] = cnt > 0 ? sqrt(red[2][0] / cnt) : nanv;
    const long long c = (long long)cnt;
    for (int m = 0; m < 3; ++m) {
        SelState& q = st[s * 3 + m];
        q.prefix[0] = q.prefix[1] = 0ull;
        q.rank[0] = (c - 1) / 2;
        q.rank[1] = c / 2;
        q.count = c;
        q.shift = 0.0;
    }
}

// NMAD selections centre on the set's absolute median
__global__ void sets_shift_kernel(const double* __restrict__ out, int n_sets, SelState* __restrict__ st) {
    const int s = threadIdx.x;
    if (s < n_sets) st[s * 3 + 2].shift = out[s * 8 + 5];
}

// up to SEL_GROUP selectors of one histogram pass.  A selector ranks the values of set(j) in value mode mode(j); its state is
// entry sel(j) of the call's selector table st[].  The eight-number calls lay their table out as set * 3 + mode (mode 0 median,
// 1 absolute median, 2 NMAD), the quantile calls as set * n_q + quantile.
// One word per selector (set | mode << 8 | sel << 16; 20 sets, 3 modes, 160 table entries fit): the histogram loop reads one
// scalar per selector and round where two arrays would cost two, and a pass of the medians measured 2 % shorter for it.
struct SelGroup {
    int n;
    unsigned code[SEL_GROUP];
    __host__ __device__ int set(int j) const { return (int)(code[j] & 255u); }
    __host__ __device__ int mode(int j) const { return (int)((code[j] >> 8) & 255u); }
    __host__ __device__ int sel(int j) const { return (int)(code[j] >> 16); }
    void put(int j, int set, int mode, int sel) { code[j] = (unsigned)set | (unsigned)mode << 8 | (unsigned)sel << 16; }
};

// The histogram kernels.  hist[j*512 + side*256 + bin]: the pass's byte histogram of selector j's values under each of its two
// prefixes; while the two prefixes agree both ranks read side 0 (the values are counted once).  A kernel holds HB pixels per
// thread in registers per round, so the selector parameters are read once per round, not per pixel.
__device__ __forceinline__ void hist_begin(unsigned* lh, unsigned long long (*pf)[2], double* sh, const SelGroup& g,
                                           const SelState* __restrict__ st) {
    for (int i = threadIdx.x; i < g.n * 512; i += blockDim.x) lh[i] = 0u;
    if (threadIdx.x < g.n) {
        const SelState& t = st[g.sel(threadIdx.x)];
        pf[threadIdx.x][0] = t.prefix[0];
        pf[threadIdx.x][1] = t.prefix[1];
        sh[threadIdx.x] = t.shift;
    }
    __syncthreads();
}

// one selector's histogram h over HB values r[] of class c[] (-1: no value there)
__device__ __forceinline__ void hist_count(unsigned* h, const double (&r)[HB], const int (&c)[HB], int need, double thr,
                                           int mode, double shift, unsigned long long p0, unsigned long long p1, int pass) {
    const int hs = 8 * (pass + 1);
#pragma unroll
    for (int u = 0; u < HB; ++u) {
        if (c[u] < 0 || (c[u] & need) != need || (thr > 0.0 && !(fabs(r[u]) <= thr))) continue;
        const unsigned long long k = key_of(pick_value(r[u], mode, shift));
        const unsigned long long hi = pass == 7 ? 0ull : (k >> hs);
        const unsigned b = (unsigned)((k >> (8 * pass)) & 255ull);
        if (hi == p0)
            atomicAdd(&h[b], 1u);
        else if (hi == p1)
            atomicAdd(&h[256 + b], 1u);
    }
}

__device__ __forceinline__ void hist_flush(const unsigned* lh, const SelGroup& g, unsigned* __restrict__ hist) {
    __syncthreads();
    for (int i = threadIdx.x; i < g.n * 512; i += blockDim.x)
        if (lh[i]) atomicAdd(&hist[i], lh[i]);
}

__global__ __launch_bounds__(512) void sets_hist_kernel(const double* __restrict__ src0, const double* __restrict__ src1,
                                                        const uint8_t* __restrict__ cls, long n, SetSpecs sp, SelGroup g,
                                                        int pass, const SelState* __restrict__ st,
                                                        unsigned* __restrict__ hist) {
    __shared__ unsigned lh[SEL_GROUP * 512];
    __shared__ unsigned long long pf[SEL_GROUP][2];
    __shared__ double sh[SEL_GROUP];
    hist_begin(lh, pf, sh, g, st);
    const long step = (long)gridDim.x * blockDim.x * HB;
    for (long base = (long)blockIdx.x * blockDim.x * HB + threadIdx.x; base < n; base += step) {
        double r0[HB], r1[HB];
        int c[HB];
#pragma unroll
        for (int u = 0; u < HB; ++u) {
            const long i = base + (long)u * blockDim.x;
            const bool ok = i < n;
            r0[u] = ok ? src0[i] : 0.0;
            r1[u] = ok ? src1[i] : 0.0;
            c[u] = ok ? (int)cls[i] : -1;
        }
        for (int j = 0; j < g.n; ++j) {
            const int s = g.set(j), src = sp.src[s];
            double r[HB];
#pragma unroll
            for (int u = 0; u < HB; ++u) r[u] = src ? r1[u] : r0[u];
            hist_count(lh + j * 512, r, c, (int)sp.need[s], sp.thr[s], g.mode(j), sh[j], pf[j][0], pf[j][1], pass);
        }
    }
    hist_flush(lh, g, hist);
}

// per round the class bytes and validity words of HB pixels are read once; per plane the HB values, and the class with the
// plane's validity folded in (-1 = skip)
__global__ __launch_bounds__(512) void pooled_hist_kernel(const double* __restrict__ src, long plane_stride, int p0, int p1,
                                                          const uint8_t* __restrict__ cls, const uint16_t* __restrict__ valid,
                                                          long n, SetSpecs sp, SelGroup g, int pass,
                                                          const SelState* __restrict__ st, unsigned* __restrict__ hist) {
    __shared__ unsigned lh[SEL_GROUP * 512];
    __shared__ unsigned long long pf[SEL_GROUP][2];
    __shared__ double sh[SEL_GROUP];
    hist_begin(lh, pf, sh, g, st);
    const long step = (long)gridDim.x * blockDim.x * HB;
    for (long base = (long)blockIdx.x * blockDim.x * HB + threadIdx.x; base < n; base += step) {
        int c0[HB];
        unsigned v[HB];
#pragma unroll
        for (int u = 0; u < HB; ++u) {
            const long i = base + (long)u * blockDim.x;
            const bool ok = i < n;
            c0[u] = ok ? (int)cls[i] : -1;
            v[u] = ok ? (valid ? (unsigned)valid[i] : 0xffffu) : 0u;
        }
        const double* q = src + (long)p0 * plane_stride;
        for (int p = p0; p < p1; ++p, q += plane_stride) {
            double r[HB];
            int c[HB];
#pragma unroll
            for (int u = 0; u < HB; ++u) {
                const long i = base + (long)u * blockDim.x;
                const bool ok = c0[u] >= 0 && ((v[u] >> p) & 1u);
                r[u] = ok ? q[i] : 0.0;
                c[u] = ok ? c0[u] : -1;
            }
            for (int j = 0; j < g.n; ++j) {
                const int s = g.set(j);
                hist_count(lh + j * 512, r, c, (int)sp.need[s], sp.thr[s], g.mode(j), sh[j], pf[j][0], pf[j][1], pass);
            }
        }
    }
    hist_flush(lh, g, hist);
}

// one block per selector: the bin holding each rank (block-wide inclusive scan), prefixes and ranks advance, the
// selector's histogram is cleared for the next pass
__global__ __launch_bounds__(256) void sets_pick_kernel(SelGroup g, SelState* __restrict__ st, unsigned* __restrict__ hist) {
    __shared__ unsigned long long scan[256];
    __shared__ int bin_of[2];
    __shared__ unsigned long long below_of[2];
    const int j = blockIdx.x, t = threadIdx.x;
    SelState& S = st[g.sel(j)];
    const bool same = S.prefix[0] == S.prefix[1];
    unsigned* h = hist + j * 512;
    for (int side = 0; side < 2; ++side) {
        const unsigned c = h[(side && !same ? 256 : 0) + t];
        scan[t] = c;
        if (t == 0) {
            bin_of[side] = 255;
            below_of[side] = 0;
        }
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const unsigned long long v = t >= o ? scan[t - o] : 0ull;
            __syncthreads();
            scan[t] += v;
            __syncthreads();
        }
        const unsigned long long incl = scan[t], excl = incl - c;
        const unsigned long long rank = (unsigned long long)S.rank[side];
        if (c && excl <= rank && rank < incl) {
            bin_of[side] = t;
            below_of[side] = excl;
        }
        __syncthreads();
    }
    if (t == 0) {
        for (int side = 0; side < 2; ++side) {
            S.prefix[side] = (S.prefix[side] << 8) | (unsigned long long)bin_of[side];
            S.rank[side] -= (long long)below_of[side];
        }
    }
    h[t] = 0u;
    h[256 + t] = 0u;
}

__global__ void sets_select_finish_kernel(SelGroup g, const SelState* __restrict__ st, double* __restrict__ out) {
    const int j = threadIdx.x;
    if (j >= g.n) return;
    const SelState& S = st[g.sel(j)];
    const int m = g.mode(j);
    const double nanv = __longlong_as_double(0x7ff8000000000000ll);
    const double scale = m == 2 ? 1.4826 : 1.0;
    out[g.set(j) * 8 + (m == 1 ? 5 : (m == 0 ? 6 : 7))] =
        S.count > 0 ? scale * (0.5 * (unkey(S.prefix[0]) + unkey(S.prefix[1]))) : nanv;
}

__global__ void sets_zero_kernel(unsigned* __restrict__ p, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) p[i] = 0u;
}

// ---- host side of the two forms ----
static void fill_rects(EvalRects& area, const int* rects, int n_rects) {
    area.n = n_rects;
    for (int q = 0; q < n_rects; ++q)
        for (int e = 0; e < 4; ++e) area.r[q][e] = rects[q * 4 + e];
}
static dim3 classify_grid(int rows, int cols) { return dim3((cols + 255) / 256, rows < 65535 ? rows : 65535); }

// set_src == nullptr: every set reads source 0
static void fill_specs(SetSpecs& sp, int n_sets, const int* set_src, const int* set_need, const double* set_thr) {
    sp.n = n_sets;
    for (int i = 0; i < RD_STATS_MAX_SETS; ++i) {
        sp.src[i] = i < n_sets && set_src ? set_src[i] : 0;
        sp.need[i] = i < n_sets ? (unsigned)set_need[i] : 0u;
        sp.thr[i] = i < n_sets ? set_thr[i] : -1.0;
    }
}

static int sets_moment_blocks(long n) {
    long g = (n + 255) / 256;
    return (int)(g > 1024 ? 1024 : (g < 1 ? 1 : g));
}
static int sets_hist_blocks(long n) {
    long g = (n + 512 * HB - 1) / (512 * HB);
    return (int)(g > 1024 ? 1024 : (g < 1 ? 1 : g));
}

// the workspace of a statistics call: block partials | selection states | histograms
struct StatsWs {
    double* partial;
    SelState* st;
    unsigned* hist;
};
// -> the bytes a call over n values needs; with w, the layout carved from ws
static size_t stats_ws_layout(long n, void* ws = nullptr, StatsWs* w = nullptr) {
    const size_t o_st = (size_t)sets_moment_blocks(n) * RD_STATS_MAX_SETS * 5 * sizeof(double);
    const size_t o_hist = o_st + (size_t)RD_STATS_MAX_SETS * 3 * sizeof(SelState);
    if (w) *w = StatsWs{(double*)ws, (SelState*)((char*)ws + o_st), (unsigned*)((char*)ws + o_hist)};
    return o_hist + (size_t)SEL_GROUP * 512 * sizeof(unsigned) + 256;
}

// the most groups a call schedules: the medians' two phases (2 x n_sets and n_sets selectors, each rounded up to whole groups)
// or the RD_STATS_MAX_SETS x RD_DIST_MAX_Q selectors of a quantile call
constexpr int MAX_GROUPS = (RD_STATS_MAX_SETS * RD_DIST_MAX_Q + SEL_GROUP - 1) / SEL_GROUP;
static_assert(MAX_GROUPS >= 3 * RD_STATS_MAX_SETS / SEL_GROUP + 3, "the medians' groups must fit");

// selectors: every set's median and absolute median (phase 0), then every set's NMAD (phase 1), SEL_GROUP per pass
struct SelectPlan {
    SelGroup groups[MAX_GROUPS];
    int phase_end[2], ng;
};
static SelectPlan make_select_plan(int n_sets) {
    SelectPlan plan;
    plan.ng = 0;
    for (int phase = 0; phase < 2; ++phase) {
        const int nsel = phase == 0 ? 2 * n_sets : n_sets;
        for (int j0 = 0; j0 < nsel; j0 += SEL_GROUP) {
            SelGroup& g = plan.groups[plan.ng++];
            g.n = nsel - j0 < SEL_GROUP ? nsel - j0 : SEL_GROUP;
            for (int j = 0; j < SEL_GROUP; ++j) {
                const int q = j0 + (j < g.n ? j : 0);
                const int set = phase == 0 ? q >> 1 : q, mode = phase == 0 ? (q & 1) : 2;
                g.put(j, set, mode, set * 3 + mode);
            }
        }
        plan.phase_end[phase] = plan.ng;
    }
    return plan;
}

// the schedule of one group, whatever its selectors stand for: 8 x (launch_hist(group, pass), pick), then finish(group)
template <class LaunchHist, class Finish>
static void run_group(hipStream_t s, const SelGroup& g, SelState* st, unsigned* hist, LaunchHist launch_hist, Finish finish) {
    for (int pass = 7; pass >= 0; --pass) {
        launch_hist(g, pass);
        RD_LAUNCH(sets_pick_kernel, dim3(g.n), dim3(256), 0, s, g, st, hist);
    }
    finish(g);
}

// the medians, per group: [the NMAD shifts before the first group of phase 1,] run_group with the medians' finish
template <class LaunchHist>
static void run_selection(hipStream_t s, const SelectPlan& plan, int n_sets, double* out, SelState* st, unsigned* hist,
                          LaunchHist launch_hist) {
    for (int gi = 0; gi < plan.ng; ++gi) {
        if (gi == plan.phase_end[0]) RD_LAUNCH(sets_shift_kernel, dim3(1), dim3(64), 0, s, (const double*)out, n_sets, st);
        run_group(s, plan.groups[gi], st, hist, launch_hist, [&](const SelGroup& g) {
            RD_LAUNCH(sets_select_finish_kernel, dim3(1), dim3(64), 0, s, g, (const SelState*)st, out);
        });
    }
}

}  // namespace rd

extern "C" {

int rd_dilate_mask(const uint8_t* in, uint8_t* out, int rows, int cols, int iterations, rd_stream_t s_) {
    RD_REQUIRE(in && out && in != out && rows > 0 && cols > 0, "rd_dilate_mask: bad arguments");
    RD_REQUIRE(iterations >= 1 && iterations <= RD_DILATE_MAX_ITER, "rd_dilate_mask: iterations %d outside 1..%d",
               iterations, RD_DILATE_MAX_ITER);
    hipStream_t s = (hipStream_t)s_;
    ProfScope ps(s, "dilate_mask", 0, 2.0 * rows * cols);
    const dim3 grid((cols + DIL_TW - 1) / DIL_TW, (rows + DIL_TH - 1) / DIL_TH);
    RD_LAUNCH(dilate_kernel, grid, dim3(256), 0, s, in, out, rows, cols, iterations);
    RD_LAUNCH_CHECK("dilate_mask");
    return RD_OK;
}

int rd_eval_classify(const double* prediction, const void* initial, int initial_f64, const void* gt, int gt_f64,
                     const uint8_t* gt_mask, const uint8_t* building, const uint8_t* building_nodata,
                     const uint8_t* water, const uint8_t* forest, const int* rects, int n_rects, int rows, int cols,
                     double nodata, double* r_before, double* r_after, uint8_t* cls, rd_stream_t s_) {
    RD_REQUIRE(prediction && initial && gt && r_before && r_after && cls && rows > 0 && cols > 0,
               "rd_eval_classify: bad arguments");
    RD_REQUIRE(n_rects <= RD_EVAL_MAX_RECTS && (n_rects <= 0 || rects), "rd_eval_classify: %d area rectangles (at most %d)",
               n_rects, RD_EVAL_MAX_RECTS);
    EvalRects area;
    fill_rects(area, rects, n_rects);
    hipStream_t s = (hipStream_t)s_;
    const double n = (double)rows * cols;
    ProfScope ps(s, "eval_classify", 0, n * (8.0 + (initial_f64 ? 8 : 4) + (gt_f64 ? 8 : 4) + 16.0 + 1.0));
    RD_LAUNCH(eval_classify_kernel, classify_grid(rows, cols), dim3(256), 0, s, prediction, initial, initial_f64 ? 1 : 0, gt,
              gt_f64 ? 1 : 0, gt_mask, building, building_nodata, water, forest, area, rows, cols, nodata, r_before, r_after,
              cls);
    RD_LAUNCH_CHECK("eval_classify");
    return RD_OK;
}

int rd_eval_classify_planes(const double* planes, long long plane_stride, int n_planes, const double* extra,
                            const void* initial, int initial_f64, const void* gt, int gt_f64, const uint8_t* gt_mask,
                            const uint8_t* building, const uint8_t* building_nodata, const uint8_t* water,
                            const uint8_t* forest, const int* rects, int n_rects, int rows, int cols, double nodata,
                            double* r_before, double* residuals, double* r_extra, uint8_t* cls, uint16_t* valid,
                            rd_stream_t s_) {
    RD_REQUIRE(planes && initial && gt && residuals && cls && valid && rows > 0 && cols > 0,
               "rd_eval_classify_planes: bad arguments");
    RD_REQUIRE(n_planes >= 1 && n_planes <= RD_EVAL_MAX_PLANES, "rd_eval_classify_planes: n_planes must be in 1..%d (got %d)",
               RD_EVAL_MAX_PLANES, n_planes);
    RD_REQUIRE(plane_stride >= (long long)rows * cols, "rd_eval_classify_planes: plane_stride %lld < rows * cols = %lld",
               plane_stride, (long long)rows * cols);
    RD_REQUIRE(!extra == !r_extra, "rd_eval_classify_planes: extra and r_extra come together");
    RD_REQUIRE(n_rects <= RD_EVAL_MAX_RECTS && (n_rects <= 0 || rects),
               "rd_eval_classify_planes: %d area rectangles (at most %d)", n_rects, RD_EVAL_MAX_RECTS);
    EvalRects area;
    fill_rects(area, rects, n_rects);
    hipStream_t s = (hipStream_t)s_;
    const double n = (double)rows * cols;
    ProfScope ps(s, "eval_classify_planes", 0,
                 n * (16.0 * (n_planes + (extra ? 1 : 0)) + (initial_f64 ? 8 : 4) + (gt_f64 ? 8 : 4) + (r_before ? 8.0 : 0.0) + 3.0));
    RD_LAUNCH(eval_classify_planes_kernel, classify_grid(rows, cols), dim3(256), 0, s, planes, (long)plane_stride, n_planes,
              extra, initial, initial_f64 ? 1 : 0, gt, gt_f64 ? 1 : 0, gt_mask, building, building_nodata, water, forest, area,
              rows, cols, nodata, r_before, residuals, r_extra, cls, valid);
    RD_LAUNCH_CHECK("eval_classify_planes");
    return RD_OK;
}

size_t rd_residual_stats_sets_ws_bytes(long long n, int n_sets) { return stats_ws_layout(n); }

int rd_residual_stats_sets(const double* src0, const double* src1, const uint8_t* cls, long long n, const int* set_src,
                           const int* set_need, const double* set_thr, int n_sets, double* out, void* ws,
                           size_t ws_bytes, rd_stream_t s_) {
    RD_REQUIRE(src0 && cls && out && n > 0 && set_src && set_need && set_thr, "rd_residual_stats_sets: bad arguments");
    RD_REQUIRE(n_sets >= 1 && n_sets <= RD_STATS_MAX_SETS, "rd_residual_stats_sets: %d sets (1..%d)", n_sets,
               RD_STATS_MAX_SETS);
    if (!ws || ws_bytes < rd_residual_stats_sets_ws_bytes(n, n_sets)) {
        set_error("rd_residual_stats_sets: workspace too small (%zu < %zu)", ws_bytes,
                  rd_residual_stats_sets_ws_bytes(n, n_sets));
        return RD_ERR_WS;
    }
    SetSpecs sp;
    fill_specs(sp, n_sets, set_src, set_need, set_thr);
    for (int i = 0; i < n_sets; ++i)
        RD_REQUIRE(sp.src[i] == 0 || (sp.src[i] == 1 && src1), "rd_residual_stats_sets: set %d reads source %d", i,
                   sp.src[i]);
    if (!src1) src1 = src0;
    hipStream_t s = (hipStream_t)s_;
    const int nbm = sets_moment_blocks(n), nbh = sets_hist_blocks(n);
    StatsWs w;
    stats_ws_layout(n, ws, &w);
    const SelectPlan plan = make_select_plan(n_sets);
    ProfScope ps(s, "residual_stats_sets", 0, 17.0 * n * (1 + 8 * plan.ng));
    RD_LAUNCH(sets_zero_kernel, dim3(1), dim3(256), 0, s, w.hist, SEL_GROUP * 512);
    RD_LAUNCH(sets_moments_kernel, dim3(nbm), dim3(256), 0, s, src0, src1, cls, (long)n, sp, w.partial);
    RD_LAUNCH(sets_moments_finish_kernel, dim3(n_sets), dim3(256), 0, s, (const double*)w.partial, nbm, n_sets, out, w.st);
    run_selection(s, plan, n_sets, out, w.st, w.hist, [&](const SelGroup& g, int pass) {
        RD_LAUNCH(sets_hist_kernel, dim3(nbh), dim3(512), 0, s, src0, src1, cls, (long)n, sp, g, pass, (const SelState*)w.st,
                  w.hist);
    });
    RD_LAUNCH_CHECK("residual_stats_sets");
    return RD_OK;
}

size_t rd_residual_stats_pooled_ws_bytes(long long n, int n_sets) { return rd_residual_stats_sets_ws_bytes(n, n_sets); }

int rd_residual_stats_pooled(const double* src, long long plane_stride, int n_planes, int p0, int p1, const uint8_t* cls,
                             const uint16_t* valid, long long n, const int* set_need, const double* set_thr, int n_sets,
                             double* out, void* ws, size_t ws_bytes, rd_stream_t s_) {
    RD_REQUIRE(src && cls && out && n > 0 && set_need && set_thr, "rd_residual_stats_pooled: bad arguments");
    RD_REQUIRE(n_planes >= 1 && n_planes <= RD_EVAL_MAX_PLANES, "rd_residual_stats_pooled: n_planes must be in 1..%d (got %d)",
               RD_EVAL_MAX_PLANES, n_planes);
    RD_REQUIRE(p0 >= 0 && p0 < p1 && p1 <= n_planes, "rd_residual_stats_pooled: planes [%d, %d) outside the %d planes", p0, p1,
               n_planes);
    RD_REQUIRE(plane_stride >= n, "rd_residual_stats_pooled: plane_stride %lld < n = %lld", plane_stride, n);
    RD_REQUIRE(n_sets >= 1 && n_sets <= RD_STATS_MAX_SETS, "rd_residual_stats_pooled: %d sets (1..%d)", n_sets,
               RD_STATS_MAX_SETS);
    // the histograms are 32-bit counters: a bin may hold every member of a set
    RD_REQUIRE(n < (1ll << 32) && (long long)(p1 - p0) * n < (1ll << 32),
               "rd_residual_stats_pooled: (p1 - p0) * n = %d * %lld values reach 2^32 (32-bit histogram counters)", p1 - p0, n);
    if (!ws || ws_bytes < rd_residual_stats_pooled_ws_bytes(n, n_sets)) {
        set_error("rd_residual_stats_pooled: workspace too small (%zu < %zu)", ws_bytes,
                  rd_residual_stats_pooled_ws_bytes(n, n_sets));
        return RD_ERR_WS;
    }
    SetSpecs sp;
    fill_specs(sp, n_sets, nullptr, set_need, set_thr);
    hipStream_t s = (hipStream_t)s_;
    const int nbm = sets_moment_blocks(n), nbh = sets_hist_blocks(n);
    StatsWs w;
    stats_ws_layout(n, ws, &w);
    const SelectPlan plan = make_select_plan(n_sets);
    const double pass_bytes = (double)n * (8.0 * (p1 - p0) + 1.0 + (valid ? 2.0 : 0.0));
    {
        ProfScope ps(s, "residual_stats_pooled|moments", 0, pass_bytes);
        RD_LAUNCH(sets_zero_kernel, dim3(1), dim3(256), 0, s, w.hist, SEL_GROUP * 512);
        RD_LAUNCH(pooled_moments_kernel, dim3(nbm), dim3(256), 0, s, src, (long)plane_stride, p0, p1, cls, valid, (long)n, sp,
                  w.partial);
        RD_LAUNCH(sets_moments_finish_kernel, dim3(n_sets), dim3(256), 0, s, (const double*)w.partial, nbm, n_sets, out, w.st);
    }
    // one profiler class per width of the pool, so a single-plane pass and a pooled pass are timed apart
    char cls_name[48];
    snprintf(cls_name, sizeof cls_name, "residual_stats_pooled|select x%d", p1 - p0);
    ProfScope ps(s, cls_name, 0, pass_bytes * 8 * plan.ng);
    run_selection(s, plan, n_sets, out, w.st, w.hist, [&](const SelGroup& g, int pass) {
        RD_LAUNCH(pooled_hist_kernel, dim3(nbh), dim3(512), 0, s, src, (long)plane_stride, p0, p1, cls, valid, (long)n, sp, g,
                  pass, (const SelState*)w.st, w.hist);
    });
    RD_LAUNCH_CHECK("residual_stats_pooled");
    return RD_OK;
}

}  // extern "C"

// ---- quantiles and within-tolerance shares of the same sets (include/resdepth_hip_dist.h) -------------------------------
// The two forms again, on the same engine.  One counting pass gives every set's member count and, per tolerance, the number of
// members with |r| <= tau: integers all the way (a wave's ballot is counted with popcount, one lane adds the wave's number to
// the block's 32-bit LDS counter, a block adds its counters to the call's 64-bit ones with integer atomics), so the same input
// gives the same bits whatever the schedule.  dist_prepare_kernel turns each count into the shares and into the two ranks and
// the weight of every quantile -- a quantile is one more selector of the radix select: value mode 0 or 1, ranks lo and hi,
// selector set * n_q + j of the table -- and the groups of SEL_GROUP selectors run through hist_begin / hist_count / hist_flush,
// sets_pick_kernel and run_group as the medians do.  dist_finish_kernel interpolates.
namespace rd {

struct DistTaus {
    int n;
    double tau[RD_DIST_MAX_T];
};
struct DistLevels {
    int n;
    double q[RD_DIST_MAX_Q];
    int mode[RD_DIST_MAX_Q];
};
constexpr int DIST_COUNTERS = RD_STATS_MAX_SETS * (1 + RD_DIST_MAX_T);

// lc[s * (1 + tt.n)]: members of set s among a wave's HB x 64 values; lc[s * (1 + tt.n) + 1 + k]: those with |r| <= tau[k].
// value_of(s, u): what set s reads at the thread's u-th value; c[u] < 0: no value there.  Every lane of the wave is here.
template <class ValueOf>
__device__ __forceinline__ void dist_count(unsigned* lc, const SetSpecs& sp, const DistTaus& tt, const int (&c)[HB],
                                           ValueOf value_of) {
    const bool first = (threadIdx.x & 63) == 0;
    for (int s = 0; s < sp.n; ++s) {
        const int need = (int)sp.need[s];
        const double thr = sp.thr[s];
        unsigned member = 0u, cnt = 0u;
#pragma unroll
        for (int u = 0; u < HB; ++u) {
            const bool m = c[u] >= 0 && (c[u] & need) == need && !(thr > 0.0 && !(fabs(value_of(s, u)) <= thr));
            member |= (m ? 1u : 0u) << u;
            cnt += (unsigned)__popcll(__ballot(m));
        }
        if (cnt == 0u) continue;                       // wave-uniform
        unsigned* o = lc + s * (1 + tt.n);
        if (first) atomicAdd(o, cnt);
        for (int k = 0; k < tt.n; ++k) {
            const double tau = tt.tau[k];
            unsigned w = 0u;
#pragma unroll
            for (int u = 0; u < HB; ++u) w += (unsigned)__popcll(__ballot(((member >> u) & 1u) && fabs(value_of(s, u)) <= tau));
            if (w && first) atomicAdd(o + 1 + k, w);
        }
    }
}

__device__ __forceinline__ void dist_count_begin(unsigned* lc) {
    for (int i = threadIdx.x; i < DIST_COUNTERS; i += blockDim.x) lc[i] = 0u;
    __syncthreads();
}
__device__ __forceinline__ void dist_count_flush(const unsigned* lc, int n_counters, unsigned long long* __restrict__ total) {
    __syncthreads();
    for (int i = threadIdx.x; i < n_counters; i += blockDim.x)
        if (lc[i]) atomicAdd(&total[i], (unsigned long long)lc[i]);
}

// the rounds are those of sets_hist_kernel, with a block-uniform loop: every lane of a wave reaches every ballot
__global__ __launch_bounds__(512) void sets_dist_count_kernel(const double* __restrict__ src0, const double* __restrict__ src1,
                                                              const uint8_t* __restrict__ cls, long n, SetSpecs sp, DistTaus tt,
                                                              unsigned long long* __restrict__ total) {
    __shared__ unsigned lc[DIST_COUNTERS];
    dist_count_begin(lc);
    const long step = (long)gridDim.x * blockDim.x * HB;
    for (long b0 = (long)blockIdx.x * blockDim.x * HB; b0 < n; b0 += step) {
        double r0[HB], r1[HB];
        int c[HB];
#pragma unroll
        for (int u = 0; u < HB; ++u) {
            const long i = b0 + threadIdx.x + (long)u * blockDim.x;
            const bool ok = i < n;
            r0[u] = ok ? src0[i] : 0.0;
            r1[u] = ok ? src1[i] : 0.0;
            c[u] = ok ? (int)cls[i] : -1;
        }
        dist_count(lc, sp, tt, c, [&](int s, int u) { return sp.src[s] ? r1[u] : r0[u]; });
    }
    dist_count_flush(lc, sp.n * (1 + tt.n), total);
}

// the rounds are those of pooled_hist_kernel: class bytes and validity words once per round, the plane loop outside
__global__ __launch_bounds__(512) void pooled_dist_count_kernel(const double* __restrict__ src, long plane_stride, int p0, int p1,
                                                                const uint8_t* __restrict__ cls,
                                                                const uint16_t* __restrict__ valid, long n, SetSpecs sp,
                                                                DistTaus tt, unsigned long long* __restrict__ total) {
    __shared__ unsigned lc[DIST_COUNTERS];
    dist_count_begin(lc);
    const long step = (long)gridDim.x * blockDim.x * HB;
    for (long b0 = (long)blockIdx.x * blockDim.x * HB; b0 < n; b0 += step) {
        int c0[HB];
        unsigned v[HB];
#pragma unroll
        for (int u = 0; u < HB; ++u) {
            const long i = b0 + threadIdx.x + (long)u * blockDim.x;
            const bool ok = i < n;
            c0[u] = ok ? (int)cls[i] : -1;
            v[u] = ok ? (valid ? (unsigned)valid[i] : 0xffffu) : 0u;
        }
        const double* q = src + (long)p0 * plane_stride;
        for (int p = p0; p < p1; ++p, q += plane_stride) {
            double r[HB];
            int c[HB];
#pragma unroll
            for (int u = 0; u < HB; ++u) {
                const long i = b0 + threadIdx.x + (long)u * blockDim.x;
                const bool ok = c0[u] >= 0 && ((v[u] >> p) & 1u);
                r[u] = ok ? q[i] : 0.0;
                c[u] = ok ? c0[u] : -1;
            }
            dist_count(lc, sp, tt, c, [&](int, int u) { return r[u]; });
        }
    }
    dist_count_flush(lc, sp.n * (1 + tt.n), total);
}

// one thread per set: out row = count, [quantiles: the finish kernel's], shares; selector set * n_q + j gets the ranks
// lo = floor(h), hi = lo + (g > 0) of h = fl((c - 1) * q_j) and the weight g = h - lo (exact: h < 2^53 has no more fraction
// bits than fit), all from the count that exists only here
__global__ void dist_prepare_kernel(const unsigned long long* __restrict__ total, int n_sets, DistLevels lv, int n_t,
                                    double* __restrict__ out, SelState* __restrict__ st, double* __restrict__ weight) {
    const int s = threadIdx.x;
    if (s >= n_sets) return;
    const double nanv = __longlong_as_double(0x7ff8000000000000ll);
    const unsigned long long* t = total + s * (1 + n_t);
    const long long c = (long long)t[0];
    double* o = out + (long)s * (1 + lv.n + n_t);
    o[0] = (double)c;
    for (int k = 0; k < n_t; ++k) o[1 + lv.n + k] = c > 0 ? (double)t[1 + k] / (double)c : nanv;
    for (int j = 0; j < lv.n; ++j) {
        const double h = c > 0 ? __dmul_rn((double)(c - 1), lv.q[j]) : 0.0;
        const double lo = floor(h), g = h - lo;
        SelState& q = st[s * lv.n + j];
        q.prefix[0] = q.prefix[1] = 0ull;
        q.rank[0] = (long long)lo;
        q.rank[1] = (long long)lo + (g > 0.0 ? 1 : 0);
        q.count = c;
        q.shift = 0.0;
        weight[s * lv.n + j] = g;
    }
}

// Q = v_lo when the weight is zero, else v_lo + g * (v_hi - v_lo) in three separately rounded operations (never contracted)
__global__ void dist_finish_kernel(SelGroup g, const SelState* __restrict__ st, const double* __restrict__ weight, int n_q,
                                   int row, double* __restrict__ out) {
    const int j = threadIdx.x;
    if (j >= g.n) return;
    const SelState& S = st[g.sel(j)];
    const double nanv = __longlong_as_double(0x7ff8000000000000ll);
    const double w = weight[g.sel(j)], lo = unkey(S.prefix[0]), hi = unkey(S.prefix[1]);
    const double v = w == 0.0 ? lo : __dadd_rn(lo, __dmul_rn(w, __dsub_rn(hi, lo)));
    out[(long)g.set(j) * row + 1 + (g.sel(j) - g.set(j) * n_q)] = S.count > 0 ? v : nanv;
}

// the workspace of a quantile call: histograms | 64-bit counters | selection states | weights.  The histograms and the counters
// lie together: one launch clears both.
struct DistWs {
    unsigned* hist;
    unsigned long long* total;
    SelState* st;
    double* weight;
};
constexpr int DIST_ZERO_WORDS = SEL_GROUP * 512 + 2 * DIST_COUNTERS;
static size_t dist_ws_layout(void* ws = nullptr, DistWs* w = nullptr) {
    const size_t o_total = (size_t)SEL_GROUP * 512 * sizeof(unsigned);
    const size_t o_st = o_total + (size_t)DIST_COUNTERS * sizeof(unsigned long long);
    const size_t o_w = o_st + (size_t)RD_STATS_MAX_SETS * RD_DIST_MAX_Q * sizeof(SelState);
    if (w) *w = DistWs{(unsigned*)ws, (unsigned long long*)((char*)ws + o_total), (SelState*)((char*)ws + o_st),
                       (double*)((char*)ws + o_w)};
    return o_w + (size_t)RD_STATS_MAX_SETS * RD_DIST_MAX_Q * sizeof(double) + 256;
}

// what both forms refuse, nothing launched
static int dist_check(const char* who, int n_sets, const double* q, const int* q_mode, int n_q, const double* tau, int n_t,
                      DistLevels& lv, DistTaus& tt) {
    RD_REQUIRE(n_sets >= 1 && n_sets <= RD_STATS_MAX_SETS, "%s: %d sets (1..%d)", who, n_sets, RD_STATS_MAX_SETS);
    RD_REQUIRE(n_q >= 0 && n_q <= RD_DIST_MAX_Q && n_t >= 0 && n_t <= RD_DIST_MAX_T && n_q + n_t > 0,
               "%s: %d quantiles (0..%d) and %d tolerances (0..%d), at least one of either", who, n_q, RD_DIST_MAX_Q, n_t,
               RD_DIST_MAX_T);
    RD_REQUIRE((n_q == 0 || (q && q_mode)) && (n_t == 0 || tau), "%s: bad arguments", who);
    lv.n = n_q;
    tt.n = n_t;
    for (int j = 0; j < RD_DIST_MAX_Q; ++j) {
        lv.q[j] = j < n_q ? q[j] : 0.0;
        lv.mode[j] = j < n_q ? q_mode[j] : 0;
        // !(a && b) also catches a NaN level
        RD_REQUIRE(lv.q[j] >= 0.0 && lv.q[j] <= 1.0, "%s: level %d = %g outside [0, 1]", who, j, lv.q[j]);
        RD_REQUIRE(lv.mode[j] == 0 || lv.mode[j] == 1, "%s: mode %d = %d (0: residual, 1: |residual|)", who, j, lv.mode[j]);
    }
    for (int k = 0; k < RD_DIST_MAX_T; ++k) {
        tt.tau[k] = k < n_t ? tau[k] : 0.0;
        RD_REQUIRE(tt.tau[k] >= 0.0 && tt.tau[k] <= 1.7976931348623157e308, "%s: tolerance %d = %g negative or not finite", who,
                   k, tt.tau[k]);
    }
    return RD_OK;
}

// the selectors j0 .. of the table set * n_q + quantile, SEL_GROUP per group
static SelGroup dist_group(int n_sets, const DistLevels& lv, int j0) {
    SelGroup g;
    const int nsel = n_sets * lv.n;
    g.n = nsel - j0 < SEL_GROUP ? nsel - j0 : SEL_GROUP;
    for (int j = 0; j < SEL_GROUP; ++j) {
        const int q = j0 + (j < g.n ? j : 0);
        g.put(j, q / lv.n, lv.mode[q % lv.n], q);
    }
    return g;
}

// after the form's counting pass: shares and ranks, then the groups
template <class LaunchHist>
static void run_dist(hipStream_t s, int n_sets, const DistLevels& lv, int n_t, double* out, const DistWs& w,
                     LaunchHist launch_hist) {
    RD_LAUNCH(dist_prepare_kernel, dim3(1), dim3(64), 0, s, (const unsigned long long*)w.total, n_sets, lv, n_t, out, w.st,
              w.weight);
    for (int j0 = 0; j0 < n_sets * lv.n; j0 += SEL_GROUP)
        run_group(s, dist_group(n_sets, lv, j0), w.st, w.hist, launch_hist, [&](const SelGroup& g) {
            RD_LAUNCH(dist_finish_kernel, dim3(1), dim3(64), 0, s, g, (const SelState*)w.st, (const double*)w.weight, lv.n,
                      1 + lv.n + n_t, out);
        });
}

}  // namespace rd

extern "C" {

size_t rd_residual_dist_sets_ws_bytes(long long n, int n_sets, int n_q, int n_t) { return dist_ws_layout(); }

int rd_residual_dist_sets(const double* src0, const double* src1, const uint8_t* cls, long long n, const int* set_src,
                          const int* set_need, const double* set_thr, int n_sets, const double* q, const int* q_mode, int n_q,
                          const double* tau, int n_t, double* out, void* ws, size_t ws_bytes, rd_stream_t s_) {
    RD_REQUIRE(src0 && cls && out && n > 0 && set_src && set_need && set_thr, "rd_residual_dist_sets: bad arguments");
    DistLevels lv;
    DistTaus tt;
    if (const int rc = dist_check("rd_residual_dist_sets", n_sets, q, q_mode, n_q, tau, n_t, lv, tt)) return rc;
    // 32-bit histogram counters, as in the pooled form
    RD_REQUIRE(n < (1ll << 32), "rd_residual_dist_sets: n = %lld values reach 2^32 (32-bit histogram counters)", n);
    SetSpecs sp;
    fill_specs(sp, n_sets, set_src, set_need, set_thr);
    for (int i = 0; i < n_sets; ++i)
        RD_REQUIRE(sp.src[i] == 0 || (sp.src[i] == 1 && src1), "rd_residual_dist_sets: set %d reads source %d", i, sp.src[i]);
    if (!ws || ws_bytes < dist_ws_layout()) {
        set_error("rd_residual_dist_sets: workspace too small (%zu < %zu)", ws_bytes, dist_ws_layout());
        return RD_ERR_WS;
    }
    if (!src1) src1 = src0;
    hipStream_t s = (hipStream_t)s_;
    const int nbh = sets_hist_blocks(n);
    DistWs w;
    dist_ws_layout(ws, &w);
    const int ng = (n_sets * n_q + SEL_GROUP - 1) / SEL_GROUP;
    ProfScope ps(s, "residual_dist_sets", 0, 17.0 * n * (1 + 8 * ng));
    RD_LAUNCH(sets_zero_kernel, dim3(1), dim3(256), 0, s, w.hist, DIST_ZERO_WORDS);
    RD_LAUNCH(sets_dist_count_kernel, dim3(nbh), dim3(512), 0, s, src0, src1, cls, (long)n, sp, tt, w.total);
    run_dist(s, n_sets, lv, n_t, out, w, [&](const SelGroup& g, int pass) {
        RD_LAUNCH(sets_hist_kernel, dim3(nbh), dim3(512), 0, s, src0, src1, cls, (long)n, sp, g, pass, (const SelState*)w.st,
                  w.hist);
    });
    RD_LAUNCH_CHECK("residual_dist_sets");
    return RD_OK;
}

size_t rd_residual_dist_pooled_ws_bytes(long long n, int n_sets, int n_q, int n_t) { return dist_ws_layout(); }

int rd_residual_dist_pooled(const double* src, long long plane_stride, int n_planes, int p0, int p1, const uint8_t* cls,
                            const uint16_t* valid, long long n, const int* set_need, const double* set_thr, int n_sets,
                            const double* q, const int* q_mode, int n_q, const double* tau, int n_t, double* out, void* ws,
                            size_t ws_bytes, rd_stream_t s_) {
    RD_REQUIRE(src && cls && out && n > 0 && set_need && set_thr, "rd_residual_dist_pooled: bad arguments");
    RD_REQUIRE(n_planes >= 1 && n_planes <= RD_EVAL_MAX_PLANES, "rd_residual_dist_pooled: n_planes must be in 1..%d (got %d)",
               RD_EVAL_MAX_PLANES, n_planes);
    RD_REQUIRE(p0 >= 0 && p0 < p1 && p1 <= n_planes, "rd_residual_dist_pooled: planes [%d, %d) outside the %d planes", p0, p1,
               n_planes);
    RD_REQUIRE(plane_stride >= n, "rd_residual_dist_pooled: plane_stride %lld < n = %lld", plane_stride, n);
    DistLevels lv;
    DistTaus tt;
    if (const int rc = dist_check("rd_residual_dist_pooled", n_sets, q, q_mode, n_q, tau, n_t, lv, tt)) return rc;
    RD_REQUIRE(n < (1ll << 32) && (long long)(p1 - p0) * n < (1ll << 32),
               "rd_residual_dist_pooled: (p1 - p0) * n = %d * %lld values reach 2^32 (32-bit histogram counters)", p1 - p0, n);
    if (!ws || ws_bytes < dist_ws_layout()) {
        set_error("rd_residual_dist_pooled: workspace too small (%zu < %zu)", ws_bytes, dist_ws_layout());
        return RD_ERR_WS;
    }
    SetSpecs sp;
    fill_specs(sp, n_sets, nullptr, set_need, set_thr);
    hipStream_t s = (hipStream_t)s_;
    const int nbh = sets_hist_blocks(n);
    DistWs w;
    dist_ws_layout(ws, &w);
    const int ng = (n_sets * n_q + SEL_GROUP - 1) / SEL_GROUP;
    ProfScope ps(s, "residual_dist_pooled", 0, (double)n * (8.0 * (p1 - p0) + 1.0 + (valid ? 2.0 : 0.0)) * (1 + 8 * ng));
    RD_LAUNCH(sets_zero_kernel, dim3(1), dim3(256), 0, s, w.hist, DIST_ZERO_WORDS);
    RD_LAUNCH(pooled_dist_count_kernel, dim3(nbh), dim3(512), 0, s, src, (long)plane_stride, p0, p1, cls, valid, (long)n, sp, tt,
              w.total);
    run_dist(s, n_sets, lv, n_t, out, w, [&](const SelGroup& g, int pass) {
        RD_LAUNCH(pooled_hist_kernel, dim3(nbh), dim3(512), 0, s, src, (long)plane_stride, p0, p1, cls, valid, (long)n, sp, g,
                  pass, (const SelState*)w.st, w.hist);
    });
    RD_LAUNCH_CHECK("residual_dist_pooled");
    return RD_OK;
}

}  // extern "C"

// ---- per-pixel fusion of P rasters of one surface (rd_fuse_planes, include/resdepth_hip_pairs.h) -----------------------
// A streaming kernel: P x 8 bytes in, 8 or 16 out per pixel.  A thread takes TWO neighbouring pixels, so every plane is read
// with one 16-byte non-temporal load per thread (8-byte accesses reach 0.54-0.70 of the 16-byte rate on this part) and the
// outputs leave as 16-byte stores; the P loads of a thread are independent and in flight together.  The 2 x P values live
// in registers: the kernel is a template on P and every index below is a compile-time constant -- the sorting network is a
// constexpr table applied through an index sequence, because an array indexed by a runtime value goes to scratch
// (scripts/check_isa.sh fails the build on any).  The modes are wave-uniform branches.
// Order rules (the header states them; a float64 host loop reproduces mean / median / range bit for bit):
//   mean    acc = v_0; acc = acc + v_p (p = 1 .. P - 1); acc / P            (a division, not a multiply by 1 / P)
//   median  ascending order statistics; odd P: the middle one; even P: (a + b) * 0.5 of the two middle ones (np.median)
//   range   max - min                  std  sqrt(sum_p (v_p - mean)^2 / P), summed in plane order
//   a NaN in any plane -> NaN in every output of the pixel (min / max / the network alone would drop it)
namespace rd {

constexpr int FUSE_MAX_P = 16;
constexpr int FUSE_MAX_CE = 63;         // Batcher's odd-even merge sort: 63 comparators at n = 16, fewer below

struct SortNet {
    int n;
    int a[FUSE_MAX_CE], b[FUSE_MAX_CE];
};

// Batcher's odd-even merge sort for ANY n (the partner test `/ (2 p)` keeps a comparator inside its merge block, which is
// what makes the n < 2^k networks the 2^k network with the comparators that touch a missing wire dropped)
constexpr SortNet make_sort_net(int n) {
    SortNet net{};
    for (int p = 1; p < n; p *= 2)
        for (int k = p; k >= 1; k /= 2)
            for (int j = k % p; j + k < n; j += 2 * k)
                for (int i = 0; i < k && i + j + k < n; ++i)
                    if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
                        net.a[net.n] = i + j;
                        net.b[net.n] = i + j + k;
                        ++net.n;
                    }
    return net;
}

__device__ __forceinline__ void fuse_cmpswap(double& lo, double& hi) {
    const double x = lo, y = hi;
    const bool sw = y < x;              // a NaN never swaps; the pixel's outputs are overwritten with NaN anyway
    lo = sw ? y : x;
    hi = sw ? x : y;
}

template <int P, size_t... I>
__device__ __forceinline__ void fuse_sort(double (&v)[P], std::index_sequence<I...>) {
    constexpr SortNet net = make_sort_net(P);
    (fuse_cmpswap(v[net.a[I]], v[net.b[I]]), ...);
}

// one pixel: v[] = its P values in plane order (sorted in place when the median is asked for)
template <int P>
__device__ __forceinline__ void fuse_pixel(double (&v)[P], int fuse_mode, int spread_mode, double& fused, double& spread) {
    const double nanv = __longlong_as_double(0x7ff8000000000000ll);
    bool nan = false;
    double acc = v[0];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        nan = nan || v[p] != v[p];
        if (p) acc = acc + v[p];
    }
    const double mean = acc / (double)P;
    spread = 0.0;
    if (spread_mode == RD_SPREAD_RANGE) {
        double lo = v[0], hi = v[0];
#pragma unroll
        for (int p = 1; p < P; ++p) {
            lo = v[p] < lo ? v[p] : lo;
            hi = v[p] > hi ? v[p] : hi;
        }
        spread = hi - lo;
    } else if (spread_mode == RD_SPREAD_STD) {
        double ss = 0.0;
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const double d = v[p] - mean;
            ss = ss + d * d;
        }
        spread = sqrt(ss / (double)P);
    }
    fused = mean;
    if (fuse_mode == RD_FUSE_MEDIAN) {
        constexpr int n_ce = make_sort_net(P).n;
        fuse_sort<P>(v, std::make_index_sequence<n_ce>{});
        fused = (P & 1) ? v[P / 2] : (v[(P - 1) / 2] + v[P / 2]) * 0.5;
    }
    if (nan) fused = spread = nanv;
}

template <int P, bool VEC>
__global__ __launch_bounds__(256) void fuse_planes_kernel(const double* __restrict__ planes, long plane_stride, long n,
                                                          int fuse_mode, int spread_mode, double* __restrict__ fused,
                                                          double* __restrict__ spread) {
    const long t0 = (long)blockIdx.x * 256 + threadIdx.x, step = (long)gridDim.x * 256;
    long tail = 0;                      // first pixel of the scalar part
    if (VEC) {
        // planes, plane_stride, fused and spread allow 16-byte accesses (the launcher checked): pixel pairs (2 q, 2 q + 1)
        const long pairs = n >> 1;
        for (long q = t0; q < pairs; q += step) {
            double a[P], b[P];
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const double2 d = ld_nt_f64x2(planes + (long)p * plane_stride + 2 * q);
                a[p] = d.x;
                b[p] = d.y;
            }
            double fa, sa, fb, sb;
            fuse_pixel<P>(a, fuse_mode, spread_mode, fa, sa);
            fuse_pixel<P>(b, fuse_mode, spread_mode, fb, sb);
            *reinterpret_cast<double2*>(fused + 2 * q) = make_double2(fa, fb);
            if (spread_mode != RD_SPREAD_NONE) *reinterpret_cast<double2*>(spread + 2 * q) = make_double2(sa, sb);
        }
        tail = pairs * 2;               // an odd n leaves one pixel
    }
    for (long i = tail + t0; i < n; i += step) {
        double a[P];
#pragma unroll
        for (int p = 0; p < P; ++p) a[p] = ld_nt_f64(planes + (long)p * plane_stride + i);
        double fa, sa;
        fuse_pixel<P>(a, fuse_mode, spread_mode, fa, sa);
        fused[i] = fa;
        if (spread_mode != RD_SPREAD_NONE) spread[i] = sa;
    }
}

template <int P>
static void fuse_launch(bool vec, int grid, hipStream_t s, const double* planes, long plane_stride, long n, int fuse_mode,
                        int spread_mode, double* fused, double* spread) {
    if (vec)
        RD_LAUNCH((fuse_planes_kernel<P, true>), dim3(grid), dim3(256), 0, s, planes, plane_stride, n, fuse_mode, spread_mode,
                  fused, spread);
    else
        RD_LAUNCH((fuse_planes_kernel<P, false>), dim3(grid), dim3(256), 0, s, planes, plane_stride, n, fuse_mode, spread_mode,
                  fused, spread);
}

}  // namespace rd

extern "C" {

int rd_fuse_planes(const double* planes, long long plane_stride, int n_planes, long long n, int fuse_mode, double* fused,
                   int spread_mode, double* spread, rd_stream_t s_) {
    RD_REQUIRE(planes && fused, "rd_fuse_planes: null pointer");
    RD_REQUIRE(n_planes >= 1 && n_planes <= FUSE_MAX_P, "rd_fuse_planes: n_planes must be in 1..%d (got %d)", FUSE_MAX_P,
               n_planes);
    RD_REQUIRE(n > 0 && plane_stride >= n, "rd_fuse_planes: bad shape (n=%lld plane_stride=%lld)", n, plane_stride);
    RD_REQUIRE(fuse_mode == RD_FUSE_MEAN || fuse_mode == RD_FUSE_MEDIAN, "rd_fuse_planes: unknown fuse_mode %d", fuse_mode);
    RD_REQUIRE(spread_mode == RD_SPREAD_NONE || spread_mode == RD_SPREAD_RANGE || spread_mode == RD_SPREAD_STD,
               "rd_fuse_planes: unknown spread_mode %d", spread_mode);
    RD_REQUIRE(spread_mode == RD_SPREAD_NONE || spread, "rd_fuse_planes: spread_mode %d needs the spread output", spread_mode);
    hipStream_t s = (hipStream_t)s_;
    const bool want_spread = spread_mode != RD_SPREAD_NONE;
    // 16-byte accesses need every plane's base, the outputs and so the plane stride on 16-byte boundaries
    const bool vec = (((uintptr_t)planes | (uintptr_t)fused | (want_spread ? (uintptr_t)spread : 0)) % 16) == 0 &&
                     (n_planes == 1 || plane_stride % 2 == 0);
    const long work = vec ? (long)((n + 1) / 2) : (long)n;
    const int grid = stats_grid(work);
    ProfScope ps(s, "fuse_planes", 0, 8.0 * n * (n_planes + 1 + (want_spread ? 1 : 0)));
    switch (n_planes) {
#define RD_FUSE_CASE(P_)                                                                                            \
    case P_:                                                                                                        \
        fuse_launch<P_>(vec, grid, s, planes, (long)plane_stride, (long)n, fuse_mode, spread_mode, fused, spread); \
        break;
        RD_FUSE_CASE(1) RD_FUSE_CASE(2) RD_FUSE_CASE(3) RD_FUSE_CASE(4) RD_FUSE_CASE(5) RD_FUSE_CASE(6) RD_FUSE_CASE(7)
        RD_FUSE_CASE(8) RD_FUSE_CASE(9) RD_FUSE_CASE(10) RD_FUSE_CASE(11) RD_FUSE_CASE(12) RD_FUSE_CASE(13)
        RD_FUSE_CASE(14) RD_FUSE_CASE(15) RD_FUSE_CASE(16)
#undef RD_FUSE_CASE
    }
    RD_LAUNCH_CHECK("fuse_planes");
    return RD_OK;
}

}  // extern "C"

// ---- the exact squared Euclidean distance transform with its feature transform, and the nearest-valid fill
// (include/resdepth_hip_edt.h).  Integer arithmetic only, no atomics.  The column pass: edt_band_kernel scans every band of
// RD_EDT_BAND_ROWS rows of every column downwards (one thread per band and column, threads along the columns, so a wave reads and
// writes consecutive addresses), leaves the nearest set row at or above each pixel INSIDE the band in d2's storage (-1: none) and
// the band's first and last set row in ws; edt_column_kernel finds the nearest set rows beyond its band by walking ws, scans the
// band upwards and replaces what d2 holds by the signed row offset to the nearest set pixel of the column, the upper one on a tie
// (RD_EDT_NONE: the column is empty).  The row pass: edt_row_kernel, one block per row, stages the row's offsets in LDS as int16
// BEFORE anything is written (d2 is updated in place), then every pixel searches outward from its own column.
namespace rd {

constexpr int EDT_THREADS = 256;
constexpr int EDT_NONE16 = -32768;                     // "no set pixel in this column" among int16 offsets: |offset| <= 32767
static_assert(RD_EDT_MAX_ROWS <= 32768, "a row offset fits an int16 beside EDT_NONE16");
static_assert((long)RD_EDT_MAX_ROWS * RD_EDT_MAX_ROWS + (long)RD_EDT_MAX_COLS * RD_EDT_MAX_COLS < 2147483647l, "d2 stays int32");
static_assert((long)RD_EDT_MAX_ROWS * RD_EDT_MAX_COLS < 2147483648l, "idx stays int32");
static_assert(RD_EDT_MAX_COLS * 2 <= 65536, "a row of offsets fits the LDS of one block");

__global__ __launch_bounds__(EDT_THREADS) void edt_band_kernel(const uint8_t* __restrict__ mask, int invert, int rows, int cols,
                                                               int bands, int32_t* __restrict__ d2, int32_t* __restrict__ ws) {
    const int c = blockIdx.x * EDT_THREADS + threadIdx.x, b = blockIdx.y;
    if (c >= cols) return;
    const int r0 = b * RD_EDT_BAND_ROWS, r1 = min(rows, r0 + RD_EDT_BAND_ROWS);
    int first = -1, last = -1;
    for (int r = r0; r < r1; ++r) {
        const size_t i = (size_t)r * cols + c;
        if ((mask[i] != 0) != (invert != 0)) {
            if (first < 0) first = r;
            last = r;
        }
        d2[i] = last;
    }
    ws[(size_t)b * cols + c] = first;
    ws[(size_t)(bands + b) * cols + c] = last;
}

__global__ __launch_bounds__(EDT_THREADS) void edt_column_kernel(int rows, int cols, int bands, int32_t* __restrict__ d2,
                                                                 const int32_t* __restrict__ ws) {
    const int c = blockIdx.x * EDT_THREADS + threadIdx.x, b = blockIdx.y;
    if (c >= cols) return;
    const int r0 = b * RD_EDT_BAND_ROWS, r1 = min(rows, r0 + RD_EDT_BAND_ROWS);
    int up = -1, next = -1;                            // the nearest set rows of the column above and below the band
    for (int bb = b - 1; bb >= 0 && up < 0; --bb) up = ws[(size_t)(bands + bb) * cols + c];
    for (int bb = b + 1; bb < bands && next < 0; ++bb) next = ws[(size_t)bb * cols + c];
    for (int r = r1 - 1; r >= r0; --r) {
        const size_t i = (size_t)r * cols + c;
        int u = d2[i];
        if (u < 0) u = up;
        if (u == r) next = r;
        int off = RD_EDT_NONE;
        if (u >= 0 && (next < 0 || r - u <= next - r))
            off = u - r;                               // the upper pixel wins a tie
        else if (next >= 0)
            off = next - r;
        d2[i] = off;
    }
}

__global__ __launch_bounds__(EDT_THREADS) void edt_row_kernel(int cols, int32_t* __restrict__ d2, int32_t* __restrict__ idx) {
    extern __shared__ short edt_offs[];                // cols int16 offsets
    const int r = blockIdx.x;
    const size_t base = (size_t)r * cols;
    int any = 0;
    for (int c = threadIdx.x; c < cols; c += EDT_THREADS) {
        const int v = d2[base + c];
        edt_offs[c] = (short)(v == RD_EDT_NONE ? EDT_NONE16 : v);
        any |= v != RD_EDT_NONE;
    }
    // the barrier between staging and writing, and the vote: a row without an offset means a mask without a set pixel
    if (!__syncthreads_or(any)) {
        for (int c = threadIdx.x; c < cols; c += EDT_THREADS) {
            d2[base + c] = RD_EDT_NONE;
            if (idx) idx[base + c] = -1;
        }
        return;
    }
    for (int c = threadIdx.x; c < cols; c += EDT_THREADS) {
        int best = RD_EDT_NONE, bc = c;
        int g = edt_offs[c];
        if (g != EDT_NONE16) best = g * g;
        const int reach = max(c, cols - 1 - c);        // beyond it both neighbours lie outside the row
        for (int dx = 1; dx <= reach && dx * dx < best; ++dx) {
            const int l = c - dx, rt = c + dx;
            if (l >= 0) {
                g = edt_offs[l];
                const int d = dx * dx + g * g;
                if (g != EDT_NONE16 && d < best) {
                    best = d;
                    bc = l;
                }
            }
            if (rt < cols) {
                g = edt_offs[rt];
                const int d = dx * dx + g * g;
                if (g != EDT_NONE16 && d < best) {
                    best = d;
                    bc = rt;
                }
            }
        }
        d2[base + c] = best;
        if (idx) idx[base + c] = best == RD_EDT_NONE ? -1 : (r + (int)edt_offs[bc]) * cols + bc;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void fill_nearest_kernel(const T* __restrict__ dsm, const int32_t* __restrict__ d2,
                                                           const int32_t* __restrict__ idx, long n, int max_d2,
                                                           T* __restrict__ out) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int d = d2[i], j = idx[i];
        const bool take = d > 0 && d <= max_d2 && j >= 0 && (long)j < n;
        out[i] = dsm[take ? (long)j : i];
    }
}

static bool edt_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

static bool edt_shape_ok(int rows, int cols) {
    return rows >= 1 && cols >= 1 && rows <= RD_EDT_MAX_ROWS && cols <= RD_EDT_MAX_COLS;
}

static int edt_bands(int rows) { return (rows + RD_EDT_BAND_ROWS - 1) / RD_EDT_BAND_ROWS; }

}  // namespace rd

extern "C" {

size_t rd_edt_ws_bytes(int rows, int cols) {
    if (!edt_shape_ok(rows, cols)) return 0;
    return (size_t)edt_bands(rows) * cols * 2 * sizeof(int32_t);
}

int rd_edt_sq(const uint8_t* mask, int invert, int rows, int cols, int32_t* d2, int32_t* idx, void* ws, size_t ws_bytes,
              rd_stream_t s_) {
    RD_REQUIRE(mask && d2 && ws, "rd_edt_sq: null pointer");
    RD_REQUIRE(edt_shape_ok(rows, cols), "rd_edt_sq: bad shape (rows=%d cols=%d; 1..%d x 1..%d)", rows, cols, RD_EDT_MAX_ROWS,
               RD_EDT_MAX_COLS);
    const size_t want = rd_edt_ws_bytes(rows, cols), n = (size_t)rows * cols;
    RD_REQUIRE(ws_bytes >= want, "rd_edt_sq: workspace of %zu bytes, %zu needed", ws_bytes, want);
    RD_REQUIRE(!edt_overlap(mask, n, d2, 4 * n) && !(idx && edt_overlap(mask, n, idx, 4 * n)),
               "rd_edt_sq: d2 or idx overlaps the mask");
    RD_REQUIRE(!(idx && edt_overlap(d2, 4 * n, idx, 4 * n)), "rd_edt_sq: d2 and idx overlap");
    hipStream_t s = (hipStream_t)s_;
    const int bands = edt_bands(rows);
    const dim3 grid((cols + EDT_THREADS - 1) / EDT_THREADS, bands);
    {
        // algorithmic bytes: the mask read, the in-band rows written and read, the offsets written
        ProfScope ps(s, "edt_columns", 0, 13.0 * (double)n);
        RD_LAUNCH(edt_band_kernel, grid, dim3(EDT_THREADS), 0, s, mask, invert ? 1 : 0, rows, cols, bands, d2, (int32_t*)ws);
        RD_LAUNCH_CHECK("edt_band");
        RD_LAUNCH(edt_column_kernel, grid, dim3(EDT_THREADS), 0, s, rows, cols, bands, d2, (const int32_t*)ws);
        RD_LAUNCH_CHECK("edt_column");
    }
    {
        // the offsets read, d2 and idx written
        ProfScope ps(s, "edt_rows", 0, (idx ? 12.0 : 8.0) * (double)n);
        RD_LAUNCH(edt_row_kernel, dim3((unsigned)rows), dim3(EDT_THREADS), (size_t)cols * sizeof(short), s, cols, d2, idx);
        RD_LAUNCH_CHECK("edt_row");
    }
    return RD_OK;
}

int rd_fill_nearest(const void* dsm, int dsm_f64, const int32_t* d2, const int32_t* idx, long long n, int max_d2, void* out,
                    rd_stream_t s_) {
    RD_REQUIRE(dsm && d2 && idx && out, "rd_fill_nearest: null pointer");
    RD_REQUIRE(n >= 1, "rd_fill_nearest: n = %lld", n);
    RD_REQUIRE(max_d2 >= 0, "rd_fill_nearest: max_d2 %d is negative", max_d2);
    const size_t width = dsm_f64 ? 8 : 4;
    RD_REQUIRE(!edt_overlap(dsm, width * (size_t)n, out, width * (size_t)n), "rd_fill_nearest: out overlaps dsm");
    hipStream_t s = (hipStream_t)s_;
    ProfScope ps(s, "fill_nearest", 0, (double)n * (8.0 + 2.0 * width));
    if (dsm_f64)
        RD_LAUNCH(fill_nearest_kernel<uint64_t>, dim3(stats_grid((long)n)), dim3(256), 0, s, (const uint64_t*)dsm, d2, idx, (long)n,
                  max_d2, (uint64_t*)out);
    else
        RD_LAUNCH(fill_nearest_kernel<uint32_t>, dim3(stats_grid((long)n)), dim3(256), 0, s, (const uint32_t*)dsm, d2, idx, (long)n,
                  max_d2, (uint32_t*)out);
    RD_LAUNCH_CHECK("fill_nearest");
    return RD_OK;
}

}  // extern "C"

// ---- where the error is and on what ground (include/resdepth_hip_errmap.h) -------------------------------------------------
// cell_stats_kernel: the statistics engine turned inside out -- not few sets of many values with global histograms and a launch
// per pass, but one block per cell with everything in the block.  The moments are SetMoments with one set (a thread adds its
// pixels in row-major order, the block adds its threads in SetMoments::reduce's tree); the medians are the engine's radix
// select on the same keys with the same two ranks per selector, the pass histograms in LDS, the pick a block-wide scan like
// sets_pick_kernel's.  Phase 0 selects the median and the absolute median out of the same eight reads of the cell, phase 1 the
// NMAD around the absolute median.  Each pass reads the cell's pixels again, consecutive lanes along x; LDS holds the
// histograms only, so a 4 x 4 and a 256 x 256 cell take the same path.
// dsm_slope_kernel: Horn's slope from a tile staged in LDS with its halo, like dilate_kernel; every operation through the
// round-to-nearest intrinsics so that nothing is contracted.
// bin_classes_kernel: the bin of a covariate value by counting the edges at or below it (the edges travel by value).
namespace rd {

constexpr int SLOPE_TW = 64, SLOPE_TH = 16;
static_assert(RD_SLOPE_MAX_ROWS == 65535 * SLOPE_TH, "grid.y of dsm_slope_kernel");

struct BinEdges {
    int n_bins;
    double e[RD_BIN_MAX + 1];
};

// a thread's walk over the w x h pixels of a cell: pixel t, t + 256, ... in row-major order, without a division per pixel
struct CellWalk {
    int x, y, dx, dy, w;
    __device__ __forceinline__ CellWalk(int w_) : x(threadIdx.x % w_), y(threadIdx.x / w_), dx(256 % w_), dy(256 / w_), w(w_) {}
    __device__ __forceinline__ void next() {
        x += dx;
        y += dy;
        if (x >= w) {
            x -= w;
            ++y;
        }
    }
};

__global__ __launch_bounds__(256) void cell_stats_kernel(const double* __restrict__ src, const uint8_t* __restrict__ cls,
                                                         int rows, int cols, int cell_h, int cell_w, int ncx, unsigned need,
                                                         double thr, double* __restrict__ out) {
    __shared__ double red[4][5];
    __shared__ double mom[5];
    __shared__ unsigned lh[2][2][256];                 // [selector][side][bin]
    __shared__ unsigned wtot[4][4];                    // [histogram][wave]: the waves' totals of the pick's scan
    __shared__ unsigned long long pf[2][2];            // [selector][rank]: the key prefix found so far
    __shared__ unsigned rk[2][2];                      // the rank among the values under that prefix
    __shared__ int bin_of[2][2];
    __shared__ unsigned below_of[2][2];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int cy = blockIdx.x / ncx, cx = blockIdx.x - cy * ncx;
    const int y0 = cy * cell_h, x0 = cx * cell_w;
    const int h = min(cell_h, rows - y0), w = min(cell_w, cols - x0);
    const double* __restrict__ sp0 = src + (long)y0 * cols + x0;
    const uint8_t* __restrict__ cp0 = cls + (long)y0 * cols + x0;
    double* __restrict__ o = out + (long)blockIdx.x * 8;
    const double nanv = __longlong_as_double(0x7ff8000000000000ll);

    SetSpecs sp;
    sp.n = 1;
    for (int i = 0; i < RD_STATS_MAX_SETS; ++i) {
        sp.src[i] = 0;
        sp.need[i] = need;
        sp.thr[i] = thr;
    }
    {
        SetMoments m;
        for (CellWalk p(w); p.y < h; p.next()) {
            const long i = (long)p.y * cols + p.x;
            const double d = sp0[i];
            m.add(sp, cp0[i], [&](int) { return d; });
        }
        m.reduce(0, red, mom);
    }
    const double cnt = mom[0];
    if (t == 0) {
        o[0] = cnt;
        o[1] = cnt > 0 ? mom[4] : nanv;
        o[2] = cnt > 0 ? mom[3] : nanv;
        o[3] = cnt > 0 ? mom[1] / cnt : nanv;
        o[4] = cnt > 0 ? sqrt(mom[2] / cnt) : nanv;
    }
    if (!(cnt > 0)) {                                  // block-uniform
        if (t == 0) o[5] = o[6] = o[7] = nanv;
        return;
    }
    const unsigned c = (unsigned)cnt;
    double shift = 0.0;
    for (int phase = 0; phase < 2; ++phase) {
        // selector j of phase 0: 0 the absolute median (value mode 1), 1 the median (mode 0); of phase 1: the NMAD (mode 2)
        const int nsel = phase == 0 ? 2 : 1;
        if (t < 4) {
            pf[t >> 1][t & 1] = 0ull;
            rk[t >> 1][t & 1] = (t & 1) ? c / 2 : (c - 1) / 2;
        }
        for (int pass = 7; pass >= 0; --pass) {
            for (int i = t; i < 2 * 2 * 256; i += 256) (&lh[0][0][0])[i] = 0u;
            __syncthreads();
            const unsigned long long p00 = pf[0][0], p01 = pf[0][1], p10 = pf[1][0], p11 = pf[1][1];
            const int hs = 8 * (pass + 1);
            for (CellWalk p(w); p.y < h; p.next()) {
                const long i = (long)p.y * cols + p.x;
                const double r = sp0[i];
                if (!in_set(sp, 0, cp0[i], r)) continue;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if (j >= nsel) continue;
                    const unsigned long long k = key_of(pick_value(r, phase == 0 ? 1 - j : 2, shift));
                    const unsigned long long hi = pass == 7 ? 0ull : (k >> hs);
                    const unsigned b = (unsigned)((k >> (8 * pass)) & 255ull);
                    if (hi == (j ? p10 : p00))
                        atomicAdd(&lh[j][0][b], 1u);
                    else if (hi == (j ? p11 : p01))
                        atomicAdd(&lh[j][1][b], 1u);
                }
            }
            __syncthreads();
            // the pick: thread t holds bin t of the four histograms (selector j, rank q); while a selector's two prefixes agree
            // both of its ranks read side 0.  An inclusive scan per histogram: shuffles inside a wave, the waves' totals in LDS
            unsigned cb[4], incl[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = q >> 1, side = q & 1;
                const bool same = (j ? p10 == p11 : p00 == p01);
                cb[q] = j < nsel ? lh[j][side && !same ? 1 : 0][t] : 0u;
                unsigned v = cb[q];
                for (int off = 1; off < 64; off <<= 1) {
                    const unsigned u = __shfl_up(v, off);
                    if (lane >= off) v += u;
                }
                incl[q] = v;
                if (lane == 63) wtot[q][wv] = v;
            }
            if (t < 4) {
                bin_of[t >> 1][t & 1] = 255;
                below_of[t >> 1][t & 1] = 0u;
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = q >> 1, side = q & 1;
                unsigned base = 0u;
                for (int u = 0; u < 4; ++u)
                    if (u < wv) base += wtot[q][u];
                const unsigned in = incl[q] + base, ex = in - cb[q];
                const unsigned rank = rk[j][side];
                if (cb[q] && ex <= rank && rank < in) {
                    bin_of[j][side] = t;
                    below_of[j][side] = ex;
                }
            }
            __syncthreads();
            if (t < 4) {
                const int j = t >> 1, side = t & 1;
                pf[j][side] = (pf[j][side] << 8) | (unsigned long long)bin_of[j][side];
                rk[j][side] -= below_of[j][side];
            }
            __syncthreads();
        }
        if (phase == 0) {
            const double am = 0.5 * (unkey(pf[0][0]) + unkey(pf[0][1]));
            if (t == 0) {
                o[5] = am;
                o[6] = 0.5 * (unkey(pf[1][0]) + unkey(pf[1][1]));
            }
            shift = am;
            __syncthreads();                            // every thread has read the prefixes before they are cleared
        } else if (t == 0) {
            o[7] = 1.4826 * (0.5 * (unkey(pf[0][0]) + unkey(pf[0][1])));
        }
    }
}

__global__ __launch_bounds__(256) void dsm_slope_kernel(const void* __restrict__ dsm, int f64, int rows, int cols,
                                                        double nodata, double run_x, double run_y,
                                                        double* __restrict__ slope) {
    constexpr int PW = SLOPE_TW + 2, PH = SLOPE_TH + 2;
    __shared__ double tile[PH * PW];                   // NaN: nodata, NaN or outside the raster
    const double nanv = __longlong_as_double(0x7ff8000000000000ll);
    const int ox = blockIdx.x * SLOPE_TW, oy = blockIdx.y * SLOPE_TH;
    for (int i = threadIdx.x; i < PH * PW; i += blockDim.x) {
        const int ty = i / PW, tx = i - ty * PW;
        const int y = oy - 1 + ty, x = ox - 1 + tx;
        double v = nanv;
        if (y >= 0 && y < rows && x >= 0 && x < cols) {
            v = load_f(dsm, f64, (long)y * cols + x);
            if (v == nodata) v = nanv;
        }
        tile[i] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SLOPE_TH * SLOPE_TW; i += blockDim.x) {
        const int ty = i / SLOPE_TW, tx = i - ty * SLOPE_TW;
        const int y = oy + ty, x = ox + tx;
        if (y >= rows || x >= cols) continue;
        const double* r0 = tile + ty * PW + tx;        // the row above, starting at the left neighbour
        const double a = r0[0], b = r0[1], c = r0[2];
        const double d = r0[PW], e = r0[PW + 1], f = r0[PW + 2];
        const double g = r0[2 * PW], hh = r0[2 * PW + 1], ii = r0[2 * PW + 2];
        const bool bad = isnan(a) || isnan(b) || isnan(c) || isnan(d) || isnan(e) || isnan(f) || isnan(g) || isnan(hh) ||
                         isnan(ii);
        const double east = __dadd_rn(__dadd_rn(c, __dmul_rn(2.0, f)), ii);
        const double west = __dadd_rn(__dadd_rn(a, __dmul_rn(2.0, d)), g);
        const double south = __dadd_rn(__dadd_rn(g, __dmul_rn(2.0, hh)), ii);
        const double north = __dadd_rn(__dadd_rn(a, __dmul_rn(2.0, b)), c);
        const double p = __ddiv_rn(__dsub_rn(east, west), run_x);
        const double q = __ddiv_rn(__dsub_rn(south, north), run_y);
        const double v = __dsqrt_rn(__dadd_rn(__dmul_rn(p, p), __dmul_rn(q, q)));
        slope[(long)y * cols + x] = bad ? nanv : v;
    }
}

__global__ __launch_bounds__(256) void bin_classes_kernel(const void* __restrict__ by, int f64, const uint8_t* __restrict__ cls,
                                                          long n, BinEdges ed, int groups, uint8_t* __restrict__ out) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const double v = load_f(by, f64, i);
        int at_or_below = 0;                           // edges <= v: 0 for a NaN
#pragma unroll
        for (int k = 0; k <= RD_BIN_MAX; ++k) at_or_below += (k <= ed.n_bins && v >= ed.e[k]) ? 1 : 0;
        const int b = at_or_below - 1;                 // -1: below the first edge; n_bins: at or above the last one
        const unsigned valid = cls[i] & 3u;
        const bool binned = b >= 0 && b < ed.n_bins;
        for (int g = 0; g < groups; ++g) {
            const int q = b - 6 * g;
            out[(long)g * n + i] = (uint8_t)(valid | ((binned && q >= 0 && q < 6) ? (4u << q) : 0u));
        }
    }
}

}  // namespace rd

extern "C" {

int rd_cell_stats(const double* src, const uint8_t* cls, int rows, int cols, int cell_h, int cell_w, int need, double thr,
                  double* out, rd_stream_t s_) {
    RD_REQUIRE(src && cls && out, "rd_cell_stats: null pointer");
    RD_REQUIRE(rows >= 1 && cols >= 1, "rd_cell_stats: bad shape (rows=%d cols=%d)", rows, cols);
    RD_REQUIRE(cell_h >= RD_CELL_MIN && cell_h <= RD_CELL_MAX && cell_w >= RD_CELL_MIN && cell_w <= RD_CELL_MAX,
               "rd_cell_stats: cell %d x %d, sides must be in %d..%d", cell_h, cell_w, RD_CELL_MIN, RD_CELL_MAX);
    RD_REQUIRE(need >= 0 && need <= 255, "rd_cell_stats: need %d outside 0..255", need);
    RD_REQUIRE(thr >= 0.0 && thr <= 1.7976931348623157e308, "rd_cell_stats: threshold %g must be finite and >= 0", thr);
    const long ncy = (rows + cell_h - 1) / cell_h, ncx = (cols + cell_w - 1) / cell_w;
    // one block of 256 threads per cell, and a launch holds fewer than 2^32 threads
    RD_REQUIRE(ncy * ncx < (long)RD_CELL_MAX_CELLS, "rd_cell_stats: %ld x %ld cells, a call takes fewer than %d", ncy, ncx,
               RD_CELL_MAX_CELLS);
    hipStream_t s = (hipStream_t)s_;
    // algorithmic bytes: 17 reads of every pixel's value and class byte, one row of eight doubles per cell
    ProfScope ps(s, "cell_stats", 0, 17.0 * 9.0 * rows * cols + 64.0 * ncy * ncx);
    RD_LAUNCH(cell_stats_kernel, dim3((unsigned)(ncy * ncx)), dim3(256), 0, s, src, cls, rows, cols, cell_h, cell_w, (int)ncx,
              (unsigned)need, thr, out);
    RD_LAUNCH_CHECK("cell_stats");
    return RD_OK;
}

int rd_dsm_slope(const void* dsm, int dsm_f64, int rows, int cols, double nodata, double gsd_x, double gsd_y, double* slope,
                 rd_stream_t s_) {
    RD_REQUIRE(dsm && slope && (const void*)slope != dsm, "rd_dsm_slope: null or aliased pointer");
    RD_REQUIRE(rows >= 1 && cols >= 1, "rd_dsm_slope: bad shape (rows=%d cols=%d)", rows, cols);
    RD_REQUIRE(gsd_x > 0.0 && gsd_x <= 1.7976931348623157e308 && gsd_y > 0.0 && gsd_y <= 1.7976931348623157e308,
               "rd_dsm_slope: GSD %g x %g must be positive and finite", gsd_x, gsd_y);
    RD_REQUIRE(rows <= RD_SLOPE_MAX_ROWS, "rd_dsm_slope: %d rows (at most %d: 65535 tiles of %d rows)", rows, RD_SLOPE_MAX_ROWS,
               SLOPE_TH);
    hipStream_t s = (hipStream_t)s_;
    ProfScope ps(s, "dsm_slope", 0, (double)rows * cols * ((dsm_f64 ? 8.0 : 4.0) + 8.0));
    const dim3 grid((cols + SLOPE_TW - 1) / SLOPE_TW, (rows + SLOPE_TH - 1) / SLOPE_TH);
    RD_LAUNCH(dsm_slope_kernel, grid, dim3(256), 0, s, dsm, dsm_f64 ? 1 : 0, rows, cols, nodata, 8.0 * gsd_x, 8.0 * gsd_y, slope);
    RD_LAUNCH_CHECK("dsm_slope");
    return RD_OK;
}

int rd_bin_classes(const void* by, int by_f64, const uint8_t* cls, long long n, const double* edges, int n_bins, uint8_t* out,
                   rd_stream_t s_) {
    RD_REQUIRE(by && cls && edges && out, "rd_bin_classes: null pointer");
    RD_REQUIRE(n >= 1, "rd_bin_classes: n = %lld", n);
    RD_REQUIRE(n_bins >= 1 && n_bins <= RD_BIN_MAX, "rd_bin_classes: %d bins (1..%d)", n_bins, RD_BIN_MAX);
    BinEdges ed;
    ed.n_bins = n_bins;
    for (int k = 0; k <= RD_BIN_MAX; ++k) ed.e[k] = k <= n_bins ? edges[k] : 0.0;
    for (int k = 0; k <= n_bins; ++k) RD_REQUIRE(ed.e[k] == ed.e[k], "rd_bin_classes: edge %d is NaN", k);
    for (int k = 0; k < n_bins; ++k)
        RD_REQUIRE(ed.e[k] < ed.e[k + 1], "rd_bin_classes: edges %d and %d do not increase (%g, %g)", k, k + 1, ed.e[k],
                   ed.e[k + 1]);
    const int groups = (n_bins + 5) / 6;
    hipStream_t s = (hipStream_t)s_;
    ProfScope ps(s, "bin_classes", 0, (double)n * ((by_f64 ? 8.0 : 4.0) + 1.0 + groups));
    RD_LAUNCH(bin_classes_kernel, dim3(stats_grid((long)n)), dim3(256), 0, s, by, by_f64 ? 1 : 0, cls, (long)n, ed, groups, out);
    RD_LAUNCH_CHECK("bin_classes");
    return RD_OK;
}

}  // extern "C"
