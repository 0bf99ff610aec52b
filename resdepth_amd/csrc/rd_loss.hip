// Masked, de-normalised training losses beyond L1 (include/resdepth_hip_loss.h): a quadratic / Huber / L1 data term plus an optional
// term on the first differences of the residual, and the masked MAE next to the loss.  Generalises the l1_* kernels of
// rd_elementwise.hip (Trainer._compute_denormalized_loss, lib/Trainer.py:87-100, with any criterion); DESIGN.md section 3.9.
//
// A block walks tiles of TR x TC pixels, each inside one sample.  The residual r (fp32, the roundings of `denorm` below) and the
// mask of the tile and of a one-pixel ring around it are staged in LDS once; every neighbour is read from there.  Cells outside
// the sample are staged with m = 0, so the stencil needs no bounds test of its own and a pair can neither cross a sample
// boundary nor wrap a row.  Sums are fp64, added in a fixed order (thread -> block tree -> one block over the per-block sums).
#include "rd_common.h"

using namespace rd;

namespace {

constexpr int TR = RD_LOSS_STRIP_ROWS, TC = RD_LOSS_STRIP_COLS;
constexpr int LROWS = TR + 2, PITCH = TC + 2;       // staged cell (lr, lc) is pixel (r0 + lr - 1, c0 + lc - 1)
constexpr int NSUM = 5;                             // A, C, D, S, Q
static_assert(2 * PITCH + 2 * TR <= 256, "the halo ring is staged by one pass of the block");
static_assert(TC % 4 == 0 && (TR * TC) % 1024 == 0, "tile interior in whole float4 passes");

__device__ __forceinline__ float denorm(float v, float sd, float mu) { return __fadd_rn(__fmul_rn(v, sd), mu); }

struct Geo {
    int tiles_x, tiles_ps, tiles;     // tiles per row of tiles, per sample, in all
};

__device__ __forceinline__ void tile_of(int t, const Geo& g, int& n, int& r0, int& c0) {
    n = t / g.tiles_ps;
    const int q = t - n * g.tiles_ps, ty = q / g.tiles_x;
    r0 = ty * TR;
    c0 = (q - ty * g.tiles_x) * TC;
}

__device__ __forceinline__ void stage_cell(float* sr, uint8_t* sm, int lr, int lc, int gr, int gc, int h, int w,
                                           const float* __restrict__ yp, const float* __restrict__ y,
                                           const uint8_t* __restrict__ mask, long base, float sd, float mu) {
    float r = 0.f;
    uint8_t m = 0;
    if (gr >= 0 && gr < h && gc >= 0 && gc < w) {
        const long e = base + (long)gr * w + gc;
        m = mask[e] != 0;
        r = denorm(yp[e], sd, mu) - denorm(y[e], sd, mu);
    }
    sr[lr * PITCH + lc] = r;
    sm[lr * PITCH + lc] = m;
}

// ring == false: the forward counts each pair once from its upper / left pixel, so the row above and the column left of the
// tile are not needed (staged as invalid without touching memory)
template <bool VEC>
__device__ __forceinline__ void stage_tile(float* sr, uint8_t* sm, bool ring, int r0, int c0, int h, int w,
                                           const float* __restrict__ yp, const float* __restrict__ y,
                                           const uint8_t* __restrict__ mask, long base, float sd, float mu) {
    if (VEC) {
        for (int i = threadIdx.x; i < TR * (TC / 4); i += 256) {
            const int row = i / (TC / 4), q = i - row * (TC / 4);
            const int gr = r0 + row, gc = c0 + 4 * q;
            float r[4] = {0.f, 0.f, 0.f, 0.f};
            uint8_t m[4] = {0, 0, 0, 0};
            if (gr < h && gc < w) {          // w % 4 == 0: the four pixels are inside together
                const long e = base + (long)gr * w + gc;
                const float4 a = *reinterpret_cast<const float4*>(yp + e), b = *reinterpret_cast<const float4*>(y + e);
                const uchar4 mm = *reinterpret_cast<const uchar4*>(mask + e);
                r[0] = denorm(a.x, sd, mu) - denorm(b.x, sd, mu);
                r[1] = denorm(a.y, sd, mu) - denorm(b.y, sd, mu);
                r[2] = denorm(a.z, sd, mu) - denorm(b.z, sd, mu);
                r[3] = denorm(a.w, sd, mu) - denorm(b.w, sd, mu);
                m[0] = mm.x != 0, m[1] = mm.y != 0, m[2] = mm.z != 0, m[3] = mm.w != 0;
            }
            const int o = (row + 1) * PITCH + 1 + 4 * q;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sr[o + j] = r[j];
                sm[o + j] = m[j];
            }
        }
        const int t = threadIdx.x;
        if (t < 2 * PITCH + 2 * TR) {
            int lr, lc;
            if (t < PITCH) {
                lr = 0, lc = t;
            } else if (t < 2 * PITCH) {
                lr = TR + 1, lc = t - PITCH;
            } else if (t < 2 * PITCH + TR) {
                lr = t - 2 * PITCH + 1, lc = 0;
            } else {
                lr = t - 2 * PITCH - TR + 1, lc = TC + 1;
            }
            const bool skip = !ring && (lr == 0 || lc == 0);
            stage_cell(sr, sm, lr, lc, skip ? -1 : r0 + lr - 1, c0 + lc - 1, h, w, yp, y, mask, base, sd, mu);
        }
    } else {
        for (int i = threadIdx.x; i < LROWS * PITCH; i += 256) {
            const int lr = i / PITCH, lc = i - lr * PITCH;
            const bool skip = !ring && (lr == 0 || lc == 0);
            stage_cell(sr, sm, lr, lc, skip ? -1 : r0 + lr - 1, c0 + lc - 1, h, w, yp, y, mask, base, sd, mu);
        }
    }
}

// rho without its scale, of |r|
__device__ __forceinline__ double rho(double ar, int kind, double delta) {
    if (kind == RD_LOSS_L1) return ar;
    if (kind == RD_LOSS_L2) return ar * ar;
    return ar <= delta ? 0.5 * ar * ar : delta * (ar - 0.5 * delta);
}

// rho' without its scale; sign(0) = 0
__device__ __forceinline__ double rho_prime(float r, int kind, double delta) {
    const double d = (double)r, sg = (double)((r > 0.f) - (r < 0.f));
    if (kind == RD_LOSS_L1) return sg;
    if (kind == RD_LOSS_L2) return 2.0 * d;
    return fabs(d) <= delta ? d : delta * sg;
}

template <bool VEC>
__global__ __launch_bounds__(256) void masked_loss_partial_kernel(const float* __restrict__ yp, const float* __restrict__ y,
                                                                  const uint8_t* __restrict__ mask,
                                                                  const float* __restrict__ mean,
                                                                  const float* __restrict__ stdv, double* __restrict__ partial,
                                                                  int h, int w, Geo g, int kind, double delta) {
    __shared__ float sr[LROWS * PITCH];
    __shared__ uint8_t sm[LROWS * PITCH];
    __shared__ double red[NSUM * 256];
    double A = 0.0, D = 0.0, S = 0.0;
    int C = 0, Q = 0;
    for (int t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        int n, r0, c0;
        tile_of(t, g, n, r0, c0);
        __syncthreads();                 // the previous tile has been read
        stage_tile<VEC>(sr, sm, false, r0, c0, h, w, yp, y, mask, (long)n * h * w, stdv[n], mean[n]);
        __syncthreads();
        for (int i = threadIdx.x; i < TR * TC; i += 256) {
            const int o = (i / TC + 1) * PITCH + (i % TC) + 1;
            if (!sm[o]) continue;
            const float r = sr[o];
            const double ar = fabs((double)r);
            A += ar;
            D += rho(ar, kind, delta);
            C += 1;
            if (sm[o + 1]) {
                S += (double)fabsf(r - sr[o + 1]);
                Q += 1;
            }
            if (sm[o + PITCH]) {
                S += (double)fabsf(r - sr[o + PITCH]);
                Q += 1;
            }
        }
    }
    const int t = threadIdx.x;
    red[t] = A, red[256 + t] = (double)C, red[512 + t] = D, red[768 + t] = S, red[1024 + t] = (double)Q;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) {
#pragma unroll
            for (int k = 0; k < NSUM; ++k) red[k * 256 + t] += red[k * 256 + t + off];
        }
        __syncthreads();
    }
    if (t < NSUM) partial[(long)blockIdx.x * NSUM + t] = red[t * 256];
}

__global__ __launch_bounds__(256) void masked_loss_reduce_kernel(const double* __restrict__ partial, double* __restrict__ sums,
                                                                 int nb, double scale) {
    __shared__ double red[NSUM * 256];
    const int t = threadIdx.x;
    double v[NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = t; b < nb; b += 256) {
#pragma unroll
        for (int k = 0; k < NSUM; ++k) v[k] += partial[(long)b * NSUM + k];
    }
#pragma unroll
    for (int k = 0; k < NSUM; ++k) red[k * 256 + t] = v[k];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) {
#pragma unroll
            for (int k = 0; k < NSUM; ++k) red[k * 256 + t] += red[k * 256 + t + off];
        }
        __syncthreads();
    }
    if (t < 8) sums[t] = t < NSUM ? (t == 2 ? red[t * 256] * scale : red[t * 256]) : 0.0;
}

template <bool VEC, bool SLOPE>
__global__ __launch_bounds__(256) void masked_loss_finish_kernel(const float* __restrict__ yp, const float* __restrict__ y,
                                                                 const uint8_t* __restrict__ mask,
                                                                 const float* __restrict__ mean,
                                                                 const float* __restrict__ stdv, const double* __restrict__ sums,
                                                                 int kind, double delta, double scale, double lambda,
                                                                 const float* __restrict__ gout_dev, float* __restrict__ loss,
                                                                 float* __restrict__ mae, float* __restrict__ dyp, int h, int w,
                                                                 Geo g) {
    __shared__ float sr[SLOPE ? LROWS * PITCH : 1];
    __shared__ uint8_t sm[SLOPE ? LROWS * PITCH : 1];
    const double A = sums[0], C = sums[1], D = sums[2], S = sums[3], Q = sums[4];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (loss) loss[0] = (float)(D / C + ((lambda > 0.0 && Q > 0.0) ? lambda * S / Q : 0.0));
        if (mae) mae[0] = (float)(A / C);
    }
    if (!dyp) return;
    const double gout = gout_dev ? (double)gout_dev[0] : 1.0;
    const double cd = scale / C;
    const double cs = (SLOPE && Q > 0.0) ? lambda / Q : 0.0;
    for (int t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        int n, r0, c0;
        tile_of(t, g, n, r0, c0);
        const long base = (long)n * h * w;
        const float sd = stdv[n], mu = mean[n];
        const double gs = gout * (double)sd;
        if (SLOPE) {
            __syncthreads();
            stage_tile<VEC>(sr, sm, true, r0, c0, h, w, yp, y, mask, base, sd, mu);
            __syncthreads();
        }
        // gradient of the staged cell o (SLOPE) -- data part plus the integer stencil, one multiplication each, one rounding
        auto staged = [&](int o) -> float {
            if (!sm[o]) return 0.f;
            const float r = sr[o];
            int k = 0;
            if (sm[o - 1]) k += (r > sr[o - 1]) - (r < sr[o - 1]);
            if (sm[o + 1]) k += (r > sr[o + 1]) - (r < sr[o + 1]);
            if (sm[o - PITCH]) k += (r > sr[o - PITCH]) - (r < sr[o - PITCH]);
            if (sm[o + PITCH]) k += (r > sr[o + PITCH]) - (r < sr[o + PITCH]);
            return (float)(gs * (cd * rho_prime(r, kind, delta) + cs * (double)k));
        };
        auto direct = [&](float a, float b, uint8_t m) -> float {
            if (!m) return 0.f;
            return (float)(gs * (cd * rho_prime(denorm(a, sd, mu) - denorm(b, sd, mu), kind, delta)));
        };
        if (VEC) {
            for (int i = threadIdx.x; i < TR * (TC / 4); i += 256) {
                const int row = i / (TC / 4), q = i - row * (TC / 4);
                const int gr = r0 + row, gc = c0 + 4 * q;
                if (gr >= h || gc >= w) continue;
                const long e = base + (long)gr * w + gc;
                float4 o4;
                if (SLOPE) {
                    const int o = (row + 1) * PITCH + 1 + 4 * q;
                    o4 = make_float4(staged(o), staged(o + 1), staged(o + 2), staged(o + 3));
                } else {
                    const float4 a = *reinterpret_cast<const float4*>(yp + e), b = *reinterpret_cast<const float4*>(y + e);
                    const uchar4 mm = *reinterpret_cast<const uchar4*>(mask + e);
                    o4 = make_float4(direct(a.x, b.x, mm.x), direct(a.y, b.y, mm.y), direct(a.z, b.z, mm.z),
                                     direct(a.w, b.w, mm.w));
                }
                *reinterpret_cast<float4*>(dyp + e) = o4;
            }
        } else {
            for (int i = threadIdx.x; i < TR * TC; i += 256) {
                const int row = i / TC, col = i % TC;
                const int gr = r0 + row, gc = c0 + col;
                if (gr >= h || gc >= w) continue;
                const long e = base + (long)gr * w + gc;
                dyp[e] = SLOPE ? staged((row + 1) * PITCH + col + 1) : direct(yp[e], y[e], mask[e]);
            }
        }
    }
}

// tiles of an [n][h][w] batch; false when a size is outside what the kernels index (32-bit pixel counts)
bool make_geo(int n, int h, int w, Geo* g) {
    if (n <= 0 || h <= 0 || w <= 0) return false;
    const long long hw = (long long)h * w;
    if (hw >= (1LL << 31) || hw * n >= (1LL << 31)) return false;
    g->tiles_x = cdiv(w, TC);
    g->tiles_ps = g->tiles_x * cdiv(h, TR);
    g->tiles = g->tiles_ps * n;
    return true;
}

int loss_grid(const Geo& g) { return g.tiles < RD_LOSS_MAX_BLOCKS ? g.tiles : RD_LOSS_MAX_BLOCKS; }

bool kind_ok(int kind, double delta, double scale) {
    if (kind != RD_LOSS_L1 && kind != RD_LOSS_L2 && kind != RD_LOSS_HUBER) return false;
    if (kind == RD_LOSS_HUBER && !(delta > 0.0)) return false;
    return scale > 0.0;
}

bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" {

size_t rd_masked_loss_ws_bytes(int n, int h, int w) {
    Geo g;
    if (!make_geo(n, h, w, &g)) return 0;
    return (size_t)loss_grid(g) * NSUM * sizeof(double);
}

int rd_masked_loss_partial(const float* yp, const float* y, const uint8_t* mask, const float* mean, const float* stdv,
                           double* sums, int n, int h, int w, int kind, double delta, double scale, void* ws, size_t ws_bytes,
                           rd_stream_t s) {
    Geo g;
    RD_REQUIRE(yp && y && mask && mean && stdv && sums && make_geo(n, h, w, &g), "rd_masked_loss_partial: bad arguments");
    RD_REQUIRE(kind_ok(kind, delta, scale), "rd_masked_loss_partial: unknown kind, delta <= 0 or scale <= 0");
    const int nb = loss_grid(g);
    if (!ws || ws_bytes < (size_t)nb * NSUM * sizeof(double)) {
        set_error("rd_masked_loss_partial: workspace too small");
        return RD_ERR_WS;
    }
    const bool vec = w % 4 == 0 && aligned(yp, 16) && aligned(y, 16) && aligned(mask, 4);
    ProfScope ps((hipStream_t)s, "masked_loss", 0, 9.0 * (double)n * h * w);
    if (vec)
        RD_LAUNCH(masked_loss_partial_kernel<true>, dim3(nb), dim3(256), 0, (hipStream_t)s, yp, y, mask, mean, stdv,
                  (double*)ws, h, w, g, kind, delta);
    else
        RD_LAUNCH(masked_loss_partial_kernel<false>, dim3(nb), dim3(256), 0, (hipStream_t)s, yp, y, mask, mean, stdv,
                  (double*)ws, h, w, g, kind, delta);
    RD_LAUNCH(masked_loss_reduce_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, (const double*)ws, sums, nb, scale);
    RD_LAUNCH_CHECK("masked_loss_partial");
    return RD_OK;
}

int rd_masked_loss_finish(const float* yp, const float* y, const uint8_t* mask, const float* mean, const float* stdv,
                          const double* sums, double numel_total, int kind, double delta, double scale, double lambda,
                          const float* gout, float* loss, float* mae, float* dyp, int n, int h, int w, rd_stream_t s) {
    Geo g;
    RD_REQUIRE(yp && y && mask && mean && stdv && sums && make_geo(n, h, w, &g), "rd_masked_loss_finish: bad arguments");
    RD_REQUIRE(kind_ok(kind, delta, scale), "rd_masked_loss_finish: unknown kind, delta <= 0 or scale <= 0");
    RD_REQUIRE(numel_total > 0.0 && lambda >= 0.0 && lambda <= 1.7e308, "rd_masked_loss_finish: numel_total <= 0 or bad lambda");
    const bool vec = w % 4 == 0 && aligned(yp, 16) && aligned(y, 16) && aligned(mask, 4) && aligned(dyp, 16);
    const bool slope = lambda > 0.0;
    const dim3 grid(dyp ? loss_grid(g) : 1);
    ProfScope ps((hipStream_t)s, "masked_loss", 0, 13.0 * (double)n * h * w);
#define RD_LOSS_FINISH(V, SL)                                                                                                 \
    RD_LAUNCH((masked_loss_finish_kernel<V, SL>), grid, dim3(256), 0, (hipStream_t)s, yp, y, mask, mean, stdv, sums, kind, delta, \
              scale, lambda, gout, loss, mae, dyp, h, w, g)
    if (vec && slope)
        RD_LOSS_FINISH(true, true);
    else if (vec)
        RD_LOSS_FINISH(true, false);
    else if (slope)
        RD_LOSS_FINISH(false, true);
    else
        RD_LOSS_FINISH(false, false);
#undef RD_LOSS_FINISH
    RD_LAUNCH_CHECK("masked_loss_finish");
    return RD_OK;
}

}  // extern "C"
