// Masked, de-normalised training losses beyond L1 (include/resdepth_hip_loss.h): a quadratic / Huber / L1 data term plus an optional
// term on the first differences of the residual, and the masked MAE next to the loss.  Generalises the l1_* kernels of
// rd_elementwise.hip (Trainer._compute_denormalized_loss, lib/Trainer.py:87-100, with any criterion); DESIGN.md section 3.9.
//
// A block walks tiles of TR x TC pixels, each inside one sample.  The residual r (fp32, the roundings of `denorm` below) and the
// mask of the tile and of a one-pixel ring around it are staged in LDS once; every neighbour is read from there.  Cells outside
// the sample are staged with m = 0, so the stencil needs no bounds test of its own and a pair can neither cross a sample
// boundary nor wrap a row.  Sums are fp64, added in a fixed order (thread -> block tree -> one block over the per-block sums).
//
// The per-pixel weighted forms (include/resdepth_hip_wloss.h) are the WT = true instantiations of the same templates: a weight
// plane w is staged beside r and m (cells outside the sample with w = 0), a sixth sum Wc = sum m w joins the five, Q becomes the
// fp64 sum of the pair weights.  With w == 1 every extra operation is an exact multiplication by 1.0 in the same place of the
// same order, so both families give the same bits.
#include "rd_common.h"

using namespace rd;

namespace {

constexpr int TR = RD_LOSS_STRIP_ROWS, TC = RD_LOSS_STRIP_COLS;
constexpr int LROWS = TR + 2, PITCH = TC + 2;       // staged cell (lr, lc) is pixel (r0 + lr - 1, c0 + lc - 1)
constexpr int NSUM = 5;                             // A, C, D, S, Q
constexpr int NSUM_W = 6;                           // ... and Wc (weighted forms)
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

template <bool WT>
__device__ __forceinline__ void stage_cell(float* sr, uint8_t* sm, float* sw, int lr, int lc, int gr, int gc, int h, int w,
                                           const float* __restrict__ yp, const float* __restrict__ y,
                                           const uint8_t* __restrict__ mask, const float* __restrict__ wt, long base, float sd,
                                           float mu) {
    float r = 0.f, wv = 0.f;
    uint8_t m = 0;
    if (gr >= 0 && gr < h && gc >= 0 && gc < w) {
        const long e = base + (long)gr * w + gc;
        m = mask[e] != 0;
        r = denorm(yp[e], sd, mu) - denorm(y[e], sd, mu);
        if (WT) wv = wt[e];
    }
    sr[lr * PITCH + lc] = r;
    sm[lr * PITCH + lc] = m;
    if (WT) sw[lr * PITCH + lc] = wv;
}

// ring == false: the forward counts each pair once from its upper / left pixel, so the row above and the column left of the
// tile are not needed (staged as invalid without touching memory)
template <bool VEC, bool WT>
__device__ __forceinline__ void stage_tile(float* sr, uint8_t* sm, float* sw, bool ring, int r0, int c0, int h, int w,
                                           const float* __restrict__ yp, const float* __restrict__ y,
                                           const uint8_t* __restrict__ mask, const float* __restrict__ wt, long base, float sd,
                                           float mu) {
    if (VEC) {
        for (int i = threadIdx.x; i < TR * (TC / 4); i += 256) {
            const int row = i / (TC / 4), q = i - row * (TC / 4);
            const int gr = r0 + row, gc = c0 + 4 * q;
            float r[4] = {0.f, 0.f, 0.f, 0.f}, wv[4] = {0.f, 0.f, 0.f, 0.f};
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
                if (WT) {
                    const float4 ww = *reinterpret_cast<const float4*>(wt + e);
                    wv[0] = ww.x, wv[1] = ww.y, wv[2] = ww.z, wv[3] = ww.w;
                }
            }
            const int o = (row + 1) * PITCH + 1 + 4 * q;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sr[o + j] = r[j];
                sm[o + j] = m[j];
                if (WT) sw[o + j] = wv[j];
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
            stage_cell<WT>(sr, sm, sw, lr, lc, skip ? -1 : r0 + lr - 1, c0 + lc - 1, h, w, yp, y, mask, wt, base, sd, mu);
        }
    } else {
        for (int i = threadIdx.x; i < LROWS * PITCH; i += 256) {
            const int lr = i / PITCH, lc = i - lr * PITCH;
            const bool skip = !ring && (lr == 0 || lc == 0);
            stage_cell<WT>(sr, sm, sw, lr, lc, skip ? -1 : r0 + lr - 1, c0 + lc - 1, h, w, yp, y, mask, wt, base, sd, mu);
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

// pair weight of two staged cells: omega = (w_a + w_b) / 2 in fp64 (exact: the sum of two floats, halved)
__device__ __forceinline__ double pair_weight(float wa, float wb) { return 0.5 * ((double)wa + (double)wb); }

template <bool VEC, bool WT>
__global__ __launch_bounds__(256) void masked_loss_partial_kernel(const float* __restrict__ yp, const float* __restrict__ y,
                                                                  const uint8_t* __restrict__ mask,
                                                                  const float* __restrict__ wt,
                                                                  const float* __restrict__ mean,
                                                                  const float* __restrict__ stdv, double* __restrict__ partial,
                                                                  int h, int w, Geo g, int kind, double delta) {
    constexpr int NS = WT ? NSUM_W : NSUM;
    __shared__ float sr[LROWS * PITCH];
    __shared__ uint8_t sm[LROWS * PITCH];
    __shared__ float sw[WT ? LROWS * PITCH : 1];
    __shared__ double red[NS * 256];
    double A = 0.0, D = 0.0, S = 0.0, Qw = 0.0, Wc = 0.0;
    int C = 0, Q = 0;
    for (int t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        int n, r0, c0;
        tile_of(t, g, n, r0, c0);
        __syncthreads();                 // the previous tile has been read
        stage_tile<VEC, WT>(sr, sm, sw, false, r0, c0, h, w, yp, y, mask, wt, (long)n * h * w, stdv[n], mean[n]);
        __syncthreads();
        for (int i = threadIdx.x; i < TR * TC; i += 256) {
            const int o = (i / TC + 1) * PITCH + (i % TC) + 1;
            if (!sm[o]) continue;
            const float r = sr[o];
            const double ar = fabs((double)r);
            A += ar;
            C += 1;
            if (WT) {
                const float we = sw[o];
                D += (double)we * rho(ar, kind, delta);
                Wc += (double)we;
                if (sm[o + 1]) {
                    const double om = pair_weight(we, sw[o + 1]);
                    S += om * (double)fabsf(r - sr[o + 1]);
                    Qw += om;
                }
                if (sm[o + PITCH]) {
                    const double om = pair_weight(we, sw[o + PITCH]);
                    S += om * (double)fabsf(r - sr[o + PITCH]);
                    Qw += om;
                }
            } else {
                D += rho(ar, kind, delta);
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
    }
    const int t = threadIdx.x;
    red[t] = A, red[256 + t] = (double)C, red[512 + t] = D, red[768 + t] = S, red[1024 + t] = WT ? Qw : (double)Q;
    if (WT) red[1280 + t] = Wc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) {
#pragma unroll
            for (int k = 0; k < NS; ++k) red[k * 256 + t] += red[k * 256 + t + off];
        }
        __syncthreads();
    }
    if (t < NS) partial[(long)blockIdx.x * NS + t] = red[t * 256];
}

template <int NS>
__global__ __launch_bounds__(256) void masked_loss_reduce_kernel(const double* __restrict__ partial, double* __restrict__ sums,
                                                                 int nb, double scale) {
    __shared__ double red[NS * 256];
    const int t = threadIdx.x;
    double v[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) v[k] = 0.0;
    for (int b = t; b < nb; b += 256) {
#pragma unroll
        for (int k = 0; k < NS; ++k) v[k] += partial[(long)b * NS + k];
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) red[k * 256 + t] = v[k];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) {
#pragma unroll
            for (int k = 0; k < NS; ++k) red[k * 256 + t] += red[k * 256 + t + off];
        }
        __syncthreads();
    }
    if (t < 8) sums[t] = t < NS ? (t == 2 ? red[t * 256] * scale : red[t * 256]) : 0.0;
}

template <bool VEC, bool SLOPE, bool WT>
__global__ __launch_bounds__(256) void masked_loss_finish_kernel(const float* __restrict__ yp, const float* __restrict__ y,
                                                                 const uint8_t* __restrict__ mask,
                                                                 const float* __restrict__ wt,
                                                                 const float* __restrict__ mean,
                                                                 const float* __restrict__ stdv, const double* __restrict__ sums,
                                                                 int kind, double delta, double scale, double lambda,
                                                                 const float* __restrict__ gout_dev, float* __restrict__ loss,
                                                                 float* __restrict__ mae, float* __restrict__ dyp, int h, int w,
                                                                 Geo g) {
    __shared__ float sr[SLOPE ? LROWS * PITCH : 1];
    __shared__ uint8_t sm[SLOPE ? LROWS * PITCH : 1];
    __shared__ float sw[SLOPE && WT ? LROWS * PITCH : 1];
    const double A = sums[0], C = sums[1], D = sums[2], S = sums[3], Q = sums[4];
    const double Dn = WT ? sums[5] : C;          // what the data term is divided by: Wc = sum m w, or C
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (loss) loss[0] = (float)(D / Dn + ((lambda > 0.0 && Q > 0.0) ? lambda * S / Q : 0.0));
        if (mae) mae[0] = (float)(A / C);
    }
    if (!dyp) return;
    const double gout = gout_dev ? (double)gout_dev[0] : 1.0;
    // WT: Wc == 0 with valid pixels (all of them weighted 0) must give zeros, not 0 * inf
    const double cd = (!WT || Dn > 0.0) ? scale / Dn : 0.0;
    const double cs = (SLOPE && Q > 0.0) ? lambda / Q : 0.0;
    for (int t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        int n, r0, c0;
        tile_of(t, g, n, r0, c0);
        const long base = (long)n * h * w;
        const float sd = stdv[n], mu = mean[n];
        const double gs = gout * (double)sd;
        if (SLOPE) {
            __syncthreads();
            stage_tile<VEC, WT>(sr, sm, sw, true, r0, c0, h, w, yp, y, mask, wt, base, sd, mu);
            __syncthreads();
        }
        // gradient of the staged cell o (SLOPE) -- data part plus the stencil, one multiplication each, one rounding.  The
        // stencil is an integer, or (WT) the fp64 sum of omega * sign over left, right, upper, lower neighbour in that order
        auto staged = [&](int o) -> float {
            if (!sm[o]) return 0.f;
            const float r = sr[o];
            if (WT) {
                const float we = sw[o];
                double K = 0.0;
                if (sm[o - 1]) K += pair_weight(we, sw[o - 1]) * (double)((r > sr[o - 1]) - (r < sr[o - 1]));
                if (sm[o + 1]) K += pair_weight(we, sw[o + 1]) * (double)((r > sr[o + 1]) - (r < sr[o + 1]));
                if (sm[o - PITCH]) K += pair_weight(we, sw[o - PITCH]) * (double)((r > sr[o - PITCH]) - (r < sr[o - PITCH]));
                if (sm[o + PITCH]) K += pair_weight(we, sw[o + PITCH]) * (double)((r > sr[o + PITCH]) - (r < sr[o + PITCH]));
                return (float)(gs * (cd * ((double)we * rho_prime(r, kind, delta)) + cs * K));
            }
            int k = 0;
            if (sm[o - 1]) k += (r > sr[o - 1]) - (r < sr[o - 1]);
            if (sm[o + 1]) k += (r > sr[o + 1]) - (r < sr[o + 1]);
            if (sm[o - PITCH]) k += (r > sr[o - PITCH]) - (r < sr[o - PITCH]);
            if (sm[o + PITCH]) k += (r > sr[o + PITCH]) - (r < sr[o + PITCH]);
            return (float)(gs * (cd * rho_prime(r, kind, delta) + cs * (double)k));
        };
        auto direct = [&](float a, float b, uint8_t m, float we) -> float {
            if (!m) return 0.f;
            if (WT) return (float)(gs * (cd * ((double)we * rho_prime(denorm(a, sd, mu) - denorm(b, sd, mu), kind, delta))));
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
                    float4 ww = make_float4(1.f, 1.f, 1.f, 1.f);
                    if (WT) ww = *reinterpret_cast<const float4*>(wt + e);
                    o4 = make_float4(direct(a.x, b.x, mm.x, ww.x), direct(a.y, b.y, mm.y, ww.y), direct(a.z, b.z, mm.z, ww.z),
                                     direct(a.w, b.w, mm.w, ww.w));
                }
                *reinterpret_cast<float4*>(dyp + e) = o4;
            }
        } else {
            for (int i = threadIdx.x; i < TR * TC; i += 256) {
                const int row = i / TC, col = i % TC;
                const int gr = r0 + row, gc = c0 + col;
                if (gr >= h || gc >= w) continue;
                const long e = base + (long)gr * w + gc;
                dyp[e] = SLOPE ? staged((row + 1) * PITCH + col + 1) : direct(yp[e], y[e], mask[e], WT ? wt[e] : 1.f);
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

// the two launches of a partial pass; wt == nullptr: the unweighted family (five sums per block), else six
int launch_partial(const char* who, const float* yp, const float* y, const uint8_t* mask, const float* wt, const float* mean,
                   const float* stdv, double* sums, int n, int h, int w, int kind, double delta, double scale, void* ws,
                   size_t ws_bytes, rd_stream_t s) {
    Geo g;
    RD_REQUIRE(yp && y && mask && mean && stdv && sums && make_geo(n, h, w, &g), "%s: bad arguments", who);
    RD_REQUIRE(kind_ok(kind, delta, scale), "%s: unknown kind, delta <= 0 or scale <= 0", who);
    const int nb = loss_grid(g), ns = wt ? NSUM_W : NSUM;
    if (!ws || ws_bytes < (size_t)nb * ns * sizeof(double)) {
        set_error("%s: workspace too small", who);
        return RD_ERR_WS;
    }
    const bool vec = w % 4 == 0 && aligned(yp, 16) && aligned(y, 16) && aligned(mask, 4) && aligned(wt, 16);
    ProfScope ps((hipStream_t)s, wt ? "weighted_loss" : "masked_loss", 0, (wt ? 13.0 : 9.0) * (double)n * h * w);
#define RD_LOSS_PARTIAL(V, WT)                                                                                               \
    RD_LAUNCH((masked_loss_partial_kernel<V, WT>), dim3(nb), dim3(256), 0, (hipStream_t)s, yp, y, mask, wt, mean, stdv,       \
              (double*)ws, h, w, g, kind, delta)
    if (wt) {
        if (vec)
            RD_LOSS_PARTIAL(true, true);
        else
            RD_LOSS_PARTIAL(false, true);
        RD_LAUNCH(masked_loss_reduce_kernel<NSUM_W>, dim3(1), dim3(256), 0, (hipStream_t)s, (const double*)ws, sums, nb, scale);
    } else {
        if (vec)
            RD_LOSS_PARTIAL(true, false);
        else
            RD_LOSS_PARTIAL(false, false);
        RD_LAUNCH(masked_loss_reduce_kernel<NSUM>, dim3(1), dim3(256), 0, (hipStream_t)s, (const double*)ws, sums, nb, scale);
    }
#undef RD_LOSS_PARTIAL
    RD_LAUNCH_CHECK(who);
    return RD_OK;
}

int launch_finish(const char* who, const float* yp, const float* y, const uint8_t* mask, const float* wt, const float* mean,
                  const float* stdv, const double* sums, double numel_total, int kind, double delta, double scale, double lambda,
                  const float* gout, float* loss, float* mae, float* dyp, int n, int h, int w, rd_stream_t s) {
    Geo g;
    RD_REQUIRE(yp && y && mask && mean && stdv && sums && make_geo(n, h, w, &g), "%s: bad arguments", who);
    RD_REQUIRE(kind_ok(kind, delta, scale), "%s: unknown kind, delta <= 0 or scale <= 0", who);
    RD_REQUIRE(numel_total > 0.0 && lambda >= 0.0 && lambda <= 1.7e308, "%s: numel_total <= 0 or bad lambda", who);
    const bool vec = w % 4 == 0 && aligned(yp, 16) && aligned(y, 16) && aligned(mask, 4) && aligned(dyp, 16) && aligned(wt, 16);
    const bool slope = lambda > 0.0;
    const dim3 grid(dyp ? loss_grid(g) : 1);
    ProfScope ps((hipStream_t)s, wt ? "weighted_loss" : "masked_loss", 0, (wt ? 17.0 : 13.0) * (double)n * h * w);
#define RD_LOSS_FINISH(V, SL, WT)                                                                                             \
    RD_LAUNCH((masked_loss_finish_kernel<V, SL, WT>), grid, dim3(256), 0, (hipStream_t)s, yp, y, mask, wt, mean, stdv, sums, kind, \
              delta, scale, lambda, gout, loss, mae, dyp, h, w, g)
#define RD_LOSS_FINISH_BY(WT)         \
    do {                              \
        if (vec && slope)             \
            RD_LOSS_FINISH(true, true, WT);   \
        else if (vec)                 \
            RD_LOSS_FINISH(true, false, WT);  \
        else if (slope)               \
            RD_LOSS_FINISH(false, true, WT);  \
        else                          \
            RD_LOSS_FINISH(false, false, WT); \
    } while (0)
    if (wt)
        RD_LOSS_FINISH_BY(true);
    else
        RD_LOSS_FINISH_BY(false);
#undef RD_LOSS_FINISH_BY
#undef RD_LOSS_FINISH
    RD_LAUNCH_CHECK(who);
    return RD_OK;
}

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
    return launch_partial("rd_masked_loss_partial", yp, y, mask, nullptr, mean, stdv, sums, n, h, w, kind, delta, scale, ws,
                          ws_bytes, s);
}

int rd_masked_loss_finish(const float* yp, const float* y, const uint8_t* mask, const float* mean, const float* stdv,
                          const double* sums, double numel_total, int kind, double delta, double scale, double lambda,
                          const float* gout, float* loss, float* mae, float* dyp, int n, int h, int w, rd_stream_t s) {
    return launch_finish("rd_masked_loss_finish", yp, y, mask, nullptr, mean, stdv, sums, numel_total, kind, delta, scale, lambda,
                         gout, loss, mae, dyp, n, h, w, s);
}

size_t rd_weighted_loss_ws_bytes(int n, int h, int w) {
    Geo g;
    if (!make_geo(n, h, w, &g)) return 0;
    return (size_t)loss_grid(g) * NSUM_W * sizeof(double);
}

int rd_weighted_loss_partial(const float* yp, const float* y, const uint8_t* mask, const float* weight, const float* mean,
                             const float* stdv, double* sums, int n, int h, int w, int kind, double delta, double scale, void* ws,
                             size_t ws_bytes, rd_stream_t s) {
    RD_REQUIRE(weight, "rd_weighted_loss_partial: bad arguments");
    return launch_partial("rd_weighted_loss_partial", yp, y, mask, weight, mean, stdv, sums, n, h, w, kind, delta, scale, ws,
                          ws_bytes, s);
}

int rd_weighted_loss_finish(const float* yp, const float* y, const uint8_t* mask, const float* weight, const float* mean,
                            const float* stdv, const double* sums, double numel_total, int kind, double delta, double scale,
                            double lambda, const float* gout, float* loss, float* mae, float* dyp, int n, int h, int w,
                            rd_stream_t s) {
    RD_REQUIRE(weight, "rd_weighted_loss_finish: bad arguments");
    return launch_finish("rd_weighted_loss_finish", yp, y, mask, weight, mean, stdv, sums, numel_total, kind, delta, scale,
                         lambda, gout, loss, mae, dyp, n, h, w, s);
}

}  // extern "C"
