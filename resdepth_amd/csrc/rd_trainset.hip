// Training set and normalisation statistics from rasters resident in HBM (include/resdepth_hip.h: rd_patch_moments,
// rd_region_moments, rd_assemble_train_patches): the per-patch standard deviations of
// compute_local_dsm_std_per_centered_patch (lib/utils.py:111-158), the ortho-image mean / std of
// compute_satellite_image_normalization (lib/utils.py:161-200) and the 'train' samples of DsmOrthoDataset.__getitem__
// (lib/DsmOrthoDataset.py:161-291) for batches that mix several rasters (utils.get_dataloader's ConcatDataset, :256-270).
//
// Moments are CENTRED: a block owns one piece of the data (a slab of MOM_SLAB_ROWS rows of a patch, a unit of at most
// REGION_UNIT_PX pixels of a rectangle), sums it in fp64 with a fixed tree, takes the piece's mean and reads the piece a second
// time (it has just come through the caches) for sum (x - mean)^2.  The pieces of a patch / of the whole region are then merged
// in a fixed order from (count, sum, M2): with N, S the totals,  M2 = sum_p M2_p + (N s_p - n_p S)^2 / (n_p N^2)  -- for fp32
// data of a bounded range the products N s_p and n_p S are exact in fp64, so the between-piece term carries no cancellation
// error of the means.  What a piece is depends on the patch / the rectangle alone, never on the launch: results are
// independent of n, of the place in the list and of the grid.
#include "rd_common.h"
#include "rd_tile_dev.h"

namespace rd {

constexpr int MOM_SLAB_ROWS = 8;
constexpr int REGION_UNIT_PX = 16384;

// sum of v over the 256 threads of the block, to every thread: lanes by a fixed xor butterfly, the four waves in wave order
__device__ __forceinline__ double block_sum_256(double v, double* sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();                                   // the previous use of sh has been read by everyone
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// pieces first .. first + n_pieces - 1 of `ws`, each (count, sum, M2 about the piece's mean) -> (count, mean, M2), in that order
__device__ __forceinline__ void merge_pieces(const double* __restrict__ ws, long first, int n_pieces, double* __restrict__ out) {
    double N = 0.0, S = 0.0;
    for (int k = 0; k < n_pieces; ++k) {
        N += ws[(first + k) * 4];
        S += ws[(first + k) * 4 + 1];
    }
    double m2 = 0.0;
    for (int k = 0; k < n_pieces; ++k) {
        const double c = ws[(first + k) * 4], s = ws[(first + k) * 4 + 1];
        if (c > 0.0) {
            const double d = N * s - c * S;
            m2 += ws[(first + k) * 4 + 2] + d * d / (c * N * N);
        }
    }
    out[0] = N;
    out[1] = S / N;                                    // an empty set: 0 / 0 = NaN, as np.ma.mean's masked result
    out[2] = N > 0.0 ? m2 : __longlong_as_double(0x7ff8000000000000LL);
}

// ---- per-patch moments --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void patch_moments_slab(const float* __restrict__ plane, int H, int W,
                                                          const int* __restrict__ pos, int T, float nodata, int use_nodata,
                                                          int aligned, double* __restrict__ ws) {
    __shared__ double sh[4];
    const int i = blockIdx.x, slab = blockIdx.y, S = gridDim.y, t = threadIdx.x;
    const int y0 = pos[i * 2], x0 = pos[i * 2 + 1];
    const bool ok = y0 >= 0 && x0 >= 0 && y0 + T <= H && x0 + T <= W;
    const bool vec = aligned && ((x0 | W) & 3) == 0;
    const int TQ = T / 4, r0 = slab * MOM_SLAB_ROWS, rows = min(MOM_SLAB_ROWS, T - r0);
    double s = 0.0, c = 0.0;
    if (ok) {
        int r = t / TQ, q = t - r * TQ;                // (row, quad) of element t; + 256 per step without a division
        const int dr = 256 / TQ, dq = 256 - dr * TQ;
        for (; r < rows; r += dr) {
            const float4 v = ld4(plane + (long)(y0 + r0 + r) * W + x0 + q * 4, vec);
            if (!use_nodata || v.x != nodata) { s += v.x; c += 1.0; }
            if (!use_nodata || v.y != nodata) { s += v.y; c += 1.0; }
            if (!use_nodata || v.z != nodata) { s += v.z; c += 1.0; }
            if (!use_nodata || v.w != nodata) { s += v.w; c += 1.0; }
            q += dq;
            if (q >= TQ) { q -= TQ; ++r; }
        }
    }
    const double sum = block_sum_256(s, sh), cnt = block_sum_256(c, sh);
    const double mean = cnt > 0.0 ? sum / cnt : 0.0;
    double m2 = 0.0;
    if (ok) {
        int r = t / TQ, q = t - r * TQ;
        const int dr = 256 / TQ, dq = 256 - dr * TQ;
        for (; r < rows; r += dr) {
            const float4 v = ld4(plane + (long)(y0 + r0 + r) * W + x0 + q * 4, vec);
            double d;
            if (!use_nodata || v.x != nodata) { d = (double)v.x - mean; m2 += d * d; }
            if (!use_nodata || v.y != nodata) { d = (double)v.y - mean; m2 += d * d; }
            if (!use_nodata || v.z != nodata) { d = (double)v.z - mean; m2 += d * d; }
            if (!use_nodata || v.w != nodata) { d = (double)v.w - mean; m2 += d * d; }
            q += dq;
            if (q >= TQ) { q -= TQ; ++r; }
        }
    }
    m2 = block_sum_256(m2, sh);
    if (t == 0) {
        double* o = ws + ((long)i * S + slab) * 4;
        o[0] = cnt;
        o[1] = sum;
        o[2] = m2;
    }
}

__global__ __launch_bounds__(256) void patch_moments_merge(const double* __restrict__ ws, int n, int S, double* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) merge_pieces(ws, (long)i * S, S, out + (long)i * 3);
}

// ---- moments over (plane, rectangle) pairs ------------------------------------------------------------------------------
struct RegionPlan {
    int n_rects, n_planes, units_per_plane, W;
    long plane_stride;
    int y0[RD_REGION_MAX_RECTS], y1[RD_REGION_MAX_RECTS], x0[RD_REGION_MAX_RECTS], x1[RD_REGION_MAX_RECTS];
    int rows_per_unit[RD_REGION_MAX_RECTS], unit_first[RD_REGION_MAX_RECTS + 1];
    int plane[RD_REGION_MAX_PLANES];
};

// one sweep over rows [ra, rb) x columns [x0, x1) of `pl`: f(value) for every pixel; 16-byte loads over the aligned body of a row
template <typename F>
__device__ __forceinline__ void region_sweep(const float* __restrict__ pl, int W, int ra, int rb, int x0, int x1, int aligned,
                                             long plane_off, F f) {
    const int t = threadIdx.x;
    for (int r = ra; r < rb; ++r) {
        const float* p = pl + (long)r * W;
        int a = x0, b = x0;
        if (aligned) {
            a = min(x1, x0 + (int)((4 - ((plane_off + (long)r * W + x0) & 3)) & 3));
            b = a + ((x1 - a) & ~3);
        }
        for (int c = x0 + t; c < a; c += 256) f(p[c]);
        for (int c = a + 4 * t; c < b; c += 1024) {
            const float4 v = *reinterpret_cast<const float4*>(p + c);
            f(v.x); f(v.y); f(v.z); f(v.w);
        }
        for (int c = b + t; c < x1; c += 256) f(p[c]);
    }
}

__global__ __launch_bounds__(256) void region_moments_units(const float* __restrict__ planes, RegionPlan rp, int aligned,
                                                            int n_units, double* __restrict__ ws) {
    __shared__ double sh[4];
    for (int u = blockIdx.x; u < n_units; u += gridDim.x) {          // a unit's numbers do not depend on who computes it
        const int pi = u / rp.units_per_plane, rem = u - pi * rp.units_per_plane;
        int j = 0;
        while (j + 1 < rp.n_rects && rem >= rp.unit_first[j + 1]) ++j;
        const int ra = rp.y0[j] + (rem - rp.unit_first[j]) * rp.rows_per_unit[j], rb = min(rp.y1[j], ra + rp.rows_per_unit[j]);
        const long plane_off = (long)rp.plane[pi] * rp.plane_stride;
        const float* pl = planes + plane_off;
        double s = 0.0;
        region_sweep(pl, rp.W, ra, rb, rp.x0[j], rp.x1[j], aligned, plane_off, [&](float v) { s += v; });
        const double cnt = (double)(rb - ra) * (double)(rp.x1[j] - rp.x0[j]);
        const double sum = block_sum_256(s, sh), mean = sum / cnt;
        double m2 = 0.0;
        region_sweep(pl, rp.W, ra, rb, rp.x0[j], rp.x1[j], aligned, plane_off, [&](float v) {
            const double d = (double)v - mean;
            m2 += d * d;
        });
        m2 = block_sum_256(m2, sh);
        if (threadIdx.x == 0) {
            ws[(long)u * 4] = cnt;
            ws[(long)u * 4 + 1] = sum;
            ws[(long)u * 4 + 2] = m2;
        }
    }
}

// one block: thread t takes the units t, t + 256, ... in order, the 256 partial results go through the fixed tree
__global__ __launch_bounds__(256) void region_moments_merge(const double* __restrict__ ws, int n_units, double* __restrict__ out) {
    __shared__ double sh[4];
    const int t = threadIdx.x;
    double c = 0.0, s = 0.0;
    for (int u = t; u < n_units; u += 256) {
        c += ws[(long)u * 4];
        s += ws[(long)u * 4 + 1];
    }
    const double N = block_sum_256(c, sh), S = block_sum_256(s, sh);
    double m2 = 0.0;
    for (int u = t; u < n_units; u += 256) {
        const double cu = ws[(long)u * 4], d = N * ws[(long)u * 4 + 1] - cu * S;
        m2 += ws[(long)u * 4 + 2] + d * d / (cu * N * N);
    }
    m2 = block_sum_256(m2, sh);
    if (t == 0) {
        out[0] = N;
        out[1] = S / N;
        out[2] = m2;
    }
}

// ---- training batches over several rasters ------------------------------------------------------------------------------
struct TrainSample {
    int raster, y, x, aug, dsm_mode;
    float dsm_mean;
    bool ok;
};

__device__ __forceinline__ TrainSample train_sample(const int* __restrict__ samples, int n, int i, int V,
                                                    const rd_train_raster* __restrict__ rasters, int n_rasters, int T) {
    TrainSample g;
    g.raster = samples[i];
    g.y = samples[n + i];
    g.x = samples[2 * n + i];
    g.aug = samples[3 * n + i];
    g.dsm_mode = samples[4 * n + i];
    g.dsm_mean = __int_as_float(samples[5 * n + i]);
    g.ok = g.raster >= 0 && g.raster < n_rasters && g.dsm_mode >= 0 && g.dsm_mode <= 2;
    if (g.ok) {
        const rd_train_raster& R = rasters[g.raster];
        g.ok = g.y >= 0 && g.x >= 0 && g.y + T <= R.height && g.x + T <= R.width && R.dsm_in != nullptr;
        if (V > 0) g.ok = g.ok && R.ortho != nullptr;
        for (int j = 0; g.ok && j < V; ++j) {
            const int p = samples[(RD_TRAIN_SAMPLE_INTS + j) * n + i];
            g.ok = p >= 0 && p < R.n_planes;
        }
    }
    return g;
}

// sums[i] = (DSM sum, DSM count, ortho sum, ortho count) in the order of patch_sums_kernel (rd_tiles.hip): thread t adds the
// elements t, t + 256, ... of the patch, plane after plane, then the same tree_sum_256 -- what GpuPatchSampler.sample's means
// are made of, so a sample assembled here or there has the same bits.  blockIdx.y: 0 = DSM, 1 = orthos.
__global__ __launch_bounds__(256) void train_patch_sums(const rd_train_raster* __restrict__ rasters, int n_rasters,
                                                        const int* __restrict__ samples, int n, int V, int T,
                                                        double* __restrict__ sums) {
    __shared__ double red[2 * 256];
    const int i = blockIdx.x, which = blockIdx.y, t = threadIdx.x;
    const TrainSample g = train_sample(samples, n, i, V, rasters, n_rasters, T);
    double s = 0.0, c = 0.0;
    bool want = false;
    if (g.ok) {
        const rd_train_raster& R = rasters[g.raster];
        want = which == 0 ? g.dsm_mode == 2 : (V > 0 && R.ortho_mode == 2);
        if (want) {
            const int P = which == 0 ? 1 : V;
            const long plane = (long)R.height * R.width;
            const int r_first = t / T, c_first = t - r_first * T, dr = 256 / T, dc = 256 - dr * T;
            for (int p = 0; p < P; ++p) {
                const float* pl = which == 0 ? R.dsm_in : R.ortho + (long)samples[(RD_TRAIN_SAMPLE_INTS + p) * n + i] * plane;
                pl += (long)g.y * R.width + g.x;
                int r = r_first, cc = c_first;
                while (r < T) {
                    const float v = pl[(long)r * R.width + cc];
                    if (which == 1 || v != R.nodata) {
                        s += v;
                        c += 1.0;
                    }
                    r += dr;
                    cc += dc;
                    if (cc >= T) { cc -= T; ++r; }
                }
            }
        }
    }
    if (!want) return;                                   // uniform over the block
    tree_sum_256<2>({s, c}, red);
    if (t == 0) {
        sums[(long)i * 4 + which * 2] = red[0];
        sums[(long)i * 4 + which * 2 + 1] = red[256];
    }
}

// grid (sample, output plane, row block): a lane writes four adjacent output pixels (16-byte stores, 4-byte mask stores) and
// gathers their sources through aug_src; a row that is neither rotated nor mirrored left-right is one 16-byte load
// aug & RD_TRAIN_AUG_BOX: the mask is cut to the sample's box (columns RD_TRAIN_SAMPLE_INTS + V .. + 3), the 'val' samples of
// DsmOrthoDataset._get_dsm_loss_mask (lib/DsmOrthoDataset.py:434-470); an unflagged sample never touches those columns
__global__ __launch_bounds__(256) void train_patch_write(const rd_train_raster* __restrict__ rasters, int n_rasters,
                                                         const int* __restrict__ samples, int n, int V, int dsm_channel, int T,
                                                         const double* __restrict__ sums, int rows_per_block,
                                                         float* __restrict__ input, float* __restrict__ target,
                                                         uint8_t* __restrict__ mask, float* __restrict__ dsm_mean_out) {
    const int i = blockIdx.x, p = blockIdx.y, rb = blockIdx.z, t = threadIdx.x;
    const int C = dsm_channel + V;
    const TrainSample g = train_sample(samples, n, i, V, rasters, n_rasters, T);
    const float qnan = __int_as_float(0x7fc00000);
    const rd_train_raster& R = rasters[g.ok ? g.raster : 0];
    const bool is_target = p == C;
    const bool ok = g.ok && (!is_target || R.dsm_gt != nullptr);
    // the means: fp64 sums rounded once to fp32, GpuPatchSampler's (sum / count).float()
    float dmean = g.dsm_mode == 1 ? g.dsm_mean : 0.f;
    if (g.ok && g.dsm_mode == 2) dmean = (float)(sums[(long)i * 4] / sums[(long)i * 4 + 1]);
    if (p == 0 && rb == 0 && t == 0) dsm_mean_out[i] = g.ok ? dmean : qnan;
    const float* src = nullptr;
    float* dst;
    float mean = dmean, sdv = 1.f, nodata = 0.f;
    int mode = g.dsm_mode, W = 0;
    if (ok) {
        W = R.width;
        sdv = R.dsm_std;
        nodata = R.nodata;
        if (p < dsm_channel) {
            src = R.dsm_in;
        } else if (p < C) {
            src = R.ortho + (long)samples[(RD_TRAIN_SAMPLE_INTS + p - dsm_channel) * n + i] * ((long)R.height * R.width);
            mode = R.ortho_mode;
            mean = mode == 1 ? R.ortho_mean : 0.f;
            if (mode == 2) mean = (float)(sums[(long)i * 4 + 2] / sums[(long)i * 4 + 3]);
            sdv = R.ortho_std;
        } else {
            src = R.dsm_gt;
        }
        src += (long)g.y * W + g.x;
    }
    dst = is_target ? target + (long)i * T * T : input + ((long)i * C + p) * T * T;
    const int a = g.aug;
    // k == 0 (bits 0-1) and no left-right mirror (bit 3), every row of the patch 16-B aligned
    const bool vec = ok && (a & 11) == 0 && (W & 3) == 0 && ((uintptr_t)src & 15) == 0;
    const int TQ = T / 4, r0 = rb * rows_per_block, r1 = min(T, r0 + rows_per_block);
    // the mask's box in output-tile coordinates (inclusive): the whole tile, or the RD_TRAIN_AUG_BOX sample's own columns -- read
    // by the target plane of a flagged sample only; a box that is not inside the tile is empty
    int by0 = 0, bx0 = 0, by1 = T - 1, bx1 = T - 1;
    if (is_target && ok && (a & RD_TRAIN_AUG_BOX)) {
        const int* bc = samples + (long)(RD_TRAIN_SAMPLE_INTS + V) * n + i;
        by0 = bc[0];
        bx0 = bc[n];
        by1 = bc[2L * n];
        bx1 = bc[3L * n];
        if (by0 < 0 || bx0 < 0 || by1 >= T || bx1 >= T || by1 < by0 || bx1 < bx0) { by0 = bx0 = 1; by1 = bx1 = 0; }
    }
    for (int e = t; e < (r1 - r0) * TQ; e += 256) {
        const int r = r0 + e / TQ, c = (e % TQ) * 4;
        float4 v = make_float4(qnan, qnan, qnan, qnan), o = v;
        if (ok) {
            if (vec) {       // k == 0, no left-right mirror: the source row is r or its up-down mirror, columns as they are
                v = *reinterpret_cast<const float4*>(src + (long)((a & 4) ? T - 1 - r : r) * W + c);
            } else {
                float xs[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    int sr, sc;
                    aug_src(a, T, r, c + j, sr, sc);
                    xs[j] = src[(long)sr * W + sc];
                }
                v = make_float4(xs[0], xs[1], xs[2], xs[3]);
            }
            o = mode ? norm4(v, mean, sdv) : v;
        }
        *reinterpret_cast<float4*>(dst + (long)r * T + c) = o;
        if (is_target)
            *reinterpret_cast<uchar4*>(mask + (long)i * T * T + (long)r * T + c) =
                mask4(v, ok && r >= by0 && r <= by1, c, bx0, bx1, nodata);
    }
}

// ---- weight tiles (include/resdepth_hip_wloss.h) ---------------------------------------------------------------------------
// grid (sample, row block): a lane writes four adjacent output pixels (one 16-byte store) and gathers their sources through
// aug_src, the way train_patch_write orients the target plane; a row that is neither rotated nor mirrored left-right is one
// 16-byte load (fp32 weights) or one 4-byte load (class bytes, looked up in the raster's table)
__global__ __launch_bounds__(256) void train_weight_write(const rd_weight_raster* __restrict__ rasters, int n_rasters,
                                                          const int* __restrict__ samples, int n, int T, int rows_per_block,
                                                          float* __restrict__ out) {
    const int i = blockIdx.x, rb = blockIdx.y, t = threadIdx.x;
    const int id = samples[i], y0 = samples[n + i], x0 = samples[2 * n + i], a = samples[3 * n + i];
    const float qnan = __int_as_float(0x7fc00000);
    bool ok = id >= 0 && id < n_rasters;
    const rd_weight_raster& R = rasters[ok ? id : 0];
    const bool cls = R.kind == RD_WEIGHT_CLASS_U8;
    ok = ok && (R.kind == RD_WEIGHT_F32 || cls) && R.plane != nullptr && (!cls || R.table != nullptr) && y0 >= 0 && x0 >= 0 &&
         y0 + T <= R.height && x0 + T <= R.width;
    const int W = R.width;
    const float* srcf = nullptr;
    const uint8_t* srcb = nullptr;
    const float* __restrict__ tab = R.table;
    bool vec = false;
    if (ok) {
        const bool plain_rows = (a & 11) == 0 && (W & 3) == 0;      // k == 0 (bits 0-1) and no left-right mirror (bit 3)
        if (cls) {
            srcb = static_cast<const uint8_t*>(R.plane) + (long)y0 * W + x0;
            vec = plain_rows && ((uintptr_t)srcb & 3) == 0;
        } else {
            srcf = static_cast<const float*>(R.plane) + (long)y0 * W + x0;
            vec = plain_rows && ((uintptr_t)srcf & 15) == 0;
        }
    }
    float* dst = out + (long)i * T * T;
    const int TQ = T / 4, r0 = rb * rows_per_block, r1 = min(T, r0 + rows_per_block);
    for (int e = t; e < (r1 - r0) * TQ; e += 256) {
        const int r = r0 + e / TQ, c = (e % TQ) * 4;
        float4 v = make_float4(qnan, qnan, qnan, qnan);
        if (ok) {
            if (vec) {       // the source row is r or its up-down mirror, columns as they are
                const long o = (long)((a & 4) ? T - 1 - r : r) * W + c;
                if (cls) {
                    const uchar4 b = *reinterpret_cast<const uchar4*>(srcb + o);
                    v = make_float4(tab[b.x], tab[b.y], tab[b.z], tab[b.w]);
                } else {
                    v = *reinterpret_cast<const float4*>(srcf + o);
                }
            } else {
                float xs[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    int sr, sc;
                    aug_src(a, T, r, c + j, sr, sc);
                    const long o = (long)sr * W + sc;
                    xs[j] = cls ? tab[srcb[o]] : srcf[o];
                }
                v = make_float4(xs[0], xs[1], xs[2], xs[3]);
            }
        }
        *reinterpret_cast<float4*>(dst + (long)r * T + c) = v;
    }
}

static bool region_plan(RegionPlan* rp, int height, int width, long long plane_stride, const int* plane_idx, int n_planes,
                        int n_stack, const int* rects, int n_rects) {
    if (n_planes <= 0 || n_planes > RD_REGION_MAX_PLANES || n_rects <= 0 || n_rects > RD_REGION_MAX_RECTS) return false;
    rp->n_rects = n_rects;
    rp->n_planes = n_planes;
    rp->W = width;
    rp->plane_stride = (long)plane_stride;
    int first = 0;
    for (int j = 0; j < n_rects; ++j) {
        const int y0 = rects[j * 4], y1 = rects[j * 4 + 1], x0 = rects[j * 4 + 2], x1 = rects[j * 4 + 3];
        if (y0 < 0 || x0 < 0 || y1 > height || x1 > width || y0 >= y1 || x0 >= x1) return false;
        rp->y0[j] = y0; rp->y1[j] = y1; rp->x0[j] = x0; rp->x1[j] = x1;
        const int rows = REGION_UNIT_PX / (x1 - x0) < 1 ? 1 : REGION_UNIT_PX / (x1 - x0);
        rp->rows_per_unit[j] = rows;
        rp->unit_first[j] = first;
        first += cdiv(y1 - y0, rows);
    }
    rp->unit_first[n_rects] = first;
    rp->units_per_plane = first;
    for (int k = 0; k < n_planes; ++k) {
        if (plane_idx[k] < 0 || plane_idx[k] >= n_stack) return false;
        rp->plane[k] = plane_idx[k];
    }
    return (long long)first * n_planes < (1LL << 30);
}

}  // namespace rd

using namespace rd;

extern "C" {

size_t rd_patch_moments_ws_bytes(int n, int tile) {
    if (n <= 0 || tile <= 0) return 0;
    return (size_t)n * (size_t)cdiv(tile, MOM_SLAB_ROWS) * 4 * sizeof(double);
}

int rd_patch_moments(const float* plane, int height, int width, const int* pos, int n, int tile, float nodata, int use_nodata,
                     double* out, void* ws, size_t ws_bytes, rd_stream_t s) {
    RD_REQUIRE(plane && pos && out && n > 0 && height >= tile && width >= tile, "rd_patch_moments: bad arguments");
    RD_REQUIRE(tile >= 4 && tile % 4 == 0 && tile <= 1024, "rd_patch_moments: tile must be a multiple of 4 in 4..1024 (got %d)", tile);
    RD_REQUIRE(ws && ws_bytes >= rd_patch_moments_ws_bytes(n, tile), "rd_patch_moments: workspace too small (%zu < %zu bytes)",
               ws_bytes, rd_patch_moments_ws_bytes(n, tile));
    const int S = cdiv(tile, MOM_SLAB_ROWS);
    RD_REQUIRE(S <= 65535, "rd_patch_moments: tile too large");
    const int aligned = (uintptr_t)plane % 16 == 0;
    {
        ProfScope ps((hipStream_t)s, "patch_moments_slab", 0, 4.0 * n * tile * tile);
        RD_LAUNCH(patch_moments_slab, dim3(n, S), dim3(256), 0, (hipStream_t)s, plane, height, width, pos, tile, nodata, use_nodata,
                  aligned, (double*)ws);
        RD_LAUNCH_CHECK("patch_moments_slab");
    }
    RD_LAUNCH(patch_moments_merge, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)s, (const double*)ws, n, S, out);
    RD_LAUNCH_CHECK("patch_moments_merge");
    return RD_OK;
}

size_t rd_region_moments_ws_bytes(int height, int width, int n_planes, const int* rects, int n_rects) {
    RegionPlan rp;
    int none = 0;
    if (!rects || !region_plan(&rp, height, width, 0, &none, 1, 1, rects, n_rects) || n_planes <= 0) return 0;
    return (size_t)rp.units_per_plane * (size_t)n_planes * 4 * sizeof(double);
}

int rd_region_moments(const float* planes, long long plane_stride, int n_stack, int height, int width, const int* plane_idx,
                      int n_planes, const int* rects, int n_rects, double* out, void* ws, size_t ws_bytes, rd_stream_t s) {
    RD_REQUIRE(planes && plane_idx && rects && out && height > 0 && width > 0 && n_stack > 0 &&
                   plane_stride >= (long long)height * width,
               "rd_region_moments: bad arguments");
    RegionPlan rp;
    RD_REQUIRE(region_plan(&rp, height, width, plane_stride, plane_idx, n_planes, n_stack, rects, n_rects),
               "rd_region_moments: at most %d planes and %d non-empty rectangles inside the raster", RD_REGION_MAX_PLANES,
               RD_REGION_MAX_RECTS);
    const int n_units = rp.units_per_plane * n_planes;
    const size_t need = (size_t)n_units * 4 * sizeof(double);
    RD_REQUIRE(ws && ws_bytes >= need, "rd_region_moments: workspace too small (%zu < %zu bytes)", ws_bytes, need);
    const int aligned = (uintptr_t)planes % 16 == 0;
    double px = 0.0;
    for (int j = 0; j < n_rects; ++j) px += (double)(rp.y1[j] - rp.y0[j]) * (rp.x1[j] - rp.x0[j]);
    {
        ProfScope ps((hipStream_t)s, "region_moments_units", 0, 4.0 * px * n_planes);
        RD_LAUNCH(region_moments_units, dim3(n_units < 8192 ? n_units : 8192), dim3(256), 0, (hipStream_t)s, planes, rp, aligned,
                  n_units, (double*)ws);
        RD_LAUNCH_CHECK("region_moments_units");
    }
    RD_LAUNCH(region_moments_merge, dim3(1), dim3(256), 0, (hipStream_t)s, (const double*)ws, n_units, out);
    RD_LAUNCH_CHECK("region_moments_merge");
    return RD_OK;
}

int rd_assemble_train_patches(const rd_train_raster* rasters, int n_rasters, const int* samples, int n, int views, int dsm_channel,
                              int tile, float* input, float* target, uint8_t* mask, float* dsm_mean_out, double* sums,
                              rd_stream_t s) {
    RD_REQUIRE(rasters && n_rasters > 0 && samples && input && dsm_mean_out && sums && n > 0 && views >= 0,
               "rd_assemble_train_patches: bad arguments");
    RD_REQUIRE(tile >= 4 && tile % 4 == 0 && tile <= 1024,
               "rd_assemble_train_patches: tile must be a multiple of 4 in 4..1024 (got %d)", tile);
    RD_REQUIRE((dsm_channel == 0 || dsm_channel == 1) && dsm_channel + views >= 1 && dsm_channel + views + 1 <= 65535,
               "rd_assemble_train_patches: no input channel");
    RD_REQUIRE((target == nullptr) == (mask == nullptr), "rd_assemble_train_patches: target and mask go together");
    RD_REQUIRE(((uintptr_t)input | (uintptr_t)target) % 16 == 0 && (uintptr_t)mask % 4 == 0,
               "rd_assemble_train_patches: input / target must be 16-byte aligned, mask 4-byte aligned");
    const double px = (double)n * tile * tile;
    {
        ProfScope ps((hipStream_t)s, "train_patch_sums", 0, 4.0 * px * (1 + views));
        RD_LAUNCH(train_patch_sums, dim3(n, views > 0 ? 2 : 1), dim3(256), 0, (hipStream_t)s, rasters, n_rasters, samples, n, views,
                  tile, sums);
        RD_LAUNCH_CHECK("train_patch_sums");
    }
    const int planes_out = dsm_channel + views + (target ? 1 : 0);
    const int rows_per_block = tile_rows_per_block(tile);
    ProfScope ps((hipStream_t)s, "train_patch_write", 0, px * (8.0 * planes_out + (target ? 1.0 : 0.0)));
    RD_LAUNCH(train_patch_write, dim3(n, planes_out, cdiv(tile, rows_per_block)), dim3(256), 0, (hipStream_t)s, rasters, n_rasters,
              samples, n, views, dsm_channel, tile, (const double*)sums, rows_per_block, input, target, mask, dsm_mean_out);
    RD_LAUNCH_CHECK("train_patch_write");
    return RD_OK;
}

int rd_assemble_train_weights(const rd_weight_raster* rasters, int n_rasters, const int* samples, int n, int views, int tile,
                              float* out, rd_stream_t s) {
    RD_REQUIRE(rasters && n_rasters > 0 && samples && out && n > 0 && views >= 0, "rd_assemble_train_weights: bad arguments");
    RD_REQUIRE(tile >= 4 && tile % 4 == 0 && tile <= 1024,
               "rd_assemble_train_weights: tile must be a multiple of 4 in 4..1024 (got %d)", tile);
    RD_REQUIRE((uintptr_t)out % 16 == 0, "rd_assemble_train_weights: out must be 16-byte aligned");
    const int rows_per_block = tile_rows_per_block(tile);
    ProfScope ps((hipStream_t)s, "train_weight_write", 0, 8.0 * (double)n * tile * tile);
    RD_LAUNCH(train_weight_write, dim3(n, cdiv(tile, rows_per_block)), dim3(256), 0, (hipStream_t)s, rasters, n_rasters, samples,
              n, tile, rows_per_block, out);
    RD_LAUNCH_CHECK("train_weight_write");
    return RD_OK;
}

}  // extern "C"
