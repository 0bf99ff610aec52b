// The tile data path (gfx950): what cuts network inputs out of rasters resident in HBM and puts predictions back.
//   * tiled inference: the linear blend of predicted tiles into an fp64 raster (lib/evaluation.py:497-511), plain, for tiles
//     predicted in any of the square's eight orientations (test-time augmentation) and into one raster per image pair;
//   * training samples of one raster: per-patch sums and the assembled, augmented patches (GpuPatchSampler);
//   * validation / inference grid tiles (lib/DsmOrthoDataset.py:161-291, sampling_strategy 'val' / 'test'), plain and oriented.
//   * the ortho planes themselves: raw views ortho-rectified onto the DSM grid through their RPC camera models (last section).
// Training batches that mix several rasters are rd_trainset.hip's; the pieces both share (the D4 maps, the four-pixel blocks,
// the 256-leaf tree, a tile's means) live in rd_tile_dev.h, once.  All of it is HBM-bound gather / scatter with fixed-order
// fp64 sums: no float atomics, results independent of the launch shape.
#include "rd_common.h"
#include "rd_tile_dev.h"

namespace rd {

// ---- tiled inference: linear blend --------------------------------------------------------------
__device__ __forceinline__ double blend_axis(int c, int lo, int hi, int T, int overlap, double step) {
    // np.linspace(0, 1, overlap): ramp[i] = i * step, last element exactly 1
    double w = 1.0;
    if (lo > 0) {
        if (c < lo - overlap) return 0.0;
        if (c < lo) {
            const int i = c - (lo - overlap);
            w *= (i == overlap - 1 && overlap > 1) ? 1.0 : i * step;
        }
    }
    if (hi < T - 1 && c > hi) {
        const int i = overlap - 1 - (c - hi - 1);
        w *= (i < 0) ? 0.0 : ((i == overlap - 1 && overlap > 1) ? 1.0 : i * step);
    }
    return w;
}

// All tiles of a batch in ONE launch with the accumulation order of per-tile launches (tile 0, 1, 2, ... per raster
// pixel: the reference's order, lib/evaluation.py:497-511).  Thread (tile i, pixel e) OWNS its raster pixel iff no earlier
// tile of the batch covers it; the owner adds the contributions of tiles i, i+1, ... that cover the pixel, in order, and
// every other thread exits -- no atomics, no inter-thread ordering needed, any tile placement (overlapping areas, shifted
// border tiles) works.
__global__ __launch_bounds__(256) void blend_batch_kernel(const float* __restrict__ pred, const float* __restrict__ mean,
                                                          const float* __restrict__ stdv, const int* __restrict__ pos,
                                                          const int* __restrict__ reg, int n, int T, int stride,
                                                          double* __restrict__ raster, int rows, int cols) {
    const long e_all = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e_all >= (long)n * T * T) return;
    const int i = (int)(e_all / ((long)T * T)), e = (int)(e_all - (long)i * T * T);
    const int r = e / T, c = e - r * T;
    const int y = pos[i * 2] + r, x = pos[i * 2 + 1] + c;
    if ((unsigned)y >= (unsigned)rows || (unsigned)x >= (unsigned)cols) return;
    for (int j = 0; j < i; ++j)
        if ((unsigned)(y - pos[j * 2]) < (unsigned)T && (unsigned)(x - pos[j * 2 + 1]) < (unsigned)T) return;   // not the owner
    const int overlap = T - stride;
    const double step = overlap > 1 ? 1.0 / (double)(overlap - 1) : 0.0;
    double acc = raster[(long)y * cols + x];
    for (int j = i; j < n; ++j) {
        const int rj = y - pos[j * 2], cj = x - pos[j * 2 + 1];
        if ((unsigned)rj >= (unsigned)T || (unsigned)cj >= (unsigned)T) continue;
        const double w = blend_axis(rj, reg[j * 4], reg[j * 4 + 2], T, overlap, step) *
                         blend_axis(cj, reg[j * 4 + 1], reg[j * 4 + 3], T, overlap, step);
        const float den = __fadd_rn(__fmul_rn(pred[((long)j * T + rj) * T + cj], stdv[j]), mean[j]);
        acc += (double)den * w;
    }
    raster[(long)y * cols + x] = acc;
}

// ---- test-time augmentation (the orientation codes and aug_src / aug_dst: rd_tile_dev.h) ---------------------------------
// rd_blend_accumulate_tta: blend_batch_kernel for oriented predictions.  Block (tile i = first + blockIdx.y, 32 x 32 cell of
// it); a thread holds four raster pixels of the cell (one column, rows 8 apart) and OWNS a pixel iff no tile first <= j < i
// covers it; owners add the tiles j = i .. last - 1 that cover the pixel, in order -- the per-pixel order of
// blend_batch_kernel, no atomics.  The block walks j together: the part of pred[j] that lands on the cell is an axis-aligned
// rectangle of pred[j] (<= 32 x 32), read row by row into LDS (128-B runs whatever the orientation) and picked up through
// aug_dst.  LDS row stride 33 dwords: lanes of a row differ in the LDS column (even k) or the LDS row (odd k), either way
// 32 distinct banks for ds_read_b32 / ds_write_b32.  Raster: 32 doubles = 256-B runs per row, read once and written once.
constexpr int TTA_CELL = 32;

// acc + den * w * scale in ONE rounding: the blend kernels above compile `acc += (double)den * w` to v_fmac_f64 (-ffp-contract=on),
// and den * scale (a power of two) is exact -- so this is scale x their step, bit for bit, whatever the compiler contracts here
__device__ __forceinline__ double blend_tta_add(double acc, float den, double w, double scale) {
    return fma((double)den * scale, w, acc);
}

//
// PLANES (rd_blend_accumulate_planes): sample i goes into raster + plane[i] * plane_stride, one of n_planes rasters of
// rows x cols.  Samples of different planes never meet: sample j < i takes a pixel from sample i only if plane[j] == plane[i],
// and an owner adds only the samples of its own plane -- so every plane sees its own samples in their order, as if the others
// were not in the call.  A plane index outside 0 .. n_planes - 1 owns nothing and equals no valid plane: the sample is skipped.
// Without PLANES the kernel is rd_blend_accumulate_tta's, instruction for instruction.
template <bool PLANES>
__global__ __launch_bounds__(256) void blend_tta_kernel(const float* __restrict__ pred, const float* __restrict__ mean,
                                                        const float* __restrict__ stdv, const int* __restrict__ pos,
                                                        const int* __restrict__ reg, const int* __restrict__ aug,
                                                        const int* __restrict__ plane, int first, int last, int T, int stride,
                                                        double scale, double* __restrict__ raster, int n_planes,
                                                        long plane_stride, int rows, int cols) {
    __shared__ float stage[TTA_CELL * (TTA_CELL + 1)];
    const int i = first + blockIdx.y, t = threadIdx.x;
    const int pl = PLANES && plane ? plane[i] : 0;
    if (PLANES) {
        if ((unsigned)pl >= (unsigned)n_planes) return;    // uniform over the block, before any barrier
        raster += (long)pl * plane_stride;
    }
    const int cells = (T + TTA_CELL - 1) / TTA_CELL;
    const int R0 = (blockIdx.x / cells) * TTA_CELL, C0 = (blockIdx.x % cells) * TTA_CELL;
    const int Y0 = pos[i * 2] + R0, X0 = pos[i * 2 + 1] + C0;                       // the cell's raster rectangle
    const int h = min(TTA_CELL, T - R0), w = min(TTA_CELL, T - C0);
    const int lc = t & 31, lr = t >> 5, x = X0 + lc;
    bool own[4];
    double acc[4];
    bool any = false;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int y = Y0 + lr + 8 * q;
        own[q] = lc < w && lr + 8 * q < h && (unsigned)y < (unsigned)rows && (unsigned)x < (unsigned)cols;
        for (int j = first; own[q] && j < i; ++j)
            if ((unsigned)(y - pos[j * 2]) < (unsigned)T && (unsigned)(x - pos[j * 2 + 1]) < (unsigned)T &&
                (!PLANES || !plane || plane[j] == pl))
                own[q] = false;
        acc[q] = own[q] ? raster[(long)y * cols + x] : 0.0;
        any = any || own[q];
    }
    if (!__syncthreads_or(any)) return;
    const int overlap = T - stride;
    const double step = overlap > 1 ? 1.0 / (double)(overlap - 1) : 0.0;
    for (int j = i; j < last; ++j) {
        if (PLANES && plane && plane[j] != pl) continue;   // another plane's sample: uniform over the block
        const int yj = pos[j * 2], xj = pos[j * 2 + 1];
        // the cell's part of tile j, in tile j's plain coordinates [a0, a1) x [b0, b1): uniform over the block
        const int a0 = max(Y0 - yj, 0), a1 = min(Y0 + h - yj, T), b0 = max(X0 - xj, 0), b1 = min(X0 + w - xj, T);
        if (a0 >= a1 || b0 >= b1) continue;
        const int a = aug ? aug[j] & 15 : 0;
        int p0, q0, p1, q1;
        aug_dst(a, T, a0, b0, p0, q0);
        aug_dst(a, T, a1 - 1, b1 - 1, p1, q1);
        const int pr = min(p0, p1), pc = min(q0, q1), ph = abs(p1 - p0) + 1, pw = abs(q1 - q0) + 1;
        __syncthreads();                                   // the previous tile's picks are done
        const float* src = pred + (long)j * T * T;
        for (int e = t; e < ph * pw; e += 256) {
            const int er = e / pw, ec = e - er * pw;
            stage[er * (TTA_CELL + 1) + ec] = src[(long)(pr + er) * T + pc + ec];
        }
        __syncthreads();
        const float sj = stdv[j], mj = mean[j];
        const int uly = reg[j * 4], ulx = reg[j * 4 + 1], lry = reg[j * 4 + 2], lrx = reg[j * 4 + 3];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int rj = Y0 + lr + 8 * q - yj, cj = x - xj;
            if (!own[q] || rj < a0 || rj >= a1 || cj < b0 || cj >= b1) continue;
            int r, c;
            aug_dst(a, T, rj, cj, r, c);
            const double wgt = blend_axis(rj, uly, lry, T, overlap, step) * blend_axis(cj, ulx, lrx, T, overlap, step);
            const float den = __fadd_rn(__fmul_rn(stage[(r - pr) * (TTA_CELL + 1) + c - pc], sj), mj);
            acc[q] = blend_tta_add(acc[q], den, wgt, scale);
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (own[q]) raster[(long)(Y0 + lr + 8 * q) * cols + x] = acc[q];
}

// ---- training-sample assembly -----------------------------------------------------------------------
// thread t adds the elements t, t + 256, ... of the patch, plane after plane, then the 256-leaf tree (train_patch_sums of
// rd_trainset.hip keeps this order, so a sample assembled here or there has the same means)
__global__ __launch_bounds__(256) void patch_sums_kernel(const float* __restrict__ planes, long plane_stride,
                                                         const int* __restrict__ plane_idx, int P,
                                                         const int* __restrict__ pos, int T, int W, float nodata,
                                                         int use_nodata, double* __restrict__ sums) {
    __shared__ double red[2 * 256];
    const int i = blockIdx.x, y0 = pos[i * 2], x0 = pos[i * 2 + 1];
    double s = 0.0, c = 0.0;
    for (int p = 0; p < P; ++p) {
        const float* pl = planes + (long)plane_idx[i * P + p] * plane_stride;
        for (int e = threadIdx.x; e < T * T; e += 256) {
            const float v = pl[(long)(y0 + e / T) * W + x0 + e % T];
            if (!use_nodata || v != nodata) {
                s += v;
                c += 1.0;
            }
        }
    }
    tree_sum_256<2>({s, c}, red);
    if (threadIdx.x == 0) {
        sums[i * 2] = red[0];
        sums[i * 2 + 1] = red[256];
    }
}

__global__ __launch_bounds__(256) void assemble_patches_kernel(
    const float* __restrict__ dsm_in, const float* __restrict__ dsm_gt, const float* __restrict__ ortho, long plane_stride,
    const int* __restrict__ pair_idx, int V, const int* __restrict__ pos, const int* __restrict__ aug,
    const float* __restrict__ dsm_mean, float dsm_std, const float* __restrict__ ortho_mean, float ortho_std, float nodata,
    int n, int T, int W, float* __restrict__ input, float* __restrict__ target, uint8_t* __restrict__ mask) {
    const int C = 1 + V;
    const long total = (long)n * (C + 1) * T * T;    // channel C = the target / mask plane
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int c = (int)(e % T), r = (int)((e / T) % T);
        const int ch = (int)((e / ((long)T * T)) % (C + 1));
        const int i = (int)(e / ((long)T * T * (C + 1)));
        if (ch == C && !dsm_gt) continue;
        int sr, sc;
        aug_src(aug ? aug[i] : 0, T, r, c, sr, sc);
        const long src = (long)(pos[i * 2] + sr) * W + pos[i * 2 + 1] + sc;
        if (ch == 0) {
            input[((long)i * C) * T * T + (long)r * T + c] = __fdiv_rn(__fsub_rn(dsm_in[src], dsm_mean[i]), dsm_std);
        } else if (ch < C) {
            const float v = ortho[(long)pair_idx[i * V + ch - 1] * plane_stride + src];
            input[((long)i * C + ch) * T * T + (long)r * T + c] = __fdiv_rn(__fsub_rn(v, ortho_mean[i]), ortho_std);
        } else {
            const float g = dsm_gt[src];
            target[(long)i * T * T + (long)r * T + c] = __fdiv_rn(__fsub_rn(g, dsm_mean[i]), dsm_std);
            mask[(long)i * T * T + (long)r * T + c] = (g != 0.f && g != nodata) ? 1 : 0;
        }
    }
}

// ---- validation / inference grid tiles (lib/DsmOrthoDataset.py:161-291, sampling_strategy 'val' / 'test') ------------
// Sample row (RD_GRID_SAMPLE_INTS ints): uly, ulx, box uly, box ulx, box lry, box lrx (tile coordinates, inclusive), image-pair
// index, unused.  Two kernels: grid_tile_sums writes fp64 partial sums per (tile, slab of GRID_SLAB_ROWS rows) with a fixed
// in-block tree; grid_tile_write adds the slab partials of its tile in slab order, so a tile's mean depends on the tile's
// pixels and T alone (not on the batch, the tile's place in it or the launch shape).  A lane owns four adjacent pixels:
// 16-B loads when the source rows are 16-B aligned (ulx, W and the plane stride multiples of 4), else four 4-B loads;
// 16-B stores, 4-B mask stores.
constexpr int GRID_SLAB_ROWS = 8;

struct GridSample {
    int uly, ulx, b_uly, b_ulx, b_lry, b_lrx, pair;
    bool ok, vec;
};

__device__ __forceinline__ GridSample grid_sample(const int* __restrict__ samples, int i, const int* __restrict__ pair_planes,
                                                  int n_pairs, int V, int n_planes, int H, int W, long plane_stride, int T,
                                                  int aligned) {
    const int* s = samples + (long)i * RD_GRID_SAMPLE_INTS;
    GridSample g;
    g.uly = s[0]; g.ulx = s[1]; g.b_uly = s[2]; g.b_ulx = s[3]; g.b_lry = s[4]; g.b_lrx = s[5]; g.pair = s[6];
    g.ok = g.uly >= 0 && g.ulx >= 0 && g.uly + T <= H && g.ulx + T <= W;
    if (V > 0) {
        g.ok = g.ok && g.pair >= 0 && g.pair < n_pairs;
        for (int j = 0; g.ok && j < V; ++j) {
            const int p = pair_planes[g.pair * V + j];
            g.ok = p >= 0 && p < n_planes;
        }
    }
    g.vec = aligned && ((g.ulx | W | (int)(plane_stride & 3)) & 3) == 0;
    return g;
}

__global__ __launch_bounds__(256) void grid_tile_sums(const float* __restrict__ dsm_in, const float* __restrict__ ortho,
                                                      long plane_stride, int H, int W, int n_planes,
                                                      const int* __restrict__ samples, const int* __restrict__ pair_planes,
                                                      int n_pairs, int V, int T, float nodata, int want_dsm, int want_ortho,
                                                      int aligned, double* __restrict__ ws) {
    __shared__ double red[3 * 256];
    const int i = blockIdx.x, slab = blockIdx.y, S = gridDim.y, t = threadIdx.x;
    const GridSample g = grid_sample(samples, i, pair_planes, n_pairs, V, n_planes, H, W, plane_stride, T, aligned);
    double sd = 0.0, cd = 0.0, so = 0.0;
    if (g.ok) {
        const int TQ = T / 4;
        for (int e = t; e < GRID_SLAB_ROWS * TQ; e += 256) {
            const int r = slab * GRID_SLAB_ROWS + e / TQ, c = (e % TQ) * 4;
            const long off = (long)(g.uly + r) * W + g.ulx + c;
            if (want_dsm) {
                const float4 v = ld4(dsm_in + off, g.vec);
                if (v.x != nodata) { sd += v.x; cd += 1.0; }
                if (v.y != nodata) { sd += v.y; cd += 1.0; }
                if (v.z != nodata) { sd += v.z; cd += 1.0; }
                if (v.w != nodata) { sd += v.w; cd += 1.0; }
            }
            if (want_ortho) {
                for (int j = 0; j < V; ++j) {
                    const float4 v = ld4(ortho + (long)pair_planes[g.pair * V + j] * plane_stride + off, g.vec);
                    so += v.x; so += v.y; so += v.z; so += v.w;
                }
            }
        }
    }
    tree_sum_256<3>({sd, cd, so}, red);
    if (t < 3) ws[((long)i * S + slab) * 4 + t] = red[t * 256];
}

__global__ __launch_bounds__(256) void grid_tile_write(
    const float* __restrict__ dsm_in, const float* __restrict__ dsm_gt, const float* __restrict__ ortho, long plane_stride,
    int H, int W, int n_planes, const int* __restrict__ samples, const int* __restrict__ pair_planes, int n_pairs, int V,
    int dsm_channel, int T, int S, float nodata, int dsm_mode, float dsm_mean_fixed, float dsm_std, int ortho_mode,
    float ortho_mean_fixed, float ortho_std, int aligned, const double* __restrict__ ws, int rows_per_block, float* __restrict__ input,
    float* __restrict__ target, uint8_t* __restrict__ mask, float* __restrict__ dsm_mean_out) {
    const int i = blockIdx.x, p = blockIdx.y, rb = blockIdx.z, t = threadIdx.x;
    const int C = dsm_channel + V;
    const GridSample g = grid_sample(samples, i, pair_planes, n_pairs, V, n_planes, H, W, plane_stride, T, aligned);
    float dmean, omean;
    grid_tile_means(ws, i, S, V, T, dsm_mode, dsm_mean_fixed, ortho_mode, ortho_mean_fixed, p >= dsm_channel && p < C, dmean, omean);
    if (p == 0 && rb == 0 && t == 0) dsm_mean_out[i] = g.ok ? dmean : __int_as_float(0x7fc00000);
    const float* src;
    float* dst;
    float mean = dmean, sdv = dsm_std;
    int mode = dsm_mode;
    if (p < dsm_channel) {
        src = dsm_in;
        dst = input + ((long)i * C + p) * T * T;
    } else if (p < C) {
        src = g.ok ? ortho + (long)pair_planes[g.pair * V + p - dsm_channel] * plane_stride : ortho;
        dst = input + ((long)i * C + p) * T * T;
        mean = omean;
        sdv = ortho_std;
        mode = ortho_mode;
    } else {
        src = dsm_gt;
        dst = target + (long)i * T * T;
    }
    const bool is_target = p == C;
    const int TQ = T / 4, r0 = rb * rows_per_block, r1 = min(T, r0 + rows_per_block);
    const float qnan = __int_as_float(0x7fc00000);
    for (int e = t; e < (r1 - r0) * TQ; e += 256) {
        const int r = r0 + e / TQ, c = (e % TQ) * 4;
        float4 v = make_float4(qnan, qnan, qnan, qnan), o = v;
        if (g.ok) {
            v = ld4(src + (long)(g.uly + r) * W + g.ulx + c, g.vec);
            o = mode ? norm4(v, mean, sdv) : v;
        }
        *reinterpret_cast<float4*>(dst + (long)r * T + c) = o;
        if (is_target)     // the non-overlap box of the sample row
            *reinterpret_cast<uchar4*>(mask + (long)i * T * T + (long)r * T + c) =
                mask4(v, g.ok && r >= g.b_uly && r <= g.b_lry, c, g.b_ulx, g.b_lrx, nodata);
    }
}

// rd_assemble_grid_tiles_aug: grid_tile_write for prediction tiles in a given orientation (no target / mask).  The means are
// grid_tile_write's (the slab partials of grid_tile_sums over the untransformed pixels, in slab order), every pixel goes
// through the same sub / div, so an oriented tile is the permutation of the plain one bit for bit.  Block (sample, plane,
// GRID_AUG_CELL^2 cell of the OUTPUT tile): the cell's source is an axis-aligned rectangle of the raster (sides swapped for odd
// k), read row by row (256-B runs) into LDS and written out row by row through aug_src (256-B runs).  LDS row stride 65
// dwords: the lanes of an output row differ in the LDS column (even k) or the LDS row (odd k) -- 32 distinct banks per half
// wave either way.
constexpr int GRID_AUG_CELL = 64;

__global__ __launch_bounds__(256) void grid_tile_write_aug(
    const float* __restrict__ dsm_in, const float* __restrict__ ortho, long plane_stride, int H, int W, int n_planes,
    const int* __restrict__ samples, const int* __restrict__ pair_planes, int n_pairs, int V, int dsm_channel, int T, int S,
    int dsm_mode, float dsm_mean_fixed, float dsm_std, int ortho_mode, float ortho_mean_fixed, float ortho_std,
    const double* __restrict__ ws, const int* __restrict__ aug, float* __restrict__ input, float* __restrict__ dsm_mean_out) {
    __shared__ float stage[GRID_AUG_CELL * (GRID_AUG_CELL + 1)];
    const int i = blockIdx.x, p = blockIdx.y, t = threadIdx.x;
    const int C = dsm_channel + V;
    const GridSample g = grid_sample(samples, i, pair_planes, n_pairs, V, n_planes, H, W, plane_stride, T, 0);
    float dmean, omean;
    grid_tile_means(ws, i, S, V, T, dsm_mode, dsm_mean_fixed, ortho_mode, ortho_mean_fixed, p >= dsm_channel, dmean, omean);
    if (p == 0 && blockIdx.z == 0 && t == 0) dsm_mean_out[i] = g.ok ? dmean : __int_as_float(0x7fc00000);
    const bool is_dsm = p < dsm_channel;
    const float* src = is_dsm ? dsm_in : (g.ok ? ortho + (long)pair_planes[g.pair * V + p - dsm_channel] * plane_stride : ortho);
    const float mean = is_dsm ? dmean : omean, sdv = is_dsm ? dsm_std : ortho_std;
    const int mode = is_dsm ? dsm_mode : ortho_mode;
    float* dst = input + ((long)i * C + p) * T * T;
    const int cells = (T + GRID_AUG_CELL - 1) / GRID_AUG_CELL;
    const int R0 = (blockIdx.z / cells) * GRID_AUG_CELL, C0 = (blockIdx.z % cells) * GRID_AUG_CELL;
    const int h = min(GRID_AUG_CELL, T - R0), w = min(GRID_AUG_CELL, T - C0);
    const int a = aug ? aug[i] & 15 : 0;
    int p0, q0, p1, q1;
    aug_src(a, T, R0, C0, p0, q0);
    aug_src(a, T, R0 + h - 1, C0 + w - 1, p1, q1);
    const int sr0 = min(p0, p1), sc0 = min(q0, q1), sh = abs(p1 - p0) + 1, sw = abs(q1 - q0) + 1;
    if (g.ok) {
        // no loop vectoriser: it pairs the sub of two iterations into v_pk_add_f32 (csrc/build.sh: no packed-f32 VALU anywhere)
#pragma clang loop vectorize(disable)
        for (int e = t; e < sh * sw; e += 256) {
            const int er = e / sw, ec = e - er * sw;
            const float v = src[(long)(g.uly + sr0 + er) * W + g.ulx + sc0 + ec];
            stage[er * (GRID_AUG_CELL + 1) + ec] = mode ? __fdiv_rn(__fsub_rn(v, mean), sdv) : v;
        }
    }
    __syncthreads();
    for (int e = t; e < h * w; e += 256) {
        const int er = e / w, ec = e - er * w;
        int sr, sc;
        aug_src(a, T, R0 + er, C0 + ec, sr, sc);
        dst[(long)(R0 + er) * T + C0 + ec] = g.ok ? stage[(sr - sr0) * (GRID_AUG_CELL + 1) + sc - sc0] : __int_as_float(0x7fc00000);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
// what the three blend entry points check alike, under the caller's name (the plain blend has no variants: 0)
static int blend_check(const char* name, const float* pred, const float* mean, const float* stdv, const int* pos, const int* reg,
                       int n, int tile_size, int stride, int log2_variants, const double* raster, int rows, int cols) {
    RD_REQUIRE(pred && mean && stdv && pos && reg && raster, "%s: null pointer", name);
    RD_REQUIRE(n > 0 && tile_size > 0 && stride > 0 && stride <= tile_size && rows > 0 && cols > 0,
               "%s: bad shape (n=%d tile=%d stride=%d raster=%dx%d)", name, n, tile_size, stride, rows, cols);
    RD_REQUIRE(log2_variants >= 0 && log2_variants <= 4, "%s: log2_variants must be in 0..4 (got %d)", name, log2_variants);
    return RD_OK;
}

// launches of up to 64 samples, in order: within one the owner threads walk the covering samples in order, and a later
// launch adds after an earlier one -- rd_blend_accumulate's per-pixel order for any n
template <bool PLANES>
static void blend_tta_launches(const float* pred, const float* mean, const float* stdv, const int* pos, const int* reg,
                               const int* aug, const int* plane, int n, int tile_size, int stride, int log2_variants,
                               double* raster, int n_planes, long plane_stride, int rows, int cols, hipStream_t s) {
    const int cells = cdiv(tile_size, TTA_CELL);
    const double scale = 1.0 / (double)(1 << log2_variants);
    for (int first = 0; first < n; first += 64) {
        const int last = first + 64 < n ? first + 64 : n;
        RD_LAUNCH(blend_tta_kernel<PLANES>, dim3(cells * cells, last - first), dim3(256), 0, s, pred, mean, stdv, pos, reg, aug,
                  plane, first, last, tile_size, stride, scale, raster, n_planes, plane_stride, rows, cols);
    }
}

// what rd_assemble_grid_tiles and rd_assemble_grid_tiles_aug do alike, under the caller's name: the checks in the plain entry
// point's order (`plain`: those of its target / mask outputs, which the oriented one refuses beforehand) and grid_tile_sums
// with the same arguments -- the same partials, so the same means.  *aligned_out: 16-B loads need 16-B aligned rasters (a
// caller's view may start anywhere), else every tile takes the 4-B loads
static int grid_tiles_begin(const char* name, bool plain, const float* dsm_in, const float* dsm_gt, const float* ortho_planes,
                            int n_planes, int height, int width, const int* samples, const int* pair_planes, int n_pairs, int views,
                            int dsm_channel, int n, int tile, float nodata, int dsm_mode, int ortho_mode, const float* input,
                            const float* target, const uint8_t* mask, const float* dsm_mean_out, void* ws, size_t ws_bytes,
                            int* aligned_out, hipStream_t s) {
    RD_REQUIRE(dsm_in && samples && input && dsm_mean_out && n > 0 && height >= tile && width >= tile && views >= 0,
               "%s: bad arguments", name);
    RD_REQUIRE(tile >= GRID_SLAB_ROWS && tile % GRID_SLAB_ROWS == 0, "%s: tile must be a positive multiple of %d (got %d)", name,
               GRID_SLAB_ROWS, tile);
    RD_REQUIRE((dsm_channel == 0 || dsm_channel == 1) && dsm_channel + views >= 1, "%s: no input channel", name);
    RD_REQUIRE(views == 0 || (ortho_planes && pair_planes && n_pairs > 0 && n_planes > 0), "%s: ortho inputs missing", name);
    RD_REQUIRE(!plain || !dsm_gt || (target && mask), "%s: target / mask outputs missing", name);
    RD_REQUIRE(dsm_mode >= 0 && dsm_mode <= 2 && ortho_mode >= 0 && ortho_mode <= 2, "%s: bad mode", name);
    const int want_dsm = dsm_mode == 2, want_ortho = ortho_mode == 2 && views > 0;
    if (want_dsm || want_ortho)
        RD_REQUIRE(ws && ws_bytes >= rd_assemble_grid_tiles_ws_bytes(n, tile), "%s: workspace too small (%zu < %zu bytes)", name,
                   ws_bytes, rd_assemble_grid_tiles_ws_bytes(n, tile));
    RD_REQUIRE(!plain || (((uintptr_t)input | (uintptr_t)target) % 16 == 0 && (uintptr_t)mask % 4 == 0),
               "%s: input / target must be 16-byte aligned, mask 4-byte aligned", name);
    *aligned_out = (((uintptr_t)dsm_in | (uintptr_t)(plain ? dsm_gt : nullptr) | (uintptr_t)ortho_planes) % 16) == 0;
    if (want_dsm || want_ortho) {
        ProfScope ps(s, "grid_tile_sums", 0, 4.0 * n * tile * tile * (want_dsm + (want_ortho ? views : 0)));
        RD_LAUNCH(grid_tile_sums, dim3(n, tile / GRID_SLAB_ROWS), dim3(256), 0, s, dsm_in, ortho_planes, (long)height * width,
                  height, width, n_planes, samples, pair_planes, n_pairs, views, tile, nodata, want_dsm, want_ortho, *aligned_out,
                  (double*)ws);
        RD_LAUNCH_CHECK("grid_tile_sums");
    }
    return RD_OK;
}

}  // namespace rd

using namespace rd;

extern "C" {

int rd_blend_accumulate(const float* pred, const float* mean, const float* stdv, const int* pos, const int* reg, int n,
                        int tile_size, int stride, double* raster, int rows, int cols, rd_stream_t s) {
    if (int rc = blend_check("rd_blend_accumulate", pred, mean, stdv, pos, reg, n, tile_size, stride, 0, raster, rows, cols)) return rc;
    ProfScope ps((hipStream_t)s, "blend_accumulate", 0, 20.0 * n * tile_size * tile_size);
    // launches of up to 64 tiles, in order (the owner threads of one walk its covering tiles in order; more tiles would make
    // that walk long): a later launch adds after an earlier one, so every raster pixel sees tile 0, 1, 2, ... for any n
    for (int first = 0; first < n; first += 64) {
        const int m = first + 64 < n ? 64 : n - first;
        const long total = (long)m * tile_size * tile_size;
        RD_LAUNCH(blend_batch_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)s,
                  pred + (long)first * tile_size * tile_size, mean + first, stdv + first, pos + 2 * first, reg + 4 * first, m,
                  tile_size, stride, raster, rows, cols);
    }
    RD_LAUNCH_CHECK("blend_accumulate");
    return RD_OK;
}

int rd_blend_accumulate_tta(const float* pred, const float* mean, const float* stdv, const int* pos, const int* reg,
                            const int* aug, int n, int tile_size, int stride, int log2_variants, double* raster, int rows,
                            int cols, rd_stream_t s) {
    if (int rc = blend_check("rd_blend_accumulate_tta", pred, mean, stdv, pos, reg, n, tile_size, stride, log2_variants, raster,
                             rows, cols))
        return rc;
    ProfScope ps((hipStream_t)s, "blend_accumulate_tta", 0, 20.0 * n * tile_size * tile_size);
    blend_tta_launches<false>(pred, mean, stdv, pos, reg, aug, nullptr, n, tile_size, stride, log2_variants, raster, 1, 0L, rows,
                              cols, (hipStream_t)s);
    RD_LAUNCH_CHECK("blend_accumulate_tta");
    return RD_OK;
}

int rd_blend_accumulate_planes(const float* pred, const float* mean, const float* stdv, const int* pos, const int* reg,
                               const int* aug, const int* plane, int n, int tile_size, int stride, int log2_variants,
                               double* raster, int n_planes, long long plane_stride, int rows, int cols, rd_stream_t s) {
    if (int rc = blend_check("rd_blend_accumulate_planes", pred, mean, stdv, pos, reg, n, tile_size, stride, log2_variants, raster,
                             rows, cols))
        return rc;
    RD_REQUIRE(n_planes >= 1 && plane_stride >= (long long)rows * cols,
               "rd_blend_accumulate_planes: n_planes must be positive and plane_stride >= rows x cols (n_planes=%d "
               "plane_stride=%lld raster=%dx%d)", n_planes, plane_stride, rows, cols);
    ProfScope ps((hipStream_t)s, "blend_accumulate_planes", 0, 20.0 * n * tile_size * tile_size);
    blend_tta_launches<true>(pred, mean, stdv, pos, reg, aug, plane, n, tile_size, stride, log2_variants, raster, n_planes,
                             (long)plane_stride, rows, cols, (hipStream_t)s);
    RD_LAUNCH_CHECK("blend_accumulate_planes");
    return RD_OK;
}

int rd_patch_sums(const float* planes, long long plane_stride, const int* plane_idx, int p_per_patch, const int* pos,
                  int n, int tile, int width, float nodata, int use_nodata, double* sums, rd_stream_t s) {
    RD_REQUIRE(planes && plane_idx && pos && sums && n > 0 && tile > 0 && width >= tile && p_per_patch > 0,
               "rd_patch_sums: bad arguments");
    ProfScope ps((hipStream_t)s, "patch_sums", 0, 4.0 * n * p_per_patch * tile * tile);
    RD_LAUNCH(patch_sums_kernel, dim3(n), dim3(256), 0, (hipStream_t)s, planes, (long)plane_stride, plane_idx,
                       p_per_patch, pos, tile, width, nodata, use_nodata, sums);
    RD_LAUNCH_CHECK("patch_sums");
    return RD_OK;
}

int rd_assemble_patches(const float* dsm_in, const float* dsm_gt, const float* ortho_planes, long long plane_stride,
                        const int* pair_idx, int views, const int* pos, const int* aug, const float* dsm_mean,
                        float dsm_std, const float* ortho_mean, float ortho_std, float nodata, int n, int tile, int width,
                        float* input, float* target, uint8_t* mask, rd_stream_t s) {
    RD_REQUIRE(dsm_in && pos && dsm_mean && input && n > 0 && tile > 0 && width >= tile && views >= 0,
               "rd_assemble_patches: bad arguments");
    RD_REQUIRE(views == 0 || (ortho_planes && pair_idx && ortho_mean), "rd_assemble_patches: ortho inputs missing");
    RD_REQUIRE(!dsm_gt || (target && mask), "rd_assemble_patches: target / mask outputs missing");
    const long total = (long)n * (views + 2) * tile * tile;
    ProfScope ps((hipStream_t)s, "assemble_patches", 0, 8.0 * total);
    RD_LAUNCH(assemble_patches_kernel, dim3(grid_cap((total + 255) / 256, 8192)), dim3(256), 0, (hipStream_t)s,
                       dsm_in, dsm_gt, ortho_planes, (long)plane_stride, pair_idx, views, pos, aug, dsm_mean, dsm_std,
                       ortho_mean, ortho_std, nodata, n, tile, width, input, target, mask);
    RD_LAUNCH_CHECK("assemble_patches");
    return RD_OK;
}

size_t rd_assemble_grid_tiles_ws_bytes(int n, int tile) {
    if (n <= 0 || tile <= 0) return 0;
    return (size_t)n * (size_t)((tile + GRID_SLAB_ROWS - 1) / GRID_SLAB_ROWS) * 4 * sizeof(double);
}

int rd_assemble_grid_tiles(const float* dsm_in, const float* dsm_gt, const float* ortho_planes, int n_planes, int height,
                           int width, const int* samples, const int* pair_planes, int n_pairs, int views, int dsm_channel,
                           int n, int tile, float nodata, int dsm_mode, float dsm_mean, float dsm_std, int ortho_mode,
                           float ortho_mean, float ortho_std, float* input, float* target, uint8_t* mask, float* dsm_mean_out,
                           void* ws, size_t ws_bytes, rd_stream_t s) {
    int aligned;
    if (int rc = grid_tiles_begin("rd_assemble_grid_tiles", true, dsm_in, dsm_gt, ortho_planes, n_planes, height, width, samples,
                                  pair_planes, n_pairs, views, dsm_channel, n, tile, nodata, dsm_mode, ortho_mode, input, target,
                                  mask, dsm_mean_out, ws, ws_bytes, &aligned, (hipStream_t)s))
        return rc;
    const int planes_out = dsm_channel + views + (dsm_gt ? 1 : 0), rows_per_block = tile_rows_per_block(tile);
    ProfScope ps((hipStream_t)s, "grid_tile_write", 0, (double)n * tile * tile * (8.0 * planes_out + (dsm_gt ? 1.0 : 0.0)));
    RD_LAUNCH(grid_tile_write, dim3(n, planes_out, cdiv(tile, rows_per_block)), dim3(256), 0, (hipStream_t)s, dsm_in, dsm_gt,
              ortho_planes, (long)height * width, height, width, n_planes, samples, pair_planes, n_pairs, views, dsm_channel, tile,
              tile / GRID_SLAB_ROWS, nodata, dsm_mode, dsm_mean, dsm_std, ortho_mode, ortho_mean, ortho_std, aligned,
              (const double*)ws, rows_per_block, input, target, mask, dsm_mean_out);
    RD_LAUNCH_CHECK("grid_tile_write");
    return RD_OK;
}

int rd_assemble_grid_tiles_aug(const float* dsm_in, const float* dsm_gt, const float* ortho_planes, int n_planes, int height,
                               int width, const int* samples, const int* pair_planes, int n_pairs, int views, int dsm_channel,
                               int n, int tile, float nodata, int dsm_mode, float dsm_mean, float dsm_std, int ortho_mode,
                               float ortho_mean, float ortho_std, const int* aug, float* input, float* target, uint8_t* mask,
                               float* dsm_mean_out, void* ws, size_t ws_bytes, rd_stream_t s) {
    RD_REQUIRE(!target && !mask, "rd_assemble_grid_tiles_aug: oriented tiles are for prediction, target / mask must be null");
    int aligned;        // of dsm_in and the orthos: dsm_gt is accepted for the symmetry of the two signatures, nothing is cut from it
    if (int rc = grid_tiles_begin("rd_assemble_grid_tiles_aug", false, dsm_in, dsm_gt, ortho_planes, n_planes, height, width,
                                  samples, pair_planes, n_pairs, views, dsm_channel, n, tile, nodata, dsm_mode, ortho_mode, input,
                                  target, mask, dsm_mean_out, ws, ws_bytes, &aligned, (hipStream_t)s))
        return rc;
    const int planes_out = dsm_channel + views, cells = cdiv(tile, GRID_AUG_CELL);
    ProfScope ps((hipStream_t)s, "grid_tile_write_aug", 0, (double)n * tile * tile * 8.0 * planes_out);
    RD_LAUNCH(grid_tile_write_aug, dim3(n, planes_out, cells * cells), dim3(256), 0, (hipStream_t)s, dsm_in, ortho_planes,
              (long)height * width, height, width, n_planes, samples, pair_planes, n_pairs, views, dsm_channel, tile,
              tile / GRID_SLAB_ROWS, dsm_mode, dsm_mean, dsm_std, ortho_mode, ortho_mean, ortho_std, (const double*)ws, aug, input,
              dsm_mean_out);
    RD_LAUNCH_CHECK("grid_tile_write_aug");
    return RD_OK;
}

}  // extern "C"

// ---- ortho-rectification through RPC camera models (include/resdepth_hip_ortho.h) ------------------------------------------------
// What makes the ortho planes the kernels above cut tiles from.  ortho_rpc_kernel: one thread per DSM pixel takes the ground point
// to degrees once (the inverse Krueger series for a UTM grid) and walks the views: the rational polynomial projection in fp64,
// then a gather of up to 16 taps of the image.  The model is read through wave-uniform addresses (scalar loads), the taps go
// through the cache, and out / valid / coords stream out with non-temporal stores.  Every loop but the one over the views has
// a compile-time trip count and constant indices, so the monomials and the taps stay in registers: no scratch.
namespace rd {

// how a wave's 64 pixels lie on the grid (ORTHO_FW x ORTHO_FH) and the four waves of a block beside or above one another
// (64 x 1, 16 x 4 and 8 x 8 were measured, DESIGN 3.6f: the kernel is bound by its fp64 arithmetic, the first two tie and 8 x 8 is
// 2-5 % slower; the row of 64 is the one that is built)
constexpr int ORTHO_FW = 64, ORTHO_FH = 64 / ORTHO_FW;
constexpr int ORTHO_WX = ORTHO_FW >= 64 ? 1 : 4, ORTHO_WY = 4 / ORTHO_WX;
constexpr int ORTHO_TW = ORTHO_FW * ORTHO_WX, ORTHO_TH = ORTHO_FH * ORTHO_WY;
static_assert(ORTHO_FW * ORTHO_FH == 64 && ORTHO_WX * ORTHO_WY == 4, "a block is four waves of 64 pixels");
static_assert(sizeof(rd_ortho_view) == 776, "rd_ortho_view is packed by resdepth_amd/ortho.py as 776 bytes");

// WGS84 and the Krueger series to n^4
constexpr double KR_F = 1.0 / 298.257223563, KR_N = KR_F / (2.0 - KR_F), KR_N2 = KR_N * KR_N, KR_N3 = KR_N2 * KR_N, KR_N4 = KR_N2 * KR_N2;
constexpr double KR_E2 = KR_F * (2.0 - KR_F), KR_E = 0.08181919084262149;       // the first eccentricity and its square
static_assert(KR_E * KR_E - KR_E2 < 1e-17 && KR_E2 - KR_E * KR_E < 1e-17, "KR_E is the root of KR_E2");
constexpr double KR_K0A = 0.9996 * (6378137.0 / (1.0 + KR_N) * (1.0 + KR_N2 / 4.0 + KR_N4 / 64.0));
constexpr double KR_B1 = KR_N / 2.0 - 2.0 * KR_N2 / 3.0 + 37.0 * KR_N3 / 96.0 - KR_N4 / 360.0;
constexpr double KR_B2 = KR_N2 / 48.0 + KR_N3 / 15.0 - 437.0 * KR_N4 / 1440.0;
constexpr double KR_B3 = 17.0 * KR_N3 / 480.0 - 37.0 * KR_N4 / 840.0;
constexpr double KR_B4 = 4397.0 * KR_N4 / 161280.0;
constexpr double KR_DEG = 57.29577951308232;                                    // 180 / pi

__device__ __forceinline__ void st_nt_u8(uint8_t* p, uint8_t v) {
#ifdef RD_NO_NT
    *p = v;
#else
    __builtin_nontemporal_store(v, p);
#endif
}
__device__ __forceinline__ void st_nt_f64(double* p, double v) {
#ifdef RD_NO_NT
    *p = v;
#else
    __builtin_nontemporal_store(v, p);
#endif
}

// easting / northing -> degrees
__device__ __forceinline__ void ortho_utm_inverse(double X, double Y, double lon0_deg, double false_northing, double& lon,
                                                  double& lat) {
    const double xi = (Y - false_northing) / KR_K0A, eta = (X - 500000.0) / KR_K0A;
    double s2, c2;
    sincos(2.0 * xi, &s2, &c2);
    const double sh2 = sinh(2.0 * eta), ch2 = cosh(2.0 * eta);
    // the multiples 4, 6, 8 by the addition theorems
    const double s4 = 2.0 * s2 * c2, c4 = 1.0 - 2.0 * s2 * s2, sh4 = 2.0 * sh2 * ch2, ch4 = 1.0 + 2.0 * sh2 * sh2;
    const double s6 = s4 * c2 + c4 * s2, c6 = c4 * c2 - s4 * s2, sh6 = sh4 * ch2 + ch4 * sh2, ch6 = ch4 * ch2 + sh4 * sh2;
    const double s8 = 2.0 * s4 * c4, c8 = 1.0 - 2.0 * s4 * s4, sh8 = 2.0 * sh4 * ch4, ch8 = 1.0 + 2.0 * sh4 * sh4;
    const double xip = xi - (KR_B1 * s2 * ch2 + KR_B2 * s4 * ch4 + KR_B3 * s6 * ch6 + KR_B4 * s8 * ch8);
    const double etap = eta - (KR_B1 * c2 * sh2 + KR_B2 * c4 * sh4 + KR_B3 * c6 * sh6 + KR_B4 * c8 * sh8);
    double sx, cx;
    sincos(xip, &sx, &cx);
    const double she = sinh(etap);
    const double taup = sx / sqrt(she * she + cx * cx);                          // tangent of the conformal latitude
    double tau = taup;
#pragma unroll
    for (int it = 0; it < 3; ++it) {                                            // Newton on tau = tan(lat)
        const double root = sqrt(1.0 + tau * tau);
        const double sigma = sinh(KR_E * atanh(KR_E * tau / root));
        const double t = tau * sqrt(1.0 + sigma * sigma) - sigma * root;
        tau += (taup - t) / sqrt(1.0 + t * t) * (1.0 + (1.0 - KR_E2) * tau * tau) / ((1.0 - KR_E2) * root);
    }
    lat = atan(tau) * KR_DEG;
    lon = lon0_deg + atan2(she, cx) * KR_DEG;
}

__device__ __forceinline__ double ortho_poly(const double* __restrict__ k, const double (&m)[20]) {
    double s = k[0];
#pragma unroll
    for (int i = 1; i < 20; ++i) s += k[i] * m[i];
    return s;
}

template <int DT>
__device__ __forceinline__ double ortho_tap(const void* __restrict__ img, long at) {
    if (DT == RD_ORTHO_U8) return (double)((const uint8_t*)img)[at];
    if (DT == RD_ORTHO_U16) return (double)((const uint16_t*)img)[at];
    return (double)((const float*)img)[at];
}

// the value at (yi, xi) of a rows x cols image -> whether it is defined.  Nothing outside the image is read: the bounds of the
// needed taps are settled first, as doubles (NaN and the infinities fail them).
template <int RS, int DT>
__device__ __forceinline__ bool ortho_resample(const void* __restrict__ img, long pitch, int rows, int cols, double nd, double yi,
                                               double xi, double& val) {
    if (RS == RD_ORTHO_NEAREST) {
        const double yn = floor(yi + 0.5), xn = floor(xi + 0.5);
        if (!(yn >= 0.0 && xn >= 0.0 && yn <= (double)(rows - 1) && xn <= (double)(cols - 1))) return false;
        val = ortho_tap<DT>(img, (long)(int)yn * pitch + (int)xn);
        return !(val == nd);
    }
    const double y0 = floor(yi), x0 = floor(xi);
    const double fy = yi - y0, fx = xi - x0;
    const bool two_x = fx != 0.0, two_y = fy != 0.0;
    if (RS == RD_ORTHO_BILINEAR) {
        if (!(y0 >= 0.0 && x0 >= 0.0 && y0 <= (double)(rows - (two_y ? 2 : 1)) && x0 <= (double)(cols - (two_x ? 2 : 1)))) return false;
        const long at = (long)(int)y0 * pitch + (int)x0;
        const double v00 = ortho_tap<DT>(img, at);
        const double v01 = two_x ? ortho_tap<DT>(img, at + 1) : v00;
        const double v10 = two_y ? ortho_tap<DT>(img, at + pitch) : v00;
        const double v11 = two_x && two_y ? ortho_tap<DT>(img, at + pitch + 1) : v00;
        const double top = two_x ? v00 + fx * (v01 - v00) : v00;
        const double bot = two_x ? v10 + fx * (v11 - v10) : v10;
        val = two_y ? top + fy * (bot - top) : top;
        return !(v00 == nd || v01 == nd || v10 == nd || v11 == nd);
    }
    // Catmull-Rom: rows y0 - 1 .. y0 + 2 (y0 alone with fy == 0), columns likewise
    const double ly = two_y ? 1.0 : 0.0, hy = two_y ? 3.0 : 1.0, lx = two_x ? 1.0 : 0.0, hx = two_x ? 3.0 : 1.0;
    if (!(y0 >= ly && x0 >= lx && y0 <= (double)rows - hy && x0 <= (double)cols - hx)) return false;
    const long at = (long)(int)y0 * pitch + (int)x0;
    const double wx[4] = {((-0.5 * fx + 1.0) * fx - 0.5) * fx, (1.5 * fx - 2.5) * fx * fx + 1.0, ((-1.5 * fx + 2.0) * fx + 0.5) * fx,
                          (0.5 * fx - 0.5) * fx * fx};
    const double wy[4] = {((-0.5 * fy + 1.0) * fy - 0.5) * fy, (1.5 * fy - 2.5) * fy * fy + 1.0, ((-1.5 * fy + 2.0) * fy + 0.5) * fy,
                          (0.5 * fy - 0.5) * fy * fy};
    bool ok = true;
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!two_y && j != 1) continue;
        const long rb = at + (long)(j - 1) * pitch;
        double rs;
        if (two_x) {
            const double v0 = ortho_tap<DT>(img, rb - 1), v1 = ortho_tap<DT>(img, rb), v2 = ortho_tap<DT>(img, rb + 1),
                         v3 = ortho_tap<DT>(img, rb + 2);
            ok = ok && !(v0 == nd || v1 == nd || v2 == nd || v3 == nd);
            rs = wx[0] * v0 + wx[1] * v1 + wx[2] * v2 + wx[3] * v3;
        } else {
            rs = ortho_tap<DT>(img, rb);
            ok = ok && !(rs == nd);
        }
        sum = two_y ? sum + wy[j] * rs : rs;
    }
    val = sum;
    return ok;
}

template <int RS>
__global__ __launch_bounds__(256) void ortho_rpc_kernel(const float* __restrict__ dsm, int rows, int cols, double gx0, double dx,
                                                        double gy0, double dy, int crs, double lon0_deg, double false_northing,
                                                        double dsm_nodata, double height_offset,
                                                        const rd_ortho_view* __restrict__ views, int n_views, float fill,
                                                        float* __restrict__ out, uint8_t* __restrict__ valid,
                                                        double* __restrict__ coords, int tiles_x) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int tyi = blockIdx.x / tiles_x, txi = blockIdx.x - tyi * tiles_x;
    const long c = (long)txi * ORTHO_TW + (w % ORTHO_WX) * ORTHO_FW + lane % ORTHO_FW;
    const long r = (long)tyi * ORTHO_TH + (w / ORTHO_WX) * ORTHO_FH + lane / ORTHO_FW;
    if (r >= rows || c >= cols) return;
    const long plane = (long)rows * cols, i = r * cols + c;
    const double nanv = __longlong_as_double(0x7ff8000000000000ll);
    const double z = (double)ld_nt1(dsm + i);
    const bool zok = !(isnan(z) || z == dsm_nodata);
    double lon = gx0 + ((double)c + 0.5) * dx, lat = gy0 + ((double)r + 0.5) * dy;
    if (crs == RD_ORTHO_UTM) ortho_utm_inverse(lon, lat, lon0_deg, false_northing, lon, lat);
    const double h = z + height_offset;
    for (int v = 0; v < n_views; ++v) {                                         // n_views is an argument: the same for every thread
        const rd_ortho_view& V = views[v];
        const double P = (lat - V.lat_off) / V.lat_scale, L = (lon - V.lon_off) / V.lon_scale, H = (h - V.height_off) / V.height_scale;
        const double LL = L * L, PP = P * P, HH = H * H;
        const double m[20] = {1.0, L, P, H, L * P, L * H, P * H, LL, PP, HH, P * L * H, LL * L, L * PP, L * HH, LL * P, PP * P,
                              P * HH, LL * H, PP * H, HH * H};
        const double line = ortho_poly(V.line_num, m) / ortho_poly(V.line_den, m) * V.line_scale + V.line_off;
        const double samp = ortho_poly(V.samp_num, m) / ortho_poly(V.samp_den, m) * V.samp_scale + V.samp_off;
        const double yi = line - V.line0, xi = samp - V.samp0;
        const void* img = V.image;
        const long pitch = V.pitch;
        const int ir = V.rows, ic = V.cols, dt = V.dtype;
        const double nd = V.image_nodata;
        bool ok = zok && img && ir >= 1 && ic >= 1;
        double val = 0.0;
        if (ok) {
            if (dt == RD_ORTHO_U8) ok = ortho_resample<RS, RD_ORTHO_U8>(img, pitch, ir, ic, nd, yi, xi, val);
            else if (dt == RD_ORTHO_U16) ok = ortho_resample<RS, RD_ORTHO_U16>(img, pitch, ir, ic, nd, yi, xi, val);
            else if (dt == RD_ORTHO_F32) ok = ortho_resample<RS, RD_ORTHO_F32>(img, pitch, ir, ic, nd, yi, xi, val);
            else ok = false;
        }
        const long o = (long)v * plane + i;
        st_nt1(out + o, ok ? (float)val : fill);
        if (valid) st_nt_u8(valid + o, ok ? 1 : 0);
        if (coords) {
            st_nt_f64(coords + 2 * o, zok ? yi : nanv);
            st_nt_f64(coords + 2 * o + 1, zok ? xi : nanv);
        }
    }
}

}  // namespace rd

extern "C" {

int rd_ortho_rpc(const float* dsm, int rows, int cols, double x0, double dx, double y0, double dy, int crs, double lon0_deg,
                 double false_northing, double dsm_nodata, double height_offset, const rd_ortho_view* views, int n_views,
                 int resampling, float fill, float* out, uint8_t* valid, double* coords, rd_stream_t s_) {
    constexpr double LARGEST = 1.7976931348623157e308;
    RD_REQUIRE(dsm && views && out, "rd_ortho_rpc: null pointer (dsm, views or out)");
    RD_REQUIRE(rows >= 1 && cols >= 1, "rd_ortho_rpc: bad shape (rows=%d cols=%d)", rows, cols);
    RD_REQUIRE((long)rows * cols < (1l << 31), "rd_ortho_rpc: %d x %d pixels, fewer than 2^31 are taken", rows, cols);
    RD_REQUIRE(n_views >= 1 && n_views <= RD_ORTHO_MAX_VIEWS, "rd_ortho_rpc: n_views %d outside 1..%d", n_views, RD_ORTHO_MAX_VIEWS);
    RD_REQUIRE(dx != 0.0 && fabs(dx) <= LARGEST && dy != 0.0 && fabs(dy) <= LARGEST,
               "rd_ortho_rpc: pixel size (%g, %g) must be non-zero and finite", dx, dy);
    RD_REQUIRE(crs == RD_ORTHO_GEOGRAPHIC || crs == RD_ORTHO_UTM, "rd_ortho_rpc: unknown crs %d", crs);
    RD_REQUIRE(resampling == RD_ORTHO_NEAREST || resampling == RD_ORTHO_BILINEAR || resampling == RD_ORTHO_BICUBIC,
               "rd_ortho_rpc: unknown resampling %d", resampling);
    RD_REQUIRE(fabs(lon0_deg) <= LARGEST && fabs(height_offset) <= LARGEST,
               "rd_ortho_rpc: lon0_deg %g and height_offset %g must be finite", lon0_deg, height_offset);
    hipStream_t s = (hipStream_t)s_;
    const long tiles_x = ((long)cols + ORTHO_TW - 1) / ORTHO_TW, tiles_y = ((long)rows + ORTHO_TH - 1) / ORTHO_TH;
    const double n = (double)rows * cols;
    // the model of the header's cost: ~250 fp64 operations for the ground point, ~130 per view; the DSM once, out (+ valid, coords)
    ProfScope ps(s, "ortho_rpc", n * (250.0 + 130.0 * n_views), n * (4.0 + n_views * (4.0 + (valid ? 1.0 : 0.0) + (coords ? 16.0 : 0.0))));
    const dim3 grid((unsigned)(tiles_x * tiles_y)), block(256);                 // at most rows * cols < 2^31 tiles
    if (resampling == RD_ORTHO_NEAREST)
        RD_LAUNCH(ortho_rpc_kernel<RD_ORTHO_NEAREST>, grid, block, 0, s, dsm, rows, cols, x0, dx, y0, dy, crs, lon0_deg,
                  false_northing, dsm_nodata, height_offset, views, n_views, fill, out, valid, coords, (int)tiles_x);
    else if (resampling == RD_ORTHO_BILINEAR)
        RD_LAUNCH(ortho_rpc_kernel<RD_ORTHO_BILINEAR>, grid, block, 0, s, dsm, rows, cols, x0, dx, y0, dy, crs, lon0_deg,
                  false_northing, dsm_nodata, height_offset, views, n_views, fill, out, valid, coords, (int)tiles_x);
    else
        RD_LAUNCH(ortho_rpc_kernel<RD_ORTHO_BICUBIC>, grid, block, 0, s, dsm, rows, cols, x0, dx, y0, dy, crs, lon0_deg,
                  false_northing, dsm_nodata, height_offset, views, n_views, fill, out, valid, coords, (int)tiles_x);
    RD_LAUNCH_CHECK("ortho_rpc");
    return RD_OK;
}

}  // extern "C"
