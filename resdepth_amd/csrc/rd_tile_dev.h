// Device-side helpers shared by the tile data path's translation units (rd_tiles.hip, rd_trainset.hip): the one copy of the
// D4 maps, the four-pixel load / normalise / mask blocks, the 256-leaf fp64 tree and a grid tile's means.  Samples assembled
// by different entry points have the same bits because they go through these, not through copies of them.
#pragma once
#include "rd_common.h"

namespace rd {

// ---- the square's symmetry group on a T x T tile ---------------------------------------------------------------------------
// Code a = k | flip_v << 2 | flip_h << 3 = rot90(k) -> flipud -> fliplr (lib/torch_transforms.py); higher bits are ignored.
// aug_src: the plain-tile pixel (sr, sc) that the oriented tile shows at (r, c); aug_dst is its inverse.  Both map an
// axis-aligned rectangle onto an axis-aligned rectangle (sides swapped for odd k), which is what the LDS staging of
// blend_tta_kernel and grid_tile_write_aug relies on.
__device__ __forceinline__ void aug_src(int a, int T, int r, int c, int& sr, int& sc) {
    const int k = a & 3, c1 = (a & 8) ? T - 1 - c : c, r1 = (a & 4) ? T - 1 - r : r;
    if (k == 0) { sr = r1; sc = c1; }
    else if (k == 1) { sr = c1; sc = T - 1 - r1; }
    else if (k == 2) { sr = T - 1 - r1; sc = T - 1 - c1; }
    else { sr = T - 1 - c1; sc = r1; }
}
__device__ __forceinline__ void aug_dst(int a, int T, int sr, int sc, int& r, int& c) {
    const int k = a & 3;
    int r1, c1;
    if (k == 0) { r1 = sr; c1 = sc; }
    else if (k == 1) { c1 = sr; r1 = T - 1 - sc; }
    else if (k == 2) { r1 = T - 1 - sr; c1 = T - 1 - sc; }
    else { c1 = T - 1 - sr; r1 = sc; }
    r = (a & 4) ? T - 1 - r1 : r1;
    c = (a & 8) ? T - 1 - c1 : c1;
}

// ---- four adjacent pixels of a row -----------------------------------------------------------------------------------------
// one 16-byte load when the caller knows p to be 16-byte aligned, else four 4-byte loads
__device__ __forceinline__ float4 ld4(const float* __restrict__ p, bool vec) {
    if (vec) return *reinterpret_cast<const float4*>(p);
    return make_float4(p[0], p[1], p[2], p[3]);
}

// (v - mean) / sdv, each operation rounded on its own (torch's sub then div)
__device__ __forceinline__ float4 norm4(float4 v, float mean, float sdv) {
    float4 o;
    o.x = __fdiv_rn(__fsub_rn(v.x, mean), sdv);
    o.y = __fdiv_rn(__fsub_rn(v.y, mean), sdv);
    o.z = __fdiv_rn(__fsub_rn(v.z, mean), sdv);
    o.w = __fdiv_rn(__fsub_rn(v.w, mean), sdv);
    return o;
}

// the loss mask of the ground-truth pixels v at columns c .. c + 3: inside the box (in_rows: the row is, columns x0 .. x1
// inclusive), gt != 0 and gt != nodata (lib/DsmOrthoDataset.py:434-470)
__device__ __forceinline__ uchar4 mask4(float4 v, bool in_rows, int c, int x0, int x1, float nodata) {
    uchar4 m;
    m.x = in_rows && c >= x0 && c <= x1 && v.x != 0.f && v.x != nodata;
    m.y = in_rows && c + 1 >= x0 && c + 1 <= x1 && v.y != 0.f && v.y != nodata;
    m.z = in_rows && c + 2 >= x0 && c + 2 <= x1 && v.z != 0.f && v.z != nodata;
    m.w = in_rows && c + 3 >= x0 && c + 3 <= x1 && v.w != 0.f && v.w != nodata;
    return m;
}

// ---- the 256-leaf fp64 tree ------------------------------------------------------------------------------------------------
// K sums over the 256 threads of the block: leaf t is thread t's v[k], then off = 128, 64, .. 1.  red holds K * 256 doubles;
// afterwards red[k * 256] is sum k, visible to every thread.  The order is part of the results' bits: rd_patch_sums and
// rd_assemble_train_patches promise the same means because both come through here.  (rd_trainset.hip's block_sum_256 is a
// different order and a different function.)
template <int K>
__device__ __forceinline__ void tree_sum_256(const double (&v)[K], double* red) {
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) red[k * 256 + t] = v[k];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) {
#pragma unroll
            for (int k = 0; k < K; ++k) red[k * 256 + t] += red[k * 256 + t + off];
        }
        __syncthreads();
    }
}

// ---- a grid tile's means ---------------------------------------------------------------------------------------------------
// from grid_tile_sums' slab partials (ws: four doubles per (tile, slab): DSM sum, DSM count, ortho sum), added in slab order,
// then one rounding to fp32 (GpuPatchSampler's (sum / count).float()) -- so a tile's mean depends on the tile's pixels and T
// alone.  Mode 1 takes the fixed value, mode 0 leaves 0; the ortho mean is computed for blocks that write an ortho plane only.
__device__ __forceinline__ void grid_tile_means(const double* __restrict__ ws, int i, int S, int V, int T, int dsm_mode,
                                                float dsm_mean_fixed, int ortho_mode, float ortho_mean_fixed, bool ortho_plane,
                                                float& dmean, float& omean) {
    dmean = dsm_mode == 1 ? dsm_mean_fixed : 0.f;
    omean = ortho_mode == 1 ? ortho_mean_fixed : 0.f;
    if (dsm_mode == 2) {
        double s = 0.0, c = 0.0;
        for (int k = 0; k < S; ++k) {
            s += ws[((long)i * S + k) * 4];
            c += ws[((long)i * S + k) * 4 + 1];
        }
        dmean = (float)(s / c);
    }
    if (ortho_mode == 2 && V > 0 && ortho_plane) {
        double s = 0.0;
        for (int k = 0; k < S; ++k) s += ws[((long)i * S + k) * 4 + 2];
        omean = (float)(s / ((double)V * T * T));
    }
}

// rows of a tile per block of the four-pixels-per-lane write kernels (grid_tile_write, train_patch_write): about 4096 pixels
inline int tile_rows_per_block(int tile) { return 4096 / tile < 1 ? 1 : (4096 / tile > tile ? tile : 4096 / tile); }

}  // namespace rd
