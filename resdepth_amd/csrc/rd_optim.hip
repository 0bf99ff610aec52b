// The global norm of the flat gradient (include/resdepth_hip_optim.h): one streaming pass over the finished
// buffer -- fp64 sums in a fixed order (thread -> block tree -> one block over the per-block pairs), no floating-point atomics --
// that also counts the elements that are not finite.  The statistics stay on the device.
#include "rd_common.h"

using namespace rd;

namespace {

constexpr int NT = RD_GNORM_BLOCK, VEC = RD_GNORM_VEC;
static_assert(VEC == 4 && NT == 256, "a chunk is one float4, the trees below halve from 128");

__device__ __forceinline__ void add_finite(float x, double& sum, int& bad) {
    if ((__float_as_uint(x) & 0x7f800000u) == 0x7f800000u)
        bad += 1;
    else
        sum += (double)x * (double)x;
}

// fixed tree over the block's 256 {sum, count} pairs; the result is in red[0], cnt[0]
__device__ __forceinline__ void block_tree(double* red, long long* cnt, int t) {
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) {
        if (t < off) {
            red[t] += red[t + off];
            cnt[t] += cnt[t + off];
        }
        __syncthreads();
    }
}

template <bool ALIGNED>
__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const float* __restrict__ g, long n, long chunks,
                                                                double* __restrict__ partial) {
    __shared__ double red[NT];
    __shared__ long long cnt[NT];
    double sum = 0.0;
    int bad = 0;
    const long stride = (long)gridDim.x * NT;
    long c = (long)blockIdx.x * NT + threadIdx.x;
    if (ALIGNED) {
        // four of the thread's chunks per trip: the loads are in flight together, the additions keep the thread's order
        for (; (c + 3 * stride) * VEC + VEC <= n; c += 4 * stride) {
            const float4 q0 = ld_nt4(g + c * VEC), q1 = ld_nt4(g + (c + stride) * VEC), q2 = ld_nt4(g + (c + 2 * stride) * VEC),
                         q3 = ld_nt4(g + (c + 3 * stride) * VEC);
            const float x[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
#pragma unroll
            for (int i = 0; i < 16; ++i) add_finite(x[i], sum, bad);
        }
    }
    for (; c < chunks; c += stride) {
        const long e = c * VEC;
        if (ALIGNED && e + VEC <= n) {
            const float4 q = ld_nt4(g + e);
            add_finite(q.x, sum, bad);
            add_finite(q.y, sum, bad);
            add_finite(q.z, sum, bad);
            add_finite(q.w, sum, bad);
        } else {
            const long end = e + VEC < n ? e + VEC : n;
            for (long i = e; i < end; ++i) add_finite(ld_nt1(g + i), sum, bad);
        }
    }
    const int t = threadIdx.x;
    red[t] = sum;
    cnt[t] = bad;
    block_tree(red, cnt, t);
    if (t == 0) {
        partial[2 * (long)blockIdx.x] = red[0];
        partial[2 * (long)blockIdx.x + 1] = (double)cnt[0];
    }
}

__global__ __launch_bounds__(256) void grad_norm_reduce_kernel(const double* __restrict__ partial, double* __restrict__ stats,
                                                               int nb) {
    __shared__ double red[NT];
    __shared__ long long cnt[NT];
    const int t = threadIdx.x;
    double sum = 0.0;
    long long bad = 0;
    for (int b = t; b < nb; b += NT) {
        sum += partial[2 * b];
        bad += (long long)partial[2 * b + 1];
    }
    red[t] = sum;
    cnt[t] = bad;
    block_tree(red, cnt, t);
    if (t == 0) {
        stats[0] = red[0];
        stats[1] = (double)cnt[0];
    }
}

// chunks of numel elements and the grid of the partial kernel: functions of numel alone
long gn_chunks(long long numel) { return (long)((numel + VEC - 1) / VEC); }
int gn_grid(long long numel) { return grid_cap((gn_chunks(numel) + NT - 1) / NT, RD_GNORM_MAX_BLOCKS); }

}  // namespace

extern "C" {

size_t rd_grad_norm_ws_bytes(long long numel) {
    if (numel <= 0) return 0;
    return (size_t)gn_grid(numel) * 2 * sizeof(double);
}

int rd_grad_norm(const float* g, long long numel, double* stats, void* ws, size_t ws_bytes, rd_stream_t s) {
    RD_REQUIRE(g && stats && numel > 0, "rd_grad_norm: bad arguments");
    const int nb = gn_grid(numel);
    if (!ws || ws_bytes < (size_t)nb * 2 * sizeof(double)) {
        set_error("rd_grad_norm: workspace too small");
        return RD_ERR_WS;
    }
    RD_REQUIRE(((uintptr_t)ws & 7) == 0 && ((uintptr_t)stats & 7) == 0, "rd_grad_norm: stats and ws must be 8-byte aligned");
    ProfScope ps((hipStream_t)s, "grad_norm", 0, 4.0 * numel);
    if (((uintptr_t)g & 15) == 0)
        RD_LAUNCH(grad_norm_partial_kernel<true>, dim3(nb), dim3(NT), 0, (hipStream_t)s, g, (long)numel, gn_chunks(numel),
                  (double*)ws);
    else
        RD_LAUNCH(grad_norm_partial_kernel<false>, dim3(nb), dim3(NT), 0, (hipStream_t)s, g, (long)numel, gn_chunks(numel),
                  (double*)ws);
    RD_LAUNCH(grad_norm_reduce_kernel, dim3(1), dim3(NT), 0, (hipStream_t)s, (const double*)ws, stats, nb);
    RD_LAUNCH_CHECK("grad_norm");
    return RD_OK;
}

}  // extern "C"
