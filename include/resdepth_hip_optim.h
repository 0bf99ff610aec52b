/*
 * resdepth_hip_optim.h -- statistics of the flat gradient for the optimizer path: entry points of libresdepth_hip.so
 * (rd_version >= 115), included by resdepth_hip.h; its conventions (device pointers, stream, return codes, memory contract,
 * alignment) hold here.
 *
 * Kept apart from resdepth_hip.h for the reason resdepth_hip_loss.h is: the coverage ledger over the main header
 * (tests/test_memory_contract_gpu.py) describes exactly the entry points its case table drives.  The guard-band cases of the
 * entry points below, and a ledger over THIS header, are in tests/test_optim_contract_gpu.py.
 *
 * The reference has none of this.  rd_grad_norm gives what torch.nn.utils.clip_grad_norm_ (norm_type 2) and a guard against
 * NaN / Inf gradients need of the finished flat gradient -- the sum of squares and the number of non-finite elements -- as two
 * doubles in device memory: nothing is read back, so it can sit between backward and step of a captured iteration.  One read
 * of the gradient (4 bytes per element), two launches.
 *
 * Arithmetic of rd_grad_norm over the RAW gradient g[0 .. numel):
 *     finite(x) = the exponent bits of x are not all ones
 *     stats[0] = sum over finite g[e] of (double)g[e]^2      (a squared fp32 is exact in fp64; the additions are fp64)
 *     stats[1] = number of non-finite g[e], counted in integers, stored as an exact fp64 integer
 * Schedule.  Element e belongs to chunk c = e / RD_GNORM_VEC (a chunk is RD_GNORM_VEC consecutive INDICES, wherever g lies in
 * memory).  The grid has G = min(ceil(chunks / RD_GNORM_BLOCK), RD_GNORM_MAX_BLOCKS) blocks of RD_GNORM_BLOCK threads; thread
 * j = block * RD_GNORM_BLOCK + thread takes chunks j, j + G * RD_GNORM_BLOCK, ... in that order and adds the elements of a chunk
 * in index order into ONE fp64 accumulator (and one integer counter).  A block adds its threads' accumulators by a fixed tree
 * (stride 128, 64, ... 1) and writes {sum, count} to the scratch; one block of 256 threads adds the per-block pairs (thread t
 * takes blocks t, t + 256, ... in order, then the same tree).  The mapping element -> (block, thread, position) is a function
 * of e and numel alone: no floating-point atomics, the same bits run to run.
 * Alignment rule: a 16-byte aligned g is read one chunk per access (float4), any other g one element per access; both forms
 * give the same bits.  The reads are non-temporal: the gradient is read again by the optimizer step that follows.
 *
 * The norm is sqrt(stats[0]) (times |grad_scale| for a scaled gradient); stats[1] > 0 says that torch's norm would be NaN or Inf.
 */
#ifndef RESDEPTH_HIP_OPTIM_H
#define RESDEPTH_HIP_OPTIM_H

#ifdef __cplusplus
extern "C" {
#endif

/* threads of a block, indices of a chunk and the cap of the grid of rd_grad_norm's first launch */
#define RD_GNORM_BLOCK 256
#define RD_GNORM_VEC 4
#define RD_GNORM_MAX_BLOCKS 1024

/* bytes of scratch rd_grad_norm needs for numel elements (one {sum, count} pair of fp64 per block); 0 when numel <= 0 */
size_t rd_grad_norm_ws_bytes(long long numel);

/* stats[0..1] (fp64, device) of g[0 .. numel) as above.  Two launches: grad_norm_partial_kernel<vector?> and
 * grad_norm_reduce_kernel.  A scratch smaller than rd_grad_norm_ws_bytes(numel) is refused (RD_ERR_WS) with nothing launched. */
int rd_grad_norm(const float* g, long long numel, double* stats, void* ws, size_t ws_bytes, rd_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* RESDEPTH_HIP_OPTIM_H */
