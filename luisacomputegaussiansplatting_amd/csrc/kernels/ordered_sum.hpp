// ordered_sum.hpp -- the fixed-order binary64 sums the loss kernels share (loss.hip, depth_prior.hip, bilagrid.hip): a wave's butterfly and the
// one-workgroup finish over per-workgroup partials.  No atomics: the same inputs give the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lcgs
{
constexpr int kOrderedSumThreads = 256; // the workgroup size sum_partials_in_order is launched with

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// ---- finish: the workgroups' partials (N per workgroup) in index order -- each thread a contiguous run, then thread 0 the
// 256 run sums in order.  Returns true on thread 0, whose `out` holds the N sums.
template <int N>
__device__ __forceinline__ bool sum_partials_in_order(int64_t num, const double* __restrict__ partials, double (&out)[N])
{
    constexpr int     kThreads = kOrderedSumThreads;
    __shared__ double s_sum[N][kThreads];
    const int64_t     run = (num + kThreads - 1) / kThreads;
    const int64_t     lo = (int64_t)threadIdx.x * run, hi = lo + run < num ? lo + run : num;
#pragma unroll
    for (int k = 0; k < N; ++k) out[k] = 0.0;
    for (int64_t i = lo; i < hi; ++i) {
#pragma unroll
        for (int k = 0; k < N; ++k) out[k] += partials[N * i + k];
    }
#pragma unroll
    for (int k = 0; k < N; ++k) s_sum[k][threadIdx.x] = out[k];
    __syncthreads();
    if (threadIdx.x != 0) return false;
#pragma unroll
    for (int k = 0; k < N; ++k) out[k] = 0.0;
    for (int t = 0; t < kThreads; ++t) {
#pragma unroll
        for (int k = 0; k < N; ++k) out[k] += s_sum[k][t];
    }
    return true;
}
} // namespace lcgs
