// wave_scan.hpp -- the two steps behind every kernel that ranks, compacts or offsets: an inclusive scan across the 64 lanes
// of a wave, and the carry across the waves of a workgroup through one small LDS array.  T is uint32_t or uint64_t
// (wrap-around sums); threadIdx.x is the linear thread index; wave64 only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lcgs
{

// lane l ends with the sum of lanes 0 .. l; lane 63 holds the wave's total
template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}

// exclusive form of the same, with the wave's total in every lane
template <typename T>
__device__ __forceinline__ T wave_excl_scan(T v, T& total)
{
    const T inc = wave_inclusive_scan(v);
    total       = __shfl(inc, 63, 64);
    return inc - v;
}

// `inc` is the caller's wave_inclusive_scan in a workgroup of WAVES waves, every thread calling: returns the sum of the waves
// in front of the caller's, and the sum of all waves in `total`.  One barrier, behind the store to s_wave[WAVES]; adding a
// carry-in, turning inclusive into exclusive, and the barrier before s_wave is written again are the caller's.
template <int WAVES, typename T>
__device__ __forceinline__ T block_carry(T inc, T* s_wave, T& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    T carry = 0;
    total   = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        if (w < wave) carry += s_wave[w];
        total += s_wave[w];
    }
    return carry;
}
template <int WAVES, typename T>
__device__ __forceinline__ T block_carry(T inc, T* s_wave)
{
    T total;
    return block_carry<WAVES>(inc, s_wave, total);
}

} // namespace lcgs
