// scan.hip -- inclusive prefix sum over u32, the primitive the reference borrows from lcpp
// (DeviceScan<>::InclusiveSum, call site lcgs/src/gs_tile_splatter/impl.cpp:104; lcpp itself is not
// part of the reference tree).  u32 wrap-around arithmetic, like the reference's Buffer<uint>; the same three kernels with
// u64 sums over the u32 input serve the MCMC sampler's weights (mcmc.hip), whose totals pass 2^32.
//
// Shape: reduce-then-scan in three launches (per-block sums -> scan of block sums -> per-block scan
// with carry-in).  HBM-bound: 8 B read + 4 B written per element; wave64 shuffles for the in-block
// scan, one 16-byte load per lane.  The element count may live in device memory (d_n) so that a
// whole frame can be enqueued without a host round trip; blocks past the live range exit at once.
#include "launch.hpp"
#include "wave_scan.hpp"

namespace lcgs
{
namespace
{

constexpr int kScanThreads = 256;
constexpr int kScanItems   = 4;                          // one uint4 per lane
constexpr int kScanTile    = kScanThreads * kScanItems;  // 1024 elements per block

// inclusive scan of one value per thread across a 256-thread block; returns the block total in `total`
template <typename T>
__device__ __forceinline__ T block_inclusive_scan(T v, T* s_wave /*[4]*/, T& total)
{
    const T inc   = wave_inclusive_scan(v);
    const T carry = block_carry<kScanThreads / 64>(inc, s_wave, total);
    __syncthreads();
    return inc + carry;
}

__device__ __forceinline__ void load_tile(const uint32_t* __restrict__ in, int64_t base, int64_t n, uint32_t v[4])
{
    int64_t i = base + (int64_t)threadIdx.x * kScanItems;
    if (i + 3 < n && ((reinterpret_cast<uintptr_t>(in + i) & 15) == 0)) {
        uint4 q = *reinterpret_cast<const uint4*>(in + i);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (i + k < n) ? in[i + k] : 0u;
    }
}

// T: the type of the sums (uint32_t, or uint64_t over the same u32 input)
template <typename T>
__global__ void __launch_bounds__(kScanThreads) k_scan_reduce(const uint32_t* __restrict__ in, int64_t n_host,
                                                                const uint32_t* __restrict__ d_n,
                                                                T* __restrict__ block_sums)
{
    __shared__ T  s_wave[4];
    const int64_t n    = d_n ? (int64_t)*d_n : n_host;
    const int64_t base = (int64_t)blockIdx.x * kScanTile;
    if (base >= n) return;
    uint32_t v[4];
    load_tile(in, base, n, v);
    T sum = (T)v[0] + v[1] + v[2] + v[3];
    T total;
    block_inclusive_scan(sum, s_wave, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// exclusive scan of the block sums, in place, by one block (nb <= a few thousand)
template <typename T>
__global__ void __launch_bounds__(1024) k_scan_block_sums(T* __restrict__ block_sums, int64_t n_host,
                                                           const uint32_t* __restrict__ d_n)
{
    __shared__ T  s_wave[16];
    __shared__ T  s_carry;
    const int64_t n  = d_n ? (int64_t)*d_n : n_host;
    const int64_t nb = (n + kScanTile - 1) / kScanTile;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < nb; base += 1024) {
        int64_t i     = base + threadIdx.x;
        T       v     = i < nb ? block_sums[i] : (T)0;
        T       inc   = wave_inclusive_scan(v);
        T       carry = block_carry<16>(inc, s_wave);
        carry += s_carry;
        if (i < nb) block_sums[i] = carry + inc - v; // exclusive
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = carry + inc;
        __syncthreads();
    }
}

template <typename T>
__global__ void __launch_bounds__(kScanThreads) k_scan_final(const uint32_t* __restrict__ in, T* __restrict__ out,
                                                               int64_t n_host, const uint32_t* __restrict__ d_n,
                                                               const T* __restrict__ block_sums)
{
    __shared__ T  s_wave[4];
    const int64_t n    = d_n ? (int64_t)*d_n : n_host;
    const int64_t base = (int64_t)blockIdx.x * kScanTile;
    if (base >= n) return;
    uint32_t v[4];
    load_tile(in, base, n, v);
    T s[4] = { v[0], v[1], v[2], v[3] };
    s[1] += s[0];
    s[2] += s[1];
    s[3] += s[2];
    T       total;
    T       inc   = block_inclusive_scan(s[3], s_wave, total);
    T       carry = block_sums[blockIdx.x] + (inc - s[3]);
    int64_t i     = base + (int64_t)threadIdx.x * kScanItems;
    if (i + 3 < n && ((reinterpret_cast<uintptr_t>(out + i) & 15) == 0)) {
        if constexpr (sizeof(T) == 4) {
            *reinterpret_cast<uint4*>(out + i) = make_uint4(s[0] + carry, s[1] + carry, s[2] + carry, s[3] + carry);
        } else {
            *reinterpret_cast<ulonglong2*>(out + i)     = make_ulonglong2(s[0] + carry, s[1] + carry);
            *reinterpret_cast<ulonglong2*>(out + i + 2) = make_ulonglong2(s[2] + carry, s[3] + carry);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i + k < n) out[i + k] = s[k] + carry;
    }
}

template <typename T>
void launch_inclusive_sum(const uint32_t* in, T* out, int64_t n_cap, const uint32_t* d_n, void* temp, hipStream_t stream)
{
    if (n_cap <= 0) return;
    T*      block_sums = reinterpret_cast<T*>(temp);
    int64_t nb         = (n_cap + kScanTile - 1) / kScanTile;
    hipLaunchKernelGGL(k_scan_reduce<T>, dim3((unsigned)nb), dim3(kScanThreads), 0, stream, in, n_cap, d_n, block_sums);
    hipLaunchKernelGGL(k_scan_block_sums<T>, dim3(1), dim3(1024), 0, stream, block_sums, n_cap, d_n);
    hipLaunchKernelGGL(k_scan_final<T>, dim3((unsigned)nb), dim3(kScanThreads), 0, stream, in, out, n_cap, d_n,
                       (const T*)block_sums);
}

} // namespace

size_t scan_temp_bytes(int64_t n)
{
    int64_t nb = (n + kScanTile - 1) / kScanTile;
    return (size_t)(nb + 1) * sizeof(uint64_t); // sized for the u64 sums: one buffer serves both scans
}

void launch_inclusive_sum_u32_dyn(const uint32_t* in, uint32_t* out, int64_t n_cap, const uint32_t* d_n, void* temp,
                                  hipStream_t stream)
{
    launch_inclusive_sum<uint32_t>(in, out, n_cap, d_n, temp, stream);
}

void launch_inclusive_sum_u32(const uint32_t* in, uint32_t* out, int64_t n, void* temp, hipStream_t stream)
{
    launch_inclusive_sum<uint32_t>(in, out, n, nullptr, temp, stream);
}

void launch_inclusive_sum_u64(const uint32_t* in, uint64_t* out, int64_t n, void* temp, hipStream_t stream)
{
    launch_inclusive_sum<uint64_t>(in, out, n, nullptr, temp, stream);
}

} // namespace lcgs
