// philox.hpp -- Philox4x32-10 (Salmon et al., SC'11), the counter-based generator behind every built-in sampler of the density
// control (densify.hip: a split row's children; mcmc.hip: the relocation draws and the SGLD normals).  key = the caller's seed,
// counter = what the draw is OF (a row, a child, a draw index, a step): a draw depends on nothing else -- not the launch shape,
// not the row count.  Counter layouts in use (words 0..3), kept apart by word 2:
//   densify.hip  (row low, row high, child 0 | 1, 0)
//   mcmc.hip     (draw low, draw high, kMcmcTagRelocate | kMcmcTagAdd, 0) and (row low, row high, kMcmcTagNoise, step)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lcgs
{

__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t lo0 = 0xD2511F53u * c[0], hi0 = __umulhi(0xD2511F53u, c[0]);
        const uint32_t lo1 = 0xCD9E8D57u * c[2], hi1 = __umulhi(0xCD9E8D57u, c[2]);
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = lo1;
        c[2] = n2;
        c[3] = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}
__device__ __forceinline__ float unit_open(uint32_t x) { return ((float)(x >> 8) + 0.5f) * (1.0f / 16777216.0f); } // (0, 1)
// three standard normals of one Philox block (Box-Muller; the fourth is not formed)
__device__ __forceinline__ void box_muller3(const uint32_t c[4], float n[3])
{
    const float r0 = sqrtf(-2.0f * logf(unit_open(c[0]))), t0 = 6.28318530717958647692f * unit_open(c[1]);
    const float r1 = sqrtf(-2.0f * logf(unit_open(c[2]))), t1 = 6.28318530717958647692f * unit_open(c[3]);
    n[0] = r0 * cosf(t0);
    n[1] = r0 * sinf(t0);
    n[2] = r1 * cosf(t1);
}

} // namespace lcgs
