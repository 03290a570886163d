// kept_walk.hpp -- what the kernels that walk a keep-state frame's KEPT per-tile lists once more share (maps.hip: depth and alpha
// maps and their backward; contrib.hip: per-splat blend-weight statistics): the workgroup -> tile map in the renderer's schedule,
// the tile's walk length, the staging of one list entry with the renderer's own bits, and the butterfly sum over a 16-lane row.
#pragma once

#include "launch.hpp"
#include "tile_common.hpp"

namespace lcgs
{
namespace kept_walk
{
using namespace tile;

// the value a splat contributes to the depth map
__device__ __forceinline__ float depth_value(float z, int mode) { return mode == kDepthInvZ ? 1.0f / z : z; }

// butterfly sum over each 16-lane row (every lane of the row ends with the row's total): xor 1, xor 2 inside the quads,
// then the half-row and the row mirrors
__device__ __forceinline__ float row16_sum(float x)
{
#define LCGS_DPP_ADD(CTRL) x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, true))
    LCGS_DPP_ADD(0xB1);  // quad_perm:[1,0,3,2]
    LCGS_DPP_ADD(0x4E);  // quad_perm:[2,3,0,1]
    LCGS_DPP_ADD(0x141); // row_half_mirror
    LCGS_DPP_ADD(0x140); // row_mirror
#undef LCGS_DPP_ADD
    return x;
}

// workgroup -> tile (the renderer's schedule); false: a padding slot of the XCD-aware map
__device__ __forceinline__ bool tile_of_slot(const CamParams& cp, const uint32_t* tile_order, uint32_t slot, uint32_t& tx, uint32_t& ty)
{
    if (tile_order) {
        if (slot >= cp.grid_x * cp.grid_y) return false;
        const uint32_t t = tile_order[slot];
        tx = t % cp.grid_x;
        ty = t / cp.grid_x;
        return true;
    }
    return tile_of_workgroup(slot, cp.grid_x, cp.grid_y, tx, ty);
}

// the tile's walk length: its largest n_contrib, never past its own list (uniform over the workgroup)
__device__ __forceinline__ uint32_t tile_walk_length(uint32_t last, uint32_t len, uint32_t* s_max, uint32_t lane, uint32_t wave)
{
    uint32_t wmax = last;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = __shfl_xor(wmax, off, 64);
        wmax             = o > wmax ? o : wmax;
    }
    if (lane == 0) s_max[wave] = wmax;
    __syncthreads();
    uint32_t hi = s_max[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) hi = s_max[w] > hi ? s_max[w] : hi;
    hi = hi < len ? hi : len;
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)hi);
}

// one staged entry: [0] mean.x, mean.y, -conic.x / 2, -conic.z / 2   [1] conic.y, power floor, opacity, value
// (the halved, negated diagonal and the floor are the renderer's own staging: same bits in `power`)
struct StagedEntry {
    float4 a, b;
};
__device__ __forceinline__ StagedEntry stage_entry(const SplatRecord* __restrict__ recs, uint32_t vid, int mode)
{
    const float4* p  = reinterpret_cast<const float4*>(recs + vid);
    const float4  r0 = p[0], r1 = p[1]; // mx, my, ca, cb | cc, opacity, r, g
    const float   z  = recs[vid].depth;
    const float   t  = (2.0f * __logf(255.0f * r1.y)) * 1.0001f + 2e-4f;
    StagedEntry   e;
    e.a = make_float4(r0.x, r0.y, -0.5f * r0.z, -0.5f * r1.x);
    e.b = make_float4(r0.w, fmax_(-0.5f * t, kBlendExpMin), r1.y, depth_value(z, mode));
    return e;
}

inline uint32_t maps_grid(const CamParams& cp, const uint32_t* tile_order)
{
    return tile_order ? cp.grid_x * cp.grid_y : render_grid_size(cp.grid_x, cp.grid_y);
}
} // namespace kept_walk
} // namespace lcgs
