// densify_row.hpp -- what the two statistics passes of adaptive density control (densify.hip k_densify_stats, absgrad.hip
// k_absgrad_rows) do to an on-screen row besides its gradient term: the visit count and the largest reference radius.  ONE
// statement of the radius, so that a caller may mix lcgs_densify_accumulate and lcgs_absgrad_accumulate over the steps of a run
// and find the same denom and max_radii bit for bit.
#pragma once

#include "kept_rows.hpp"

namespace lcgs
{
// scene row i of an on-screen row: denom += 1, max_radii = max(., the reference radius (gs_tile_splatter/shader.cpp:145-148) as
// the frame's cull pass evaluates it)
__device__ __forceinline__ void densify_count_row(const CamParams& cp, float scale_modifier, const float* __restrict__ pos,
                                                  const float* __restrict__ scale, const float* __restrict__ rotq, int64_t i,
                                                  uint32_t* __restrict__ denom, int32_t* __restrict__ max_radii)
{
    float v[3], t[3], Sig[3][3], cov2d[3], conic[3];
    view_transform(cp, pos[3 * i + 0], pos[3 * i + 1], pos[3 * i + 2], v);
    const float  s[3] = { scale_modifier * scale[3 * i + 0], scale_modifier * scale[3 * i + 1], scale_modifier * scale[3 * i + 2] };
    const float4 q    = *reinterpret_cast<const float4*>(rotq + 4 * i);
    cov3d_from_scale_rot(s, q.y, q.z, q.w, q.x, Sig);
    cam_clamp(cp, v, t);
    ewa_cov2d(cp, Sig, t, true, cov2d);
    int32_t radius = 0;
    conic_and_radius(cov2d[0], cov2d[1], cov2d[2], true, cp.width, cp.height, conic, radius);
    denom[i] += 1u;
    max_radii[i] = max(max_radii[i], radius);
}
} // namespace lcgs
