// adam_rows.hpp -- the optimiser's arithmetic as ONE set of device expressions: the Adam update and, per attribute kind, the
// chain rule from the gradient w.r.t. the activated value to the raw parameter, the update and the activation (train.hip's
// header has the table).  train.hip's kernels and the fused preprocess-backward + Adam kernel of backward.hip call these
// with values in registers and keep their own loads and stores; the build does not contract (-ffp-contract=off), so one
// source expression gives the same bits in every caller.
#pragma once

#include "activations.hpp"
#include "launch.hpp"

namespace lcgs
{

__device__ __forceinline__ float adam_update(float g, float& m, float& v, float lr, const AdamStep& a)
{
    m = a.b1 * m + (1.0f - a.b1) * g;
    v = a.b2 * v + (1.0f - a.b2) * g * g;
    return (lr * a.inv_bc1) * m / (sqrtf(v) * a.inv_sqrt_bc2 + a.eps);
}

// Every function: g = gradient w.r.t. the activated value; x (raw), m, v and -- where there is one -- the activated value
// are updated in place.
// pos, sh: raw == activated
__device__ __forceinline__ void adam_plain(float g, float& x, float& m, float& v, float lr, const AdamStep& a)
{
    x = x - adam_update(g, m, v, lr, a);
}
// scale s = exp(raw): g_raw = g * s
__device__ __forceinline__ void adam_scale(float g, float& x, float& m, float& v, float& s, float lr, const AdamStep& a)
{
    x = x - adam_update(g * s, m, v, lr, a);
    s = act_exp(x);
}
// opacity o = sigmoid(raw): g_raw = g o (1 - o)
__device__ __forceinline__ void adam_opacity(float g, float& x, float& m, float& v, float& o, float lr, const AdamStep& a)
{
    x = x - adam_update(g * o * (1.0f - o), m, v, lr, a);
    o = act_sigmoid(x);
}
// rotq q = raw / |raw|: g_raw = (g - q (q . g)) / |raw|   (rows are (r,x,y,z))
__device__ __forceinline__ void adam_quat(const float4& g, float4& x, float4& m, float4& v, float4& q, float lr,
                                          const AdamStep& a)
{
    const float inv_norm = 1.0f / sqrtf(x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w);
    const float qg       = q.x * g.x + q.y * g.y + q.z * g.z + q.w * g.w;
    x.x -= adam_update((g.x - q.x * qg) * inv_norm, m.x, v.x, lr, a);
    x.y -= adam_update((g.y - q.y * qg) * inv_norm, m.y, v.y, lr, a);
    x.z -= adam_update((g.z - q.z * qg) * inv_norm, m.z, v.z, lr, a);
    x.w -= adam_update((g.w - q.w * qg) * inv_norm, m.w, v.w, lr, a);
    q = act_unit(x);
}
// float4 `part` (0..11) of a degree-3 SH row: floats 0..2 of the row are the dc band
__device__ __forceinline__ void adam_sh4(const float4& g, float4& x, float4& m, float4& v, uint32_t part, float lr_dc,
                                         float lr_rest, const AdamStep& a)
{
    const float l = part == 0u ? lr_dc : lr_rest;
    x.x -= adam_update(g.x, m.x, v.x, l, a);
    x.y -= adam_update(g.y, m.y, v.y, l, a);
    x.z -= adam_update(g.z, m.z, v.z, l, a);
    x.w -= adam_update(g.w, m.w, v.w, lr_rest, a);
}

} // namespace lcgs
