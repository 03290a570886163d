// densify.hip -- adaptive density control: the per-step statistics, the clone / split / prune rewrite of the
// raw parameters with their Adam moments, and the opacity reset.  No reference counterpart (doc/roadmap.md:4 only names
// training).  The rewrite is OUT OF PLACE and order preserving: every source row emits 0, 1 or 2 consecutive output rows at
// the exclusive prefix sum of the emit counts (scan.hip), so new rows sit next to their parents (a Morton-ordered scene
// keeps its locality), the result is deterministic and no atomic is needed.
//   action 0 prune   nothing
//          1 keep    raw / m / v copied bit for bit
//          2 clone   the row, then a second copy of raw with zero moments
//          3 split   two children: pos + R(q / |q|) (s * n_k), raw scale - ln 1.6, zero moments; rotation, SH, opacity copied
// HBM-bound once-through work like train.hip: one thread per source element (16 bytes where the layout allows), streaming
// loads of the source, destination offsets monotone in the source index (coalesced stores), the zero moments of new rows
// written here instead of by a memset over the whole array.  64-bit element indices throughout.
#include "activations.hpp" // train.hip's exact expression sequences (the values equal what an Adam step writes)
#include "densify_row.hpp"
#include "kept_rows.hpp"
#include "launch.hpp"
#include "philox.hpp"
#include "stream_access.hpp"

namespace lcgs
{
namespace
{

// ---- statistics of a step: one thread per on-screen row of the last frame (count on the device)
__global__ void __launch_bounds__(256) k_densify_stats(const uint32_t* __restrict__ vis_index, const uint32_t* __restrict__ d_counts,
                                                       int64_t P, CamParams cp, float scale_modifier,
                                                       const float* __restrict__ pos, const float* __restrict__ scale,
                                                       const float* __restrict__ rotq, const float* __restrict__ grads2d,
                                                       float* __restrict__ grad_accum, uint32_t* __restrict__ denom,
                                                       int32_t* __restrict__ max_radii)
{
    const int64_t V  = (int64_t)d_counts[0];
    const float   hw = 0.5f * (float)cp.width, hh = 0.5f * (float)cp.height;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < V; r += (int64_t)gridDim.x * 256) {
        const int64_t i = (int64_t)vis_index[r];
        if (i >= P) continue;
        const float gx = grads2d[r * 12 + 0] * hw, gy = grads2d[r * 12 + 1] * hh;
        grad_accum[i] += sqrtf(gx * gx + gy * gy);
        densify_count_row(cp, scale_modifier, pos, scale, rotq, i, denom, max_radii); // (shared with absgrad.hip)
    }
}

// ---- the rewrite, step 1: one thread per source row -> emit count and action
__global__ void __launch_bounds__(256) k_densify_classify(int64_t P, DensifyRule rule, const float* __restrict__ raw_scale,
                                                          const float* __restrict__ raw_opacity,
                                                          const float* __restrict__ grad_accum,
                                                          const uint32_t* __restrict__ denom,
                                                          const int32_t* __restrict__ max_radii, uint32_t* __restrict__ emit,
                                                          uint8_t* __restrict__ action)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < P; i += (int64_t)gridDim.x * 256) {
        const uint32_t n    = denom[i];
        const float    avg  = n ? grad_accum[i] / (float)n : 0.0f;
        const float    smax = fmaxf(fmaxf(act_exp(raw_scale[3 * i + 0]), act_exp(raw_scale[3 * i + 1])), act_exp(raw_scale[3 * i + 2]));
        const float    op   = act_sigmoid(raw_opacity[i]);
        const bool     hot  = avg >= rule.grad_threshold;
        const bool     big  = smax > rule.dense_extent;
        const bool     prune =
            op < rule.min_opacity || (rule.max_screen_size > 0 && (max_radii[i] > rule.max_screen_size || smax > rule.huge_extent));
        const uint32_t a = prune ? 0u : (!hot ? 1u : (big ? 3u : 2u));
        action[i]        = (uint8_t)a;
        emit[i]          = a >= 2u ? 2u : a;
    }
}

template <int MODE> // 0 identity, 1 exp, 2 sigmoid
__device__ __forceinline__ float activate(float x)
{
    return MODE == 1 ? act_exp(x) : (MODE == 2 ? act_sigmoid(x) : x);
}
template <int MODE> // 0 identity, 3 unit quaternion
__device__ __forceinline__ float4 activate(const float4& x)
{
    return MODE == 3 ? act_unit(x) : x;
}
__device__ __forceinline__ float  zero_of(const float*) { return 0.0f; }
__device__ __forceinline__ float4 zero_of(const float4*) { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
__device__ __forceinline__ float  lowered(float x, float d) { return x - d; }
__device__ __forceinline__ float4 lowered(const float4& x, float) { return x; }

// ---- step 2, by attribute family: rows of ROW elements of T (float, or float4 for quaternions and 48-float SH rows); one
// thread per SOURCE element.  incl: inclusive sums of the emit counts.  split_drop: subtracted from a split row's raw value
// (the scale family: ln 1.6).  src_row (the scalar family only): output row -> source row.
template <int ROW, int MODE, typename T>
__global__ void __launch_bounds__(256) k_densify_rows(int64_t P, const uint8_t* __restrict__ action, const uint32_t* __restrict__ incl,
                                                      const T* __restrict__ raw, const T* __restrict__ m, const T* __restrict__ v,
                                                      T* __restrict__ o_raw, T* __restrict__ o_m, T* __restrict__ o_v,
                                                      T* o_act /* may alias o_raw */, float split_drop, uint32_t* __restrict__ src_row)
{
    const int64_t total = P * ROW;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t  r = e / ROW;
        const int      c = (int)(e - r * ROW);
        const uint32_t a = action[r];
        if (a == 0u) continue;
        const int64_t row = (int64_t)incl[r] - (a >= 2u ? 2 : 1);
        const int64_t d   = row * ROW + c;
        T             x   = ld_stream(raw + e);
        if (MODE == 1 && a == 3u) x = lowered(x, split_drop);
        const T z  = zero_of(raw);
        const T mm = a == 3u ? z : ld_stream(m + e), vv = a == 3u ? z : ld_stream(v + e); // children start from zero moments
        const T y  = activate<MODE>(x);
        st_stream(o_raw + d, x);
        st_stream(o_m + d, mm);
        st_stream(o_v + d, vv);
        if (MODE != 0 || o_act != o_raw) st_stream(o_act + d, y);
        if (ROW == 1 && src_row) src_row[row] = (uint32_t)r;
        if (a >= 2u) {
            const int64_t d2 = d + ROW;
            st_stream(o_raw + d2, x);
            st_stream(o_m + d2, z);
            st_stream(o_v + d2, z);
            if (MODE != 0 || o_act != o_raw) st_stream(o_act + d2, y);
            if (ROW == 1 && src_row) src_row[row + 1] = (uint32_t)r;
        }
    }
}

// The built-in sampler (philox.hpp): key = the seed, counter = (row, child): a child's three normals depend on nothing else --
// not the launch shape, not P.
__device__ __forceinline__ void child_normals(uint64_t seed, int64_t row, int child, float n[3])
{
    uint32_t c[4] = { (uint32_t)row, (uint32_t)((uint64_t)row >> 32), (uint32_t)child, 0u };
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    box_muller3(c, n);
}

// ---- positions: one thread per source row (a split row's children need its scale and rotation)
__global__ void __launch_bounds__(256) k_densify_pos(int64_t P, const uint8_t* __restrict__ action, const uint32_t* __restrict__ incl,
                                                     const float* __restrict__ raw, const float* __restrict__ m,
                                                     const float* __restrict__ v, const float* __restrict__ raw_scale,
                                                     const float* __restrict__ raw_rotq, const float* __restrict__ noise,
                                                     uint64_t seed, float* __restrict__ o_raw, float* __restrict__ o_m,
                                                     float* __restrict__ o_v, float* o_act /* may alias o_raw */)
{
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < P; r += (int64_t)gridDim.x * 256) {
        const uint32_t a = action[r];
        if (a == 0u) continue;
        const int64_t d = ((int64_t)incl[r] - (a >= 2u ? 2 : 1)) * 3;
        const float   p[3] = { ld_stream(raw + 3 * r + 0), ld_stream(raw + 3 * r + 1), ld_stream(raw + 3 * r + 2) };
        if (a != 3u) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                st_stream(o_raw + d + c, p[c]);
                st_stream(o_m + d + c, ld_stream(m + 3 * r + c));
                st_stream(o_v + d + c, ld_stream(v + 3 * r + c));
                if (o_act != o_raw) st_stream(o_act + d + c, p[c]);
                if (a == 2u) {
                    st_stream(o_raw + d + 3 + c, p[c]);
                    st_stream(o_m + d + 3 + c, 0.0f);
                    st_stream(o_v + d + 3 + c, 0.0f);
                    if (o_act != o_raw) st_stream(o_act + d + 3 + c, p[c]);
                }
            }
            continue;
        }
        const float  s[3] = { act_exp(raw_scale[3 * r + 0]), act_exp(raw_scale[3 * r + 1]), act_exp(raw_scale[3 * r + 2]) };
        const float4 q    = act_unit(*reinterpret_cast<const float4*>(raw_rotq + 4 * r)); // stored (r, x, y, z)
        float        R[3][3];
        rot_from_quat(q.y, q.z, q.w, q.x, R);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            float n[3];
            if (noise) {
                n[0] = noise[(r * 2 + k) * 3 + 0];
                n[1] = noise[(r * 2 + k) * 3 + 1];
                n[2] = noise[(r * 2 + k) * 3 + 2];
            } else {
                child_normals(seed, r, k, n);
            }
            const float l[3] = { s[0] * n[0], s[1] * n[1], s[2] * n[2] };
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float x = p[c] + (R[0][c] * l[0] + R[1][c] * l[1] + R[2][c] * l[2]);
                st_stream(o_raw + d + 3 * k + c, x);
                st_stream(o_m + d + 3 * k + c, 0.0f);
                st_stream(o_v + d + 3 * k + c, 0.0f);
                if (o_act != o_raw) st_stream(o_act + d + 3 * k + c, x);
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_opacity_reset(int64_t P, float ceiling, float* __restrict__ raw, float* __restrict__ m,
                                                       float* __restrict__ v, float* __restrict__ act)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < P; i += (int64_t)gridDim.x * 256) {
        const float x = fminf(raw[i], ceiling);
        raw[i]        = x;
        st_stream(m + i, 0.0f);
        st_stream(v + i, 0.0f);
        act[i] = act_sigmoid(x);
    }
}

template <int ROW, int MODE, typename T>
void launch_rows(int64_t P, const uint8_t* action, const uint32_t* incl, const float* raw, const float* m, const float* v,
                 float* o_raw, float* o_m, float* o_v, float* o_act, float split_drop, uint32_t* src_row, hipStream_t stream)
{
    hipLaunchKernelGGL((k_densify_rows<ROW, MODE, T>), dim3(grid_256(P * ROW)), dim3(256), 0, stream, P, action, incl,
                       reinterpret_cast<const T*>(raw), reinterpret_cast<const T*>(m), reinterpret_cast<const T*>(v),
                       reinterpret_cast<T*>(o_raw), reinterpret_cast<T*>(o_m), reinterpret_cast<T*>(o_v),
                       reinterpret_cast<T*>(o_act), split_drop, src_row);
}

} // namespace

void launch_densify_stats(const KeptRows& r, float* grad_accum, uint32_t* denom, int32_t* max_radii, hipStream_t stream)
{
    hipLaunchKernelGGL(k_densify_stats, dim3(grid_256(r.hint)), dim3(256), 0, stream, r.vis_index, r.d_counts, r.P, r.cp,
                       r.scale_modifier, r.pos, r.scale, r.rotq, r.grads2d, grad_accum, denom, max_radii);
}

void launch_densify_classify(int64_t P, const DensifyRule& rule, const float* raw_scale, const float* raw_opacity,
                             const float* grad_accum, const uint32_t* denom, const int32_t* max_radii, uint32_t* emit,
                             uint8_t* action, hipStream_t stream)
{
    hipLaunchKernelGGL(k_densify_classify, dim3(grid_256(P)), dim3(256), 0, stream, P, rule, raw_scale, raw_opacity, grad_accum,
                       denom, max_radii, emit, action);
}

void launch_densify_scatter(int64_t P, int sh_floats, const uint8_t* action, const uint32_t* incl, const AdamArrays& raw,
                            const AdamArrays& m, const AdamArrays& v, const AdamArrays& o_raw, const AdamArrays& o_m,
                            const AdamArrays& o_v, const AdamArrays& o_act, float split_drop, const float* noise, uint64_t seed,
                            uint32_t* src_row, hipStream_t stream)
{
    hipLaunchKernelGGL(k_densify_pos, dim3(grid_256(P)), dim3(256), 0, stream, P, action, incl, raw.pos, m.pos, v.pos, raw.scale,
                       raw.rotq, noise, seed, o_raw.pos, o_m.pos, o_v.pos, o_act.pos);
    launch_rows<3, 1, float>(P, action, incl, raw.scale, m.scale, v.scale, o_raw.scale, o_m.scale, o_v.scale, o_act.scale,
                             split_drop, nullptr, stream);
    launch_rows<1, 3, float4>(P, action, incl, raw.rotq, m.rotq, v.rotq, o_raw.rotq, o_m.rotq, o_v.rotq, o_act.rotq, 0.0f,
                              nullptr, stream);
    const bool sh_aligned = ((reinterpret_cast<uintptr_t>(raw.sh) | reinterpret_cast<uintptr_t>(m.sh) |
                              reinterpret_cast<uintptr_t>(v.sh) | reinterpret_cast<uintptr_t>(o_raw.sh) |
                              reinterpret_cast<uintptr_t>(o_m.sh) | reinterpret_cast<uintptr_t>(o_v.sh) |
                              reinterpret_cast<uintptr_t>(o_act.sh)) & 15) == 0;
#define LCGS_DENSIFY_SH(ROW, T) \
    launch_rows<ROW, 0, T>(P, action, incl, raw.sh, m.sh, v.sh, o_raw.sh, o_m.sh, o_v.sh, o_act.sh, 0.0f, nullptr, stream)
    if (sh_floats == 48 && sh_aligned) LCGS_DENSIFY_SH(12, float4);
    else if (sh_floats == 48) LCGS_DENSIFY_SH(48, float);
    else if (sh_floats == 27) LCGS_DENSIFY_SH(27, float);
    else if (sh_floats == 12) LCGS_DENSIFY_SH(12, float);
    else LCGS_DENSIFY_SH(3, float);
#undef LCGS_DENSIFY_SH
    launch_rows<1, 2, float>(P, action, incl, raw.opacity, m.opacity, v.opacity, o_raw.opacity, o_m.opacity, o_v.opacity,
                             o_act.opacity, 0.0f, src_row, stream);
}

void launch_opacity_reset(int64_t P, float ceiling, float* raw, float* m, float* v, float* act, hipStream_t stream)
{
    hipLaunchKernelGGL(k_opacity_reset, dim3(grid_256(P)), dim3(256), 0, stream, P, ceiling, raw, m, v, act);
}

} // namespace lcgs
