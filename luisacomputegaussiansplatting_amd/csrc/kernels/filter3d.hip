// filter3d.hip -- Mip-Splatting's 3-D smoothing filter (Yu et al., CVPR 2024; no reference counterpart): every
// splat's size is bounded from below by the highest rate at which any training view sampled it.
//   accumulate  min_z[i] = the smallest view depth of row i over the views that see it (Mip-Splatting's compute_3D_filter
//               visibility rule, stated in the tangent plane with cam_clamp's 1.3 tan(fov / 2) limit).  The hot pass: every row
//               against every view.  One lane owns four consecutive rows (3 float4 of positions, 1 float4 of min_z, read and
//               written once per launch); the views are looped inside the kernel from a table in the kernel's arguments that
//               every lane reads uniformly (scalar loads: 14 floats per view per wave), so a (row, view) pair costs its ~25
//               vector operations and nothing else.  No atomics: one lane owns a row.
//   finalize    filter[i] = ((finite min_z[i] ? min_z[i] : zmax) / max_focal) * sqrt(0.2), zmax = the largest finite min_z: a
//               per-wave, per-block reduction of order-preserving integer keys, one atomic max per block into one word (a max
//               does not depend on order), then one element-wise pass that reads the word.  No host read-back.
//   apply       scale_out = sqrt(s^2 + f^2), opacity_out = opacity * sqrt(prod_k s_k^2 / (s_k^2 + f^2)): the determinant ratio
//               as a product of three ratios in [0, 1] -- it cannot underflow where prod(s^2) does
//   backward    gradients with respect to the filtered values -> with respect to the unfiltered ones, in place; dense rows or the
//               compact rows of lcgs_render_backward_compact
// Element-wise passes handle four rows per lane with float4 accesses where the arrays are 16-byte aligned (scalar accesses
// otherwise, and for the last rows of a count that is no multiple of four).
#include "launch.hpp"

namespace lcgs
{
namespace
{

// N floats per row, rows [i0, i0 + 4) clipped to P -> out[4 N]; rows beyond P read as 0
template <int N>
__device__ __forceinline__ void load_rows4(const float* __restrict__ base, int64_t i0, int64_t P, float out[4 * N])
{
    const float* p = base + (int64_t)N * i0;
    if (i0 + 4 <= P && (reinterpret_cast<uintptr_t>(base) & 15) == 0) {
#pragma unroll
        for (int q = 0; q < N; ++q) {
            const float4 t = reinterpret_cast<const float4*>(p)[q];
            out[4 * q + 0] = t.x, out[4 * q + 1] = t.y, out[4 * q + 2] = t.z, out[4 * q + 3] = t.w;
        }
    } else {
        const int64_t n = (P - i0 < 4 ? P - i0 : 4) * N;
#pragma unroll
        for (int e = 0; e < 4 * N; ++e) out[e] = e < n ? p[e] : 0.0f;
    }
}
template <int N>
__device__ __forceinline__ void store_rows4(float* __restrict__ base, int64_t i0, int64_t P, const float in[4 * N])
{
    float* p = base + (int64_t)N * i0;
    if (i0 + 4 <= P && (reinterpret_cast<uintptr_t>(base) & 15) == 0) {
#pragma unroll
        for (int q = 0; q < N; ++q)
            reinterpret_cast<float4*>(p)[q] = make_float4(in[4 * q + 0], in[4 * q + 1], in[4 * q + 2], in[4 * q + 3]);
    } else {
        const int64_t n = (P - i0 < 4 ? P - i0 : 4) * N;
#pragma unroll
        for (int e = 0; e < 4 * N; ++e)
            if (e < n) p[e] = in[e];
    }
}

// ---- accumulate
__global__ void __launch_bounds__(256) k_filter3d_accumulate(int64_t P, const float* __restrict__ pos, int num_views,
                                                             Filter3dViews views, float* __restrict__ min_z)
{
    const int64_t quads = (P + 3) >> 2;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (int64_t)gridDim.x * 256) {
        const int64_t i0 = 4 * q;
        float         p[12], mz[4];
        load_rows4<3>(pos, i0, P, p);
        load_rows4<1>(min_z, i0, P, mz);
        for (int k = 0; k < num_views; ++k) {
            const Filter3dView c = views.v[k]; // uniform: scalar loads, once per view and wave
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float px = p[3 * r + 0], py = p[3 * r + 1], pz = p[3 * r + 2];
                // gs_math.hpp view_transform, same operation order
                const float vx = c.right[0] * px + c.right[1] * py + c.right[2] * pz + c.tx;
                const float vy = c.up[0] * px + c.up[1] * py + c.up[2] * pz + c.ty;
                const float vz = c.front[0] * px + c.front[1] * py + c.front[2] * pz + c.tz;
                // every comparison evaluated, no branch; a NaN fails them all: never seen
                const int seen = int(vz > 0.2f) & int(fabsf(vx) <= c.limx * vz) & int(fabsf(vy) <= c.limy * vz);
                mz[r]          = (seen & int(vz < mz[r])) ? vz : mz[r];
            }
        }
        store_rows4<1>(min_z, i0, P, mz);
    }
}

// ---- finalize
// finite floats -> u32 keys in the floats' order, all above 0; anything else -> 0 ("no finite entry")
__device__ __forceinline__ uint32_t finite_key(float x)
{
    const uint32_t b = __float_as_uint(x);
    if ((b & 0x7F800000u) == 0x7F800000u) return 0u; // inf, NaN
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
__global__ void __launch_bounds__(256) k_filter3d_zmax(int64_t P, const float* __restrict__ min_z, uint32_t* __restrict__ word)
{
    __shared__ uint32_t s_wave[4];
    const int64_t       quads = (P + 3) >> 2;
    uint32_t            best  = 0u;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (int64_t)gridDim.x * 256) {
        float z[4];
        load_rows4<1>(min_z, 4 * q, P, z);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (4 * q + r < P) best = max(best, finite_key(z[r]));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) best = max(best, (uint32_t)__shfl_down((int)best, off, 64));
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t m = max(max(s_wave[0], s_wave[1]), max(s_wave[2], s_wave[3]));
        if (m) atomicMax(word, m);
    }
}
__global__ void __launch_bounds__(256) k_filter3d_finalize(int64_t P, const float* __restrict__ min_z, float max_focal,
                                                           const uint32_t* __restrict__ word, float* __restrict__ filter)
{
    const uint32_t key   = *word;
    const float    zmax  = key_value(key);
    const float    c     = 0.44721359549995794f; // binary32 nearest to sqrt(0.2)
    const int64_t  quads = (P + 3) >> 2;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (int64_t)gridDim.x * 256) {
        float z[4], f[4];
        load_rows4<1>(min_z, 4 * q, P, z);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool finite = (__float_as_uint(z[r]) & 0x7F800000u) != 0x7F800000u;
            f[r]              = key ? ((finite ? z[r] : zmax) / max_focal) * c : 0.0f;
        }
        store_rows4<1>(filter, 4 * q, P, f);
    }
}

// ---- apply / backward: one row
struct Filtered {
    float b[3], sf[3], coef;
};
__device__ __forceinline__ Filtered filtered_row(const float s[3], float f2)
{
    Filtered o;
    float    r[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float a = s[k] * s[k];
        o.b[k]        = a + f2;
        o.sf[k]       = sqrtf(o.b[k]);
        r[k]          = a / o.b[k];
    }
    o.coef = sqrtf((r[0] * r[1]) * r[2]);
    return o;
}
__global__ void __launch_bounds__(256) k_filter3d_apply(int64_t P, const float* __restrict__ scale, const float* __restrict__ opacity,
                                                        const float* __restrict__ filter, float* __restrict__ scale_out,
                                                        float* __restrict__ opacity_out)
{
    const int64_t quads = (P + 3) >> 2;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (int64_t)gridDim.x * 256) {
        const int64_t i0 = 4 * q;
        float         s[12], o[4], f[4];
        load_rows4<3>(scale, i0, P, s);
        load_rows4<1>(opacity, i0, P, o);
        load_rows4<1>(filter, i0, P, f);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (f[r] == 0.0f) continue; // the identity filter: the row is copied bit for bit
            const Filtered t = filtered_row(s + 3 * r, f[r] * f[r]);
            s[3 * r + 0] = t.sf[0], s[3 * r + 1] = t.sf[1], s[3 * r + 2] = t.sf[2];
            o[r]         = o[r] * t.coef;
        }
        store_rows4<3>(scale_out, i0, P, s);
        store_rows4<1>(opacity_out, i0, P, o);
    }
}
// g_s, g_o: the gradients with respect to the filtered row, replaced by those with respect to (s, o)
__device__ __forceinline__ void backward_row(const float s[3], float o, float f, float g_s[3], float& g_o)
{
    if (f == 0.0f) return;
    const float    f2 = f * f;
    const Filtered t  = filtered_row(s, f2);
    const float    w  = ((g_o * o) * t.coef) * f2;
#pragma unroll
    for (int k = 0; k < 3; ++k) g_s[k] = g_s[k] * (s[k] / t.sf[k]) + w / (s[k] * t.b[k]);
    g_o = g_o * t.coef;
}
__global__ void __launch_bounds__(256) k_filter3d_backward_dense(int64_t P, const float* __restrict__ scale,
                                                                 const float* __restrict__ opacity, const float* __restrict__ filter,
                                                                 float* __restrict__ g_scale, float* __restrict__ g_opacity)
{
    const int64_t quads = (P + 3) >> 2;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (int64_t)gridDim.x * 256) {
        const int64_t i0 = 4 * q;
        float         s[12], o[4], f[4], gs[12], go[4];
        load_rows4<3>(scale, i0, P, s);
        load_rows4<1>(opacity, i0, P, o);
        load_rows4<1>(filter, i0, P, f);
        load_rows4<3>(g_scale, i0, P, gs);
        load_rows4<1>(g_opacity, i0, P, go);
#pragma unroll
        for (int r = 0; r < 4; ++r) backward_row(s + 3 * r, o[r], f[r], gs + 3 * r, go[r]);
        store_rows4<3>(g_scale, i0, P, gs);
        store_rows4<1>(g_opacity, i0, P, go);
    }
}
// gradient row r < *d_count belongs to row rows[r] (ascending) of scale / opacity / filter
__global__ void __launch_bounds__(256) k_filter3d_backward_compact(int64_t P, const float* __restrict__ scale,
                                                                   const float* __restrict__ opacity,
                                                                   const float* __restrict__ filter, const uint32_t* __restrict__ rows,
                                                                   const uint32_t* __restrict__ d_count, float* __restrict__ g_scale,
                                                                   float* __restrict__ g_opacity)
{
    const int64_t count = (int64_t)*d_count < P ? (int64_t)*d_count : P;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < count; r += (int64_t)gridDim.x * 256) {
        const int64_t i = (int64_t)rows[r];
        if (i >= P) continue;
        const float f = filter[i];
        if (f == 0.0f) continue;
        const float s[3] = { scale[3 * i + 0], scale[3 * i + 1], scale[3 * i + 2] };
        float       gs[3] = { g_scale[3 * r + 0], g_scale[3 * r + 1], g_scale[3 * r + 2] };
        float       go    = g_opacity[r];
        backward_row(s, opacity[i], f, gs, go);
        g_scale[3 * r + 0] = gs[0], g_scale[3 * r + 1] = gs[1], g_scale[3 * r + 2] = gs[2];
        g_opacity[r]       = go;
    }
}

} // namespace

void launch_filter3d_accumulate(int64_t P, const float* pos, int num_views, const Filter3dViews& views, float* min_z,
                                hipStream_t stream)
{
    hipLaunchKernelGGL(k_filter3d_accumulate, dim3(grid_256((P + 3) / 4)), dim3(256), 0, stream, P, pos, num_views, views, min_z);
}

void launch_filter3d_finalize(int64_t P, const float* min_z, float max_focal, uint32_t* word, float* filter, hipStream_t stream)
{
    // a few blocks per CU: one atomic each
    const unsigned blocks = grid_256((P + 3) / 4) < 2048u ? grid_256((P + 3) / 4) : 2048u;
    hipLaunchKernelGGL(k_filter3d_zmax, dim3(blocks), dim3(256), 0, stream, P, min_z, word);
    hipLaunchKernelGGL(k_filter3d_finalize, dim3(grid_256((P + 3) / 4)), dim3(256), 0, stream, P, min_z, max_focal, word, filter);
}

void launch_filter3d_apply(int64_t P, const float* scale, const float* opacity, const float* filter, float* scale_out,
                           float* opacity_out, hipStream_t stream)
{
    hipLaunchKernelGGL(k_filter3d_apply, dim3(grid_256((P + 3) / 4)), dim3(256), 0, stream, P, scale, opacity, filter, scale_out,
                       opacity_out);
}

void launch_filter3d_backward(int64_t P, const float* scale, const float* opacity, const float* filter, const uint32_t* rows,
                              const uint32_t* d_count, float* g_scale, float* g_opacity, hipStream_t stream)
{
    if (rows)
        hipLaunchKernelGGL(k_filter3d_backward_compact, dim3(grid_256(P)), dim3(256), 0, stream, P, scale, opacity, filter, rows,
                           d_count, g_scale, g_opacity);
    else
        hipLaunchKernelGGL(k_filter3d_backward_dense, dim3(grid_256((P + 3) / 4)), dim3(256), 0, stream, P, scale, opacity, filter,
                           g_scale, g_opacity);
}

} // namespace lcgs
