// transform.hip -- a similarity transform of a scene's activated arrays (new = s R old + t; no reference
// counterpart), and the keep mask of a crop box.  The plan (include/lcgs_hip.h lcgs_similarity_plan: 100 floats) travels in the
// kernels' arguments; every lane reads it uniformly, so the matrices live in scalar registers.  Binary32, nothing contracted,
// every sum left to right as the header writes it: one defined bit pattern per output.
//   pos      ((M[i][0] x + M[i][1] y) + M[i][2] z) + t[i]; one lane owns four consecutive rows (3 float4)
//   scale    s * scale, a flat pass over 3 P floats, four per lane
//   rotq     the plan's quaternion times the row's, (w, x, y, z) as stored; one lane per row, one float4
//   sh       band l of every colour channel times D_l.  A row is up to 192 bytes: a workgroup stages a tile of 64 rows into LDS
//            with coalesced 16-byte loads, wave c rotates channel c of the 64 rows from LDS (lane = row: with an odd row stride
//            the 32 lanes of a bank group read 32 banks), and the tile goes back out coalesced.  A workgroup has read all of
//            its tile before it writes any of it: out == in works.  Rows of 12 and 27 floats take the same path; a tile of 64
//            of them is still a whole number of float4.  Arrays that are not 16-byte aligned, and the last partial tile, are
//            staged float by float.
//   keep     |b_k| <= half[k] for the three axes of b = the pos expression; a NaN fails a comparison: dropped
// None of the pointers is __restrict__: every output may be its input.
#include "launch.hpp"

namespace lcgs
{
namespace
{

// N floats per row, rows [i0, i0 + 4) clipped to P -> out[4 N]; rows beyond P read as 0 (filter3d.hip's idiom, without
// __restrict__)
template <int N>
__device__ __forceinline__ void load_rows4(const float* base, int64_t i0, int64_t P, float out[4 * N])
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
__device__ __forceinline__ void store_rows4(float* base, int64_t i0, int64_t P, const float in[4 * N])
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

__device__ __forceinline__ void transform_point(const TransformPlan& pl, const float p[3], float b[3])
{
#pragma unroll
    for (int i = 0; i < 3; ++i) b[i] = ((pl.M[3 * i + 0] * p[0] + pl.M[3 * i + 1] * p[1]) + pl.M[3 * i + 2] * p[2]) + pl.t[i];
}

__global__ void __launch_bounds__(256) k_transform_pos(int64_t P, TransformPlan pl, const float* pos, float* out)
{
    const int64_t quads = (P + 3) >> 2;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (int64_t)gridDim.x * 256) {
        float p[12], b[12];
        load_rows4<3>(pos, 4 * q, P, p);
#pragma unroll
        for (int r = 0; r < 4; ++r) transform_point(pl, p + 3 * r, b + 3 * r);
        store_rows4<3>(out, 4 * q, P, b);
    }
}

// n = 3 P floats
__global__ void __launch_bounds__(256) k_transform_scale(int64_t n, float s, const float* scale, float* out)
{
    const int64_t quads = (n + 3) >> 2;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (int64_t)gridDim.x * 256) {
        float v[4];
        load_rows4<1>(scale, 4 * q, n, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = s * v[e];
        store_rows4<1>(out, 4 * q, n, v);
    }
}

__global__ void __launch_bounds__(256) k_transform_rotq(int64_t P, TransformPlan pl, const float* rotq, float* out)
{
    const float W = pl.q[0], X = pl.q[1], Y = pl.q[2], Z = pl.q[3];
    const bool  vec_in = (reinterpret_cast<uintptr_t>(rotq) & 15) == 0, vec_out = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < P; i += (int64_t)gridDim.x * 256) {
        float4 a;
        if (vec_in)
            a = reinterpret_cast<const float4*>(rotq)[i];
        else
            a = make_float4(rotq[4 * i + 0], rotq[4 * i + 1], rotq[4 * i + 2], rotq[4 * i + 3]);
        const float w = a.x, x = a.y, y = a.z, z = a.w; // stored (w, x, y, z)
        float4      o;
        o.x = ((W * w - X * x) - Y * y) - Z * z;
        o.y = ((W * x + X * w) + Y * z) - Z * y;
        o.z = ((W * y - X * z) + Y * w) + Z * x;
        o.w = ((W * z + X * y) - Y * x) + Z * w;
        if (vec_out)
            reinterpret_cast<float4*>(out)[i] = o;
        else
            out[4 * i + 0] = o.x, out[4 * i + 1] = o.y, out[4 * i + 2] = o.z, out[4 * i + 3] = o.w;
    }
}

// band of N = 2 l + 1 coefficients of one channel of one row, in LDS at p[3 j]: c'_k = sum_j D[k][j] c_j, j ascending, the sum
// started from its first product
template <int N>
__device__ __forceinline__ void rotate_band(const float* D, float* p)
{
    float in[N], o[N];
#pragma unroll
    for (int j = 0; j < N; ++j) in[j] = p[3 * j];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        float acc = D[k * N] * in[0];
#pragma unroll
        for (int j = 1; j < N; ++j) acc = acc + D[k * N + j] * in[j];
        o[k] = acc;
    }
#pragma unroll
    for (int k = 0; k < N; ++k) p[3 * k] = o[k];
}

constexpr int kShThreads = 3 * kTransformTileRows; // wave c = colour channel c, lane = row of the tile

template <int DEG>
__global__ void __launch_bounds__(kShThreads) k_transform_sh(int64_t P, TransformPlan pl, const float* sh, float* out)
{
    constexpr int W = 3 * (DEG + 1) * (DEG + 1); // floats per row: 12, 27, 48
    constexpr int S = W | 1;                     // LDS row stride in words, odd
    constexpr int R = kTransformTileRows;
    static_assert((R * W) % 4 == 0, "a full tile is a whole number of float4");
    __shared__ float tile[R * S];
    const int64_t row0 = (int64_t)blockIdx.x * R;
    const int     rows = (int)(P - row0 < R ? P - row0 : R); // >= 1: the grid is ceil(P / R)
    const int     n    = rows * W;
    const float*  src  = sh + row0 * W;
    float*        dst  = out + row0 * W;
    // (a tile starts a multiple of 256 W bytes into its array: it is 16-byte aligned iff the array is)
    if (rows == R && (reinterpret_cast<uintptr_t>(sh) & 15) == 0) {
        for (int i = threadIdx.x; i < R * W / 4; i += kShThreads) {
            const float4 v = reinterpret_cast<const float4*>(src)[i];
            const float  e[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int g = 4 * i + k;
                tile[(g / W) * S + g % W] = e[k];
            }
        }
    } else {
        for (int g = threadIdx.x; g < n; g += kShThreads) tile[(g / W) * S + g % W] = src[g];
    }
    __syncthreads();
    {
        const int r = threadIdx.x & (R - 1), c = threadIdx.x / R;
        if (r < rows) { // (coefficient 0 stays as it was staged: a bit copy)
            float* p = tile + r * S + c;
            rotate_band<3>(pl.D1, p + 3 * 1);
            if (DEG >= 2) rotate_band<5>(pl.D2, p + 3 * 4);
            if (DEG >= 3) rotate_band<7>(pl.D3, p + 3 * 9);
        }
    }
    __syncthreads();
    if (rows == R && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
        for (int i = threadIdx.x; i < R * W / 4; i += kShThreads) {
            float e[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int g = 4 * i + k;
                e[k]        = tile[(g / W) * S + g % W];
            }
            reinterpret_cast<float4*>(dst)[i] = make_float4(e[0], e[1], e[2], e[3]);
        }
    } else {
        for (int g = threadIdx.x; g < n; g += kShThreads) dst[g] = tile[(g / W) * S + g % W];
    }
}

struct Half3 {
    float h[3];
};
__global__ void __launch_bounds__(256) k_box_keep_mask(int64_t P, TransformPlan pl, const float* __restrict__ pos, Half3 half,
                                                       uint8_t* __restrict__ keep)
{
    const int64_t quads = (P + 3) >> 2;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (int64_t)gridDim.x * 256) {
        const int64_t i0 = 4 * q;
        float         p[12];
        load_rows4<3>(pos, i0, P, p);
        uint32_t word = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float b[3];
            transform_point(pl, p + 3 * r, b);
            // every comparison evaluated, no branch; a NaN fails them all
            const uint32_t in = uint32_t(fabsf(b[0]) <= half.h[0]) & uint32_t(fabsf(b[1]) <= half.h[1]) & uint32_t(fabsf(b[2]) <= half.h[2]);
            word |= in << (8 * r);
        }
        if (i0 + 4 <= P && (reinterpret_cast<uintptr_t>(keep) & 3) == 0) {
            reinterpret_cast<uint32_t*>(keep)[q] = word; // little-endian: byte r is row i0 + r
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (i0 + r < P) keep[i0 + r] = (uint8_t)((word >> (8 * r)) & 1u);
        }
    }
}

} // namespace

void launch_scene_transform(int64_t P, int sh_degree, const TransformPlan& plan, const float* pos, const float* scale,
                            const float* rotq, const float* sh, float* pos_out, float* scale_out, float* rotq_out, float* sh_out,
                            hipStream_t stream)
{
    if (pos_out) hipLaunchKernelGGL(k_transform_pos, dim3(grid_256((P + 3) / 4)), dim3(256), 0, stream, P, plan, pos, pos_out);
    if (scale_out)
        hipLaunchKernelGGL(k_transform_scale, dim3(grid_256((3 * P + 3) / 4)), dim3(256), 0, stream, 3 * P, plan.s, scale, scale_out);
    if (rotq_out) hipLaunchKernelGGL(k_transform_rotq, dim3(grid_256(P)), dim3(256), 0, stream, P, plan, rotq, rotq_out);
    if (sh_out && sh_degree >= 1) {
        const dim3 grid((unsigned)((P + kTransformTileRows - 1) / kTransformTileRows)), block(kShThreads);
        if (sh_degree == 1)
            hipLaunchKernelGGL(k_transform_sh<1>, grid, block, 0, stream, P, plan, sh, sh_out);
        else if (sh_degree == 2)
            hipLaunchKernelGGL(k_transform_sh<2>, grid, block, 0, stream, P, plan, sh, sh_out);
        else
            hipLaunchKernelGGL(k_transform_sh<3>, grid, block, 0, stream, P, plan, sh, sh_out);
    }
}

void launch_box_keep_mask(int64_t P, const TransformPlan& plan, const float* pos, const float half[3], uint8_t* keep,
                          hipStream_t stream)
{
    const Half3 h = { { half[0], half[1], half[2] } };
    hipLaunchKernelGGL(k_box_keep_mask, dim3(grid_256((P + 3) / 4)), dim3(256), 0, stream, P, plan, pos, h, keep);
}

} // namespace lcgs
