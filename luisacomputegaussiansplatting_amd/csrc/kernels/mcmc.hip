// mcmc.hip -- 3DGS-MCMC density control (Kheradmand et al., NeurIPS 2024): dead splats are relocated onto live
// ones drawn with probability proportional to opacity, the set grows the same way, opacity and scale of a source and its
// copies are corrected so that the rendered image stays (nearly) what it was, positions receive SGLD noise shaped by each
// splat's covariance, and opacity / scale are L1-regularised.  No reference counterpart (doc/roadmap.md:4 only names training).
//   weights     w_i = dead ? 0 : (uint32_t)(sigmoid(raw opacity) * 2^24): integers, so their u64 sums are exact and order free --
//               the sampler can be restated bit for bit off the GPU (tests/mcmc_ref.py)
//   sampler     draw j: Philox(seed; j, tag) -> u in [0, 2^64) -> t = mulhi64(u, T) in [0, T) -> the first row whose inclusive
//               sum exceeds t; u32 atomic adds count the draws per source (integer: order free)
//   values      binary64 from the binary32 raw inputs, rounded once: the work touches a few percent of the rows once per
//               hundred steps, and binary32 loses 1.6e-3 of the scale factor at o = 1 - 1e-7
//   K1 / K2     the update is IN PLACE: K1 (per draw) reads a source's original scale / opacity and writes a dead or appended
//               row; K2 (per source) then rewrites the source itself.  Dead and appended rows have weight 0 and are never
//               sources, so K1's reads and writes never meet.
// The u64 inclusive sum of the weights is scan.hip's (launch_inclusive_sum_u64).
#include "activations.hpp"
#include "launch.hpp"
#include "philox.hpp"
#include "stream_access.hpp"

namespace lcgs
{
namespace
{

// ---- weights and the dead set: one thread per row
__global__ void __launch_bounds__(256) k_mcmc_weights(int64_t P, float min_opacity, const float* __restrict__ raw_opacity,
                                                      uint32_t* __restrict__ w, uint32_t* __restrict__ dead,
                                                      uint32_t* __restrict__ src_row)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < P; i += (int64_t)gridDim.x * 256) {
        const float o = act_sigmoid(raw_opacity[i]);
        const bool  d = !(o > min_opacity); // a NaN opacity is dead; o == min_opacity is dead
        w[i]          = d ? 0u : (uint32_t)(o * 16777216.0f);
        if (dead) dead[i] = d ? 1u : 0u;
        if (src_row) src_row[i] = (uint32_t)i;
    }
}

__global__ void __launch_bounds__(256) k_mcmc_dead_list(int64_t P, const uint32_t* __restrict__ dead,
                                                        const uint32_t* __restrict__ dead_incl, uint32_t* __restrict__ dead_list)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < P; i += (int64_t)gridDim.x * 256)
        if (dead[i]) dead_list[dead_incl[i] - 1u] = (uint32_t)i; // (dead_incl[i] >= 1 here and <= P)
}

// ---- the sampler: one thread per draw
__global__ void __launch_bounds__(256) k_mcmc_draw(int64_t P, int64_t n_host, const uint32_t* __restrict__ d_n,
                                                   const uint64_t* __restrict__ cdf, const uint32_t* __restrict__ w,
                                                   const uint32_t* __restrict__ src_in, uint64_t seed, uint32_t tag,
                                                   uint32_t* __restrict__ draw_src, uint32_t* __restrict__ count,
                                                   uint32_t* __restrict__ status)
{
    const int64_t  D = d_n ? (int64_t)*d_n : n_host;
    const uint64_t T = cdf[P - 1];
    if (T == 0) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, 2u);
        return;
    }
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < D; j += (int64_t)gridDim.x * 256) {
        uint32_t s;
        if (src_in) {
            s = src_in[j];
            if ((int64_t)s >= P || w[s] == 0u) {
                atomicOr(status, 1u);
                continue;
            }
        } else {
            uint32_t c[4] = { (uint32_t)j, (uint32_t)((uint64_t)j >> 32), tag, 0u };
            philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
            const uint64_t u = (uint64_t)c[0] | ((uint64_t)c[1] << 32);
            const uint64_t t = __umul64hi(u, T); // in [0, T)
            int64_t lo = 0, hi = P - 1;          // the smallest i with cdf[i] > t: cdf[P - 1] = T > t, so it exists
            while (lo < hi) {
                const int64_t mid = lo + ((hi - lo) >> 1);
                if (cdf[mid] > t) hi = mid;
                else lo = mid + 1;
            }
            s = (uint32_t)lo; // (w[s] > 0: cdf[s] > t >= cdf[s - 1])
        }
        draw_src[j] = s;
        atomicAdd(count + s, 1u);
    }
}

// ---- relocation values, binary64
struct BinomTable {
    double c[kMcmcMaxN][kMcmcMaxN]; // c[i][k] = C(i, k), exact in binary64 (C(50, 25) < 2^47)
};
constexpr BinomTable make_binoms()
{
    BinomTable t{};
    for (int i = 0; i < kMcmcMaxN; ++i) {
        t.c[i][0] = 1.0;
        for (int k = 1; k <= i; ++k) t.c[i][k] = t.c[i - 1][k - 1] + (k < i ? t.c[i - 1][k] : 0.0);
    }
    return t;
}
__constant__ BinomTable c_binom = make_binoms();

struct Relocated {
    double log_c;       // added to every raw scale component
    float  raw_opacity; // the new raw opacity
};
// x: the source's ORIGINAL raw opacity, count: draws that landed on it.  One body for K1 and K2: a copy's values are its
// source's bit for bit.
__device__ __noinline__ Relocated mcmc_relocated(float x, uint32_t count, McmcRule rule)
{
    const int    n  = (int)min(count, (uint32_t)(rule.n_max - 1)) + 1; // min(count + 1, n_max)
    const double xd = (double)x;
    const double o  = 1.0 / (1.0 + exp(-xd));
    const double q  = 1.0 / (1.0 + exp(xd)); // 1 - o without the cancellation
    const double op = 1.0 - pow(q, 1.0 / (double)n);
    double       D  = 0.0;
    for (int i = 1; i <= n; ++i) {
        double pw = op; // op^(k + 1)
        for (int k = 0; k < i; ++k) {
            const double term = c_binom.c[i - 1][k] * pw / sqrt((double)(k + 1));
            D                 = (k & 1) ? D - term : D + term;
            pw *= op;
        }
    }
    Relocated r;
    r.log_c         = log(o / D);
    const double oh = fmin(fmax(op, (double)rule.min_opacity), 1.0 - 1.1920928955078125e-07 /* 2^-23 */);
    float ro        = (float)(log(oh) - log1p(-oh));
    // at the clamp's lower end the rounded value's binary32 sigmoid may not exceed min_opacity: the row would be dead again at
    // once.  The next binary32 values up until it is live (one step at min_opacity = 0.005, where a step moves o by 5 ulp)
    for (int it = 0; it < 64 && !(act_sigmoid(ro) > rule.min_opacity); ++it) ro = nextafterf(ro, INFINITY);
    r.raw_opacity = ro;
    return r;
}
__device__ __forceinline__ void write_scale_opacity(const Relocated& r, const float sc[3], int64_t dst, const AdamArrays& raw,
                                                    const AdamArrays& m, const AdamArrays& v, const AdamArrays& act)
{
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float s         = (float)((double)sc[c] + r.log_c);
        raw.scale[3 * dst + c] = s;
        m.scale[3 * dst + c]   = 0.0f;
        v.scale[3 * dst + c]   = 0.0f;
        act.scale[3 * dst + c] = act_exp(s);
    }
    raw.opacity[dst] = r.raw_opacity;
    m.opacity[dst]   = 0.0f;
    v.opacity[dst]   = 0.0f;
    act.opacity[dst] = act_sigmoid(r.raw_opacity);
}

// K1, per draw: everything of the destination row except its SH
__global__ void __launch_bounds__(256) k_mcmc_place(int64_t D, const uint32_t* __restrict__ dead_list, int64_t dst_first,
                                                    const uint32_t* __restrict__ draw_src, const uint32_t* __restrict__ count,
                                                    McmcRule rule, AdamArrays raw, AdamArrays m, AdamArrays v, AdamArrays act,
                                                    uint32_t* __restrict__ src_row)
{
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < D; j += (int64_t)gridDim.x * 256) {
        const int64_t   s   = (int64_t)draw_src[j];
        const int64_t   dst = dead_list ? (int64_t)dead_list[j] : dst_first + j;
        const float     sc[3] = { raw.scale[3 * s + 0], raw.scale[3 * s + 1], raw.scale[3 * s + 2] };
        const Relocated r   = mcmc_relocated(raw.opacity[s], count[s], rule);
        write_scale_opacity(r, sc, dst, raw, m, v, act);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float p        = raw.pos[3 * s + c];
            raw.pos[3 * dst + c] = p;
            m.pos[3 * dst + c]   = 0.0f;
            v.pos[3 * dst + c]   = 0.0f;
            if (act.pos != raw.pos) act.pos[3 * dst + c] = p;
        }
        const float4 q = *reinterpret_cast<const float4*>(raw.rotq + 4 * s);
        const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        *reinterpret_cast<float4*>(raw.rotq + 4 * dst) = q;
        *reinterpret_cast<float4*>(m.rotq + 4 * dst)   = z;
        *reinterpret_cast<float4*>(v.rotq + 4 * dst)   = z;
        *reinterpret_cast<float4*>(act.rotq + 4 * dst) = act_unit(q);
        if (src_row) src_row[dead_list ? dst : j] = (uint32_t)s;
    }
}
// ... and its SH: one thread per (draw, float)
__global__ void __launch_bounds__(256) k_mcmc_place_sh(int64_t D, int shf, const uint32_t* __restrict__ dead_list, int64_t dst_first,
                                                       const uint32_t* __restrict__ draw_src, float* raw, float* __restrict__ m,
                                                       float* __restrict__ v, float* act /* may be raw */)
{
    const int64_t total = D * shf;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t j   = e / shf;
        const int     c   = (int)(e - j * shf);
        const int64_t s   = (int64_t)draw_src[j];
        const int64_t dst = dead_list ? (int64_t)dead_list[j] : dst_first + j;
        const float   x   = raw[s * shf + c];
        raw[dst * shf + c] = x;
        m[dst * shf + c]   = 0.0f;
        v[dst * shf + c]   = 0.0f;
        if (act != raw) act[dst * shf + c] = x;
    }
}
// K2, per source row: in place
__global__ void __launch_bounds__(256) k_mcmc_sources(int64_t P, int shf, const uint32_t* __restrict__ count, McmcRule rule,
                                                      AdamArrays raw, AdamArrays m, AdamArrays v, AdamArrays act)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < P; i += (int64_t)gridDim.x * 256) {
        const uint32_t n = count[i];
        if (n == 0u) continue;
        const float     sc[3] = { raw.scale[3 * i + 0], raw.scale[3 * i + 1], raw.scale[3 * i + 2] };
        const Relocated r   = mcmc_relocated(raw.opacity[i], n, rule);
        write_scale_opacity(r, sc, i, raw, m, v, act);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            m.pos[3 * i + c] = 0.0f;
            v.pos[3 * i + c] = 0.0f;
        }
        const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        *reinterpret_cast<float4*>(m.rotq + 4 * i) = z;
        *reinterpret_cast<float4*>(v.rotq + 4 * i) = z;
        for (int c = 0; c < shf; ++c) {
            m.sh[i * shf + c] = 0.0f;
            v.sh[i * shf + c] = 0.0f;
        }
    }
}

// ---- SGLD noise: one thread per row, 44 bytes read and 12 written
__global__ void __launch_bounds__(256) k_mcmc_noise(int64_t P, float gain, float k, float x0, const float* __restrict__ raw_opacity,
                                                    const float* __restrict__ raw_scale, const float* __restrict__ raw_rotq,
                                                    const float* __restrict__ noise, uint64_t seed, uint32_t step, float* raw_pos,
                                                    float* act_pos /* may be raw_pos */)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < P; i += (int64_t)gridDim.x * 256) {
        const float  o = act_sigmoid(ld_stream(raw_opacity + i));
        const float  g = 1.0f / (1.0f + expf(-k * ((1.0f - o) - x0)));
        const float  a = gain * g;
        const float  s[3] = { act_exp(ld_stream(raw_scale + 3 * i + 0)), act_exp(ld_stream(raw_scale + 3 * i + 1)),
                              act_exp(ld_stream(raw_scale + 3 * i + 2)) };
        const float4 q = act_unit(ld_stream(reinterpret_cast<const float4*>(raw_rotq + 4 * i))); // stored (r, x, y, z)
        float        R[3][3];                                                                    // [column][row]
        rot_from_quat(q.y, q.z, q.w, q.x, R);
        float e[3];
        if (noise) {
            e[0] = ld_stream(noise + 3 * i + 0);
            e[1] = ld_stream(noise + 3 * i + 1);
            e[2] = ld_stream(noise + 3 * i + 2);
        } else {
            uint32_t c[4] = { (uint32_t)i, (uint32_t)((uint64_t)i >> 32), kMcmcTagNoise, step };
            philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
            box_muller3(c, e);
        }
        // Sigma eps = R S^2 R^T eps
        float t[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) t[j] = (R[j][0] * e[0] + R[j][1] * e[1] + R[j][2] * e[2]) * (s[j] * s[j]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float d = R[0][c] * t[0] + R[1][c] * t[1] + R[2][c] * t[2];
            const float p = ld_stream(raw_pos + 3 * i + c) + a * d;
            st_stream(raw_pos + 3 * i + c, p);
            if (act_pos != raw_pos) st_stream(act_pos + 3 * i + c, p);
        }
    }
}

__global__ void __launch_bounds__(256) k_mcmc_regularize(int64_t P, float add_opacity, float add_scale, float* __restrict__ d_opacity,
                                                         float* __restrict__ d_scale)
{
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < 3 * P; e += (int64_t)gridDim.x * 256) {
        d_scale[e] += add_scale;
        if (e < P) d_opacity[e] += add_opacity;
    }
}

} // namespace

void launch_mcmc_weights(int64_t P, float min_opacity, const float* raw_opacity, uint32_t* w, uint32_t* dead, uint32_t* src_row,
                         hipStream_t stream)
{
    hipLaunchKernelGGL(k_mcmc_weights, dim3(grid_256(P)), dim3(256), 0, stream, P, min_opacity, raw_opacity, w, dead, src_row);
}

void launch_mcmc_dead_list(int64_t P, const uint32_t* dead, const uint32_t* dead_incl, uint32_t* dead_list, hipStream_t stream)
{
    hipLaunchKernelGGL(k_mcmc_dead_list, dim3(grid_256(P)), dim3(256), 0, stream, P, dead, dead_incl, dead_list);
}

void launch_mcmc_draw(int64_t P, int64_t n_launch, int64_t n_host, const uint32_t* d_n, const uint64_t* cdf, const uint32_t* w,
                      const uint32_t* src_in, uint64_t seed, uint32_t tag, uint32_t* draw_src, uint32_t* count, uint32_t* status,
                      hipStream_t stream)
{
    hipLaunchKernelGGL(k_mcmc_draw, dim3(grid_256(n_launch)), dim3(256), 0, stream, P, n_host, d_n, cdf, w, src_in, seed, tag,
                       draw_src, count, status);
}

void launch_mcmc_place(int64_t D, int sh_floats, const uint32_t* dead_list, int64_t dst_first, const uint32_t* draw_src,
                       const uint32_t* count, const McmcRule& rule, const AdamArrays& raw, const AdamArrays& m, const AdamArrays& v,
                       const AdamArrays& act, uint32_t* src_row, hipStream_t stream)
{
    hipLaunchKernelGGL(k_mcmc_place, dim3(grid_256(D)), dim3(256), 0, stream, D, dead_list, dst_first, draw_src, count, rule, raw, m,
                       v, act, src_row);
    hipLaunchKernelGGL(k_mcmc_place_sh, dim3(grid_256(D * sh_floats)), dim3(256), 0, stream, D, sh_floats, dead_list, dst_first,
                       draw_src, raw.sh, m.sh, v.sh, act.sh);
}

void launch_mcmc_sources(int64_t P, int sh_floats, const uint32_t* count, const McmcRule& rule, const AdamArrays& raw,
                         const AdamArrays& m, const AdamArrays& v, const AdamArrays& act, hipStream_t stream)
{
    hipLaunchKernelGGL(k_mcmc_sources, dim3(grid_256(P)), dim3(256), 0, stream, P, sh_floats, count, rule, raw, m, v, act);
}

void launch_mcmc_noise(int64_t P, float gain, float k, float x0, const float* raw_opacity, const float* raw_scale,
                       const float* raw_rotq, const float* noise, uint64_t seed, uint32_t step, float* raw_pos, float* act_pos,
                       hipStream_t stream)
{
    hipLaunchKernelGGL(k_mcmc_noise, dim3(grid_256(P)), dim3(256), 0, stream, P, gain, k, x0, raw_opacity, raw_scale, raw_rotq, noise,
                       seed, step, raw_pos, act_pos);
}

void launch_mcmc_regularize(int64_t P, float add_opacity, float add_scale, float* d_opacity, float* d_scale, hipStream_t stream)
{
    hipLaunchKernelGGL(k_mcmc_regularize, dim3(grid_256(3 * P)), dim3(256), 0, stream, P, add_opacity, add_scale, d_opacity,
                       d_scale);
}

} // namespace lcgs
