// camera_grad.hip -- the gradient of the last backward's scalar with respect to the camera pose: twelve floats in the order of
// lcgs_camera's members (position, front, up, right; the contract is in include/lcgs_hip.h, the algebra in DESIGN.md 9).  The
// reference has no backward at all; this is the second consumer of the 2-D gradient rows a backward leaves in the context.
//
//   k_camera_grad         one lane per on-screen row (dense ids), 256-lane workgroups, grid-stride over FIXED blocks of 256
//                         rows.  The per-splat expressions are the preprocess-backward's own (splat_backward.hpp): the colour
//                         step's direction part of dL/dpos -- from the kept Jacobian (JAC) or from the coefficient rows staged
//                         through LDS as k_preprocess_backward stages them -- and geom_backward_t, which hands out dv, dT0, dT1
//                         and the four projection-Jacobian entries instead of dropping them.  Twelve doubles per lane, summed
//                         over the wave with a fixed butterfly of cross-lane moves, over the four waves through LDS in wave
//                         order; block b's twelve sums go to slab entry b with plain stores.
//   k_camera_grad_finish  one workgroup adds the slab entries in index order (21 interleaved runs per component, then the runs
//                         in order) and writes the twelve floats, each rounded once.  The entry count comes from d_counts[0].
// No atomics: the summation tree depends on the number of on-screen rows only -- not on the grid, the launch hint or timing --
// so the same 2-D rows give the same bits.
#include "kept_rows.hpp"
#include "kept_walk.hpp"
#include "splat_backward.hpp"

namespace lcgs
{
namespace
{
constexpr int kCamTerms = 12;
constexpr int kFinishRuns = 21; // 21 x 12 = 252 of the finish kernel's 256 lanes

__device__ __forceinline__ double wave_sum(double x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

template <bool JAC, bool AA>
__global__ void __launch_bounds__(256)
k_camera_grad(int sh_deg, CamParams cp, float scale_modifier, const float* __restrict__ pos, const float* __restrict__ scale,
              const float* __restrict__ rotq, const float* __restrict__ sh, const uint32_t* __restrict__ vis_index,
              const uint32_t* __restrict__ d_counts, const float* __restrict__ grads2d, const float4* __restrict__ shjac,
              const SplatRecord* __restrict__ recs, int depth_mode, double* __restrict__ slab, const float* __restrict__ opacity)
{
    __shared__ float4 s_sh[JAC ? 1 : 4][JAC ? 1 : 64 * 13]; // (the coefficient rows' slab: the SH-row path only)
    __shared__ double s_part[4][kCamTerms];
    const uint32_t V = d_counts[0];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int feat = (sh_deg + 1) * (sh_deg + 1);
    const bool staged = sh_deg == 3 && ((reinterpret_cast<uintptr_t>(sh) & 15) == 0);
    for (uint32_t blk = blockIdx.x; (uint64_t)blk * 256u < V; blk += gridDim.x) { // (no row at all: no pass, no V - 1)
        const RowBlock      b  = row_block(0u, V, blk, vis_index);
        const SplatOperands in = load_splat_operands<AA>(b.vsafe, b.idx, grads2d, pos, scale, rotq, opacity);
        float gdir[3] = { 0.0f, 0.0f, 0.0f };
        if constexpr (JAC) {
            const float4 j0 = shjac[(size_t)b.vsafe * 3 + 0], j1 = shjac[(size_t)b.vsafe * 3 + 1], j2 = shjac[(size_t)b.vsafe * 3 + 2];
            jac_colour_step<false>(cp, in, j0, j1, j2, nullptr, gdir);
        } else {
            // ---- stage the SH rows (coalesced), or fetch them lane-wise for other degrees, as k_preprocess_backward does
            float* row = reinterpret_cast<float*>(&s_sh[wave][lane * 13]);
            __syncthreads(); // the previous block's readers are done with the slab
            if (staged) {
#pragma unroll
                for (int i = 0; i < 12; ++i)
                    row_part_step(b, lane, i, [&](uint32_t slot, uint32_t part, int sidx) {
                        s_sh[wave][slot * 13u + part] = reinterpret_cast<const float4*>(sh + (size_t)sidx * 48)[part];
                    });
            } else if (b.valid) {
                const float* s = sh + (size_t)b.idx * feat * 3;
                for (int k = 0; k < 48; ++k) row[k] = k < feat * 3 ? s[k] : 0.0f;
            }
            __syncthreads();
            if (b.valid) sh_colour_step<false>(cp, in, feat, row, gdir);
        }
        double t[kCamTerms];
#pragma unroll
        for (int k = 0; k < kCamTerms; ++k) t[k] = 0.0;
        if (b.valid) {
            // the depth channel's dL/dvalue reaches view z directly (as in maps.hip k_maps_depth_to_pos)
            float gz = 0.0f;
            if (depth_mode >= 0) {
                const float gv = grads2d[(size_t)b.vid * kG2D + kG2DValueSlot];
                if (gv != 0.0f) gz = kept_walk::depth_value_backward(recs[b.vid].depth, depth_mode, gv);
            }
            camera_terms<AA>(cp, scale_modifier, in, gdir, gz, t);
        }
        // ---- the block's twelve sums: butterfly over the wave, then the four waves in order
#pragma unroll
        for (int k = 0; k < kCamTerms; ++k) t[k] = wave_sum(t[k]);
        __syncthreads(); // the previous block's s_part is read
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < kCamTerms; ++k) s_part[wave][k] = t[k];
        }
        __syncthreads();
        if (threadIdx.x < (unsigned)kCamTerms) {
            const int k = (int)threadIdx.x;
            slab[(size_t)blk * kCamTerms + k] = ((s_part[0][k] + s_part[1][k]) + s_part[2][k]) + s_part[3][k];
        }
    }
}

__global__ void __launch_bounds__(256) k_camera_grad_finish(const uint32_t* __restrict__ d_counts, const double* __restrict__ slab,
                                                            float* __restrict__ out)
{
    __shared__ double s_run[kFinishRuns][kCamTerms];
    const uint32_t V = d_counts[0];
    const uint32_t entries = V / 256u + ((V & 255u) ? 1u : 0u);
    const uint32_t t = threadIdx.x, run = t / (uint32_t)kCamTerms, k = t - run * (uint32_t)kCamTerms;
    if (run < (uint32_t)kFinishRuns) {
        double a = 0.0;
        for (uint32_t e = run; e < entries; e += (uint32_t)kFinishRuns) a += slab[(size_t)e * kCamTerms + k]; // (21 entries = 2016 contiguous bytes per step)
        s_run[run][k] = a;
    }
    __syncthreads();
    if (t < (uint32_t)kCamTerms) {
        double a = 0.0;
        for (int r = 0; r < kFinishRuns; ++r) a += s_run[r][t];
        out[t] = (float)a; // (a frame without on-screen rows: twelve zeros)
    }
}
} // namespace

size_t camera_grad_slab_bytes(int64_t P) { return (size_t)((P + 255) / 256) * kCamTerms * sizeof(double); }

void launch_camera_grad(const KeptRows& r, int depth_mode, double* slab, float* dL_dcam, hipStream_t stream)
{
    const unsigned blocks = grid_256(r.hint);
    // (one instantiation per raster mode, like the preprocess-backward's: the classic pass carries none of the other's code)
#define LCGS_LAUNCH_CAM(JAC_, AA_)                                                                                             \
    hipLaunchKernelGGL((k_camera_grad<JAC_, AA_>), dim3(blocks), dim3(256), 0, stream, r.sh_deg, r.cp, r.scale_modifier, r.pos,  \
                       r.scale, r.rotq, r.sh, r.vis_index, r.d_counts, r.grads2d, r.shjac, r.recs, depth_mode, slab, r.opacity)
    const bool jac = r.shjac && r.sh_deg == 3, aa = r.cp.raster_mode != 0;
    if (jac && aa) LCGS_LAUNCH_CAM(true, true);
    else if (jac) LCGS_LAUNCH_CAM(true, false);
    else if (aa) LCGS_LAUNCH_CAM(false, true);
    else LCGS_LAUNCH_CAM(false, false);
#undef LCGS_LAUNCH_CAM
    hipLaunchKernelGGL(k_camera_grad_finish, dim3(1), dim3(256), 0, stream, r.d_counts, slab, dL_dcam);
}

} // namespace lcgs
