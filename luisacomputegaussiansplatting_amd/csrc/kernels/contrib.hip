// contrib.hip -- per-splat blend-weight statistics of the last keep-state frame, and the keep / drop rule on them (DESIGN.md 9;
// the contract is in include/lcgs_hip.h).  No reference counterpart: its renderer composites colour only.
//
//   k_contrib_zero     one lane per on-screen row: clears the row's slab slot {sum, max bits, count}.
//   k_contrib_walk     k_render_maps' geometry and walk (maps.hip): one workgroup per 16x16 tile in the renderer's schedule, wave k
//                      = the tile's 8x8 quadrant k, the KEPT list walked front to back in rounds of 256 staged entries, strip-mask
//                      ballots, entries read back as wave-uniform LDS broadcasts, power / alpha / T the forward's expressions
//                      operation for operation (-ffp-contract=off) -- so w = T alpha is the weight the frame blended with, bit for
//                      bit.  Instead of per-pixel accumulators each entry is reduced over the PIXELS: the count is the popcount of
//                      the wave's ballot of "blended" (an entry nobody blends costs nothing more), the sum and the max take four
//                      DPP butterfly steps inside each 16-lane row and then one LDS add / LDS max per row into the entry's slot of
//                      a per-round accumulator (the max on the float's bits: non-negative floats order as their bit patterns).
//                      The lane that staged an entry flushes it: a count that is not zero leaves as three global atomics
//                      into the slab slot of the entry's on-screen row.
//   k_contrib_fold     one lane per on-screen row, no atomics (the shape of k_densify_stats): the slab slot is folded into the
//                      caller's arrays at vis_index[row]; NULL members are skipped; this is where `views` counts.
//   k_contrib_classify one lane per row: keep = every enabled minimum is met; writes lcgs_densify's action (0 prune, 1 keep) and,
//                      for the rewrite, its emit count.
// The max and the counts do not depend on the order of the atomics; the sum is a binary32 sum of non-negative terms in an order
// that differs from run to run.
#include "kept_walk.hpp"

namespace lcgs
{
using namespace kept_walk;
namespace
{
// row16_sum's butterfly with max, on unsigned bits
__device__ __forceinline__ uint32_t row16_max(uint32_t x)
{
#define LCGS_DPP_MAX(CTRL)                                                                     \
    {                                                                                          \
        const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, true); \
        x                = o > x ? o : x;                                                      \
    }
    LCGS_DPP_MAX(0xB1);  // quad_perm:[1,0,3,2]
    LCGS_DPP_MAX(0x4E);  // quad_perm:[2,3,0,1]
    LCGS_DPP_MAX(0x141); // row_half_mirror
    LCGS_DPP_MAX(0x140); // row_mirror
#undef LCGS_DPP_MAX
    return x;
}

constexpr int kSlot = 3; // words of a slab slot: the sum, the max's bits, the count

__global__ void __launch_bounds__(256) k_contrib_zero(const uint32_t* __restrict__ d_counts, uint32_t* __restrict__ slab)
{
    const int64_t n = (int64_t)d_counts[0] * kSlot;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) slab[i] = 0u;
}

__global__ void __launch_bounds__(256) k_contrib_walk(CamParams cp, const uint32_t* __restrict__ ranges,
                                                      const uint32_t* __restrict__ point_list,
                                                      const SplatRecord* __restrict__ recs,
                                                      const uint32_t* __restrict__ n_contrib,
                                                      const uint8_t* __restrict__ strip_masks,
                                                      const uint32_t* __restrict__ d_counts,
                                                      const uint32_t* __restrict__ tile_order, uint32_t* __restrict__ slab)
{
    __shared__ float4             s_rows[2][256];
    __shared__ uint32_t           s_acc[kSlot][256]; // the round's {sum, max bits, count} over the tile's pixels, per entry
    __shared__ unsigned long long s_mask[4][4];      // [staging wave][strip]
    __shared__ uint32_t           s_max[4];

    if (d_counts[1] == 0u) return; // nothing drawn: n_contrib is not this frame's, nothing was blended
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t       tx, ty;
    if (!tile_of_slot(cp, tile_order, blockIdx.x, tx, ty)) return;
    const uint32_t tile = ty * cp.grid_x + tx;
    const uint32_t px = unit_px(tx, wave, lane), py = unit_py(ty, wave, lane);
    const bool     inside = (px < cp.width) && (py < cp.height);
    const uint32_t last = inside ? n_contrib[(size_t)px + (size_t)cp.width * py] : 0u; // 1-based position of the last contributor
    const uint32_t range_start = ranges[2 * (size_t)tile + 0];
    const uint32_t hi = tile_walk_length(last, ranges[2 * (size_t)tile + 1] - range_start, s_max, lane, wave);
    const float    pxf = (float)px, pyf = (float)py;

    const uint32_t acc_base = (uint32_t)(uintptr_t)&s_acc[0][0]; // low half of a flat LDS address = LDS offset
    const bool     row_head = (lane & 15u) == 0u;
    const uint32_t row_bit  = lane & 48u; // first bit of the lane's 16-lane row in a wave ballot

    float T = 1.0f;
    for (uint32_t base = 0u; base < hi; base += 256u) {
        const uint32_t e = base + tid;
        uint32_t       kmask = 0u, vid = 0u;
        StagedEntry    se;
        se.a = se.b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (e < hi) {
            kmask = strip_masks ? strip_masks[range_start + e] : 0xFu;
            if (kmask != 0u) { // (a zero byte: not fetched)
                vid = point_list[range_start + e];
                se  = stage_entry(recs, vid, kDepthZ); // (the value it stages is not used here)
            }
        }
        __syncthreads(); // the previous round's readers are done with the slab and the masks
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned long long m = __ballot((kmask >> k) & 1u);
            if (lane == 0) s_mask[wave][k] = m;
        }
        s_rows[0][tid] = se.a;
        s_rows[1][tid] = se.b;
#pragma unroll
        for (int g = 0; g < kSlot; ++g) s_acc[g][tid] = 0u;
        __syncthreads();
        for (uint32_t w = 0; w < 4u; ++w) {
            if (__builtin_amdgcn_ballot_w64(base + w * 64u < last) == 0ull) break; // past every pixel of the strip
            unsigned long long m = s_mask[w][wave];
            m = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(m >> 32)) << 32) |
                (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m);
            while (m != 0ull) { // scalar loop control, lowest position first
                const uint32_t l = (uint32_t)__ffsll((long long)m) - 1u;
                m &= m - 1ull;
                const uint32_t idx = w * 64u + l;
                const float4   a = s_rows[0][idx];
                const float4   b = s_rows[1][idx];
                // power = -0.5 (ca dx dx + cc dy dy) - cb dx dy, products left to right: render.hip's expression
                const float dx = a.x - pxf, dy = a.y - pyf;
                const float qx = (a.z * dx) * dx, cross = b.x * dx;
                const float qy = (a.w * dy) * dy;
                const float half  = qx + qy;
                const float power = half - cross * dy;
                const bool  cand  = (base + idx < last) & !(power > 0.0f) & (power >= b.y);
                if (__builtin_amdgcn_ballot_w64(cand) == 0ull) continue;
                const float alpha   = __builtin_fminf(0.99f, b.z * blend_exp(power));
                const bool  blended = cand && !(alpha < 1.0f / 255.0f);
                const unsigned long long bl = __builtin_amdgcn_ballot_w64(blended);
                if (bl == 0ull) continue; // nobody in the strip blends it
                const float wgt = blended ? T * alpha : 0.0f;
                if (blended) T = T * (1.0f - alpha);
                const float    rsum = row16_sum(wgt);
                const uint32_t rmax = row16_max(__float_as_uint(wgt));
                if (row_head) {
                    // (raw LDS atomics, as in maps.hip / backward.hip: the compiler would wrap atomicAdd in a per-lane scan loop)
                    const uint32_t addr = acc_base + idx * 4u;
                    const uint32_t rcnt = (uint32_t)__popc((uint32_t)(bl >> row_bit) & 0xFFFFu);
                    asm volatile("ds_add_f32 %0, %1" ::"v"(addr), "v"(rsum) : "memory");
                    asm volatile("ds_max_u32 %0, %1 offset:1024" ::"v"(addr), "v"(rmax) : "memory");
                    asm volatile("ds_add_u32 %0, %1 offset:2048" ::"v"(addr), "v"(rcnt) : "memory");
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the raw LDS atomics above have landed
        __syncthreads();
        // ---- flush the round: the lane that staged an entry owns its slot
        const uint32_t cnt = s_acc[2][tid];
        if (cnt != 0u) {
            uint32_t* slot = slab + (size_t)vid * kSlot;
            atomicAdd(reinterpret_cast<float*>(slot), __uint_as_float(s_acc[0][tid]));
            atomicMax(slot + 1, s_acc[1][tid]);
            atomicAdd(slot + 2, cnt);
        }
    }
}

__global__ void __launch_bounds__(256) k_contrib_fold(const uint32_t* __restrict__ vis_index, const uint32_t* __restrict__ d_counts,
                                                      int64_t P, const uint32_t* __restrict__ slab, float* __restrict__ weight_sum,
                                                      float* __restrict__ weight_max, uint32_t* __restrict__ pixels,
                                                      uint32_t* __restrict__ views)
{
    const int64_t V = (int64_t)d_counts[0];
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < V; r += (int64_t)gridDim.x * 256) {
        const uint32_t cnt = slab[r * kSlot + 2];
        if (cnt == 0u) continue; // no pixel blended the row: untouched
        const int64_t i = (int64_t)vis_index[r];
        if (i >= P) continue;
        if (weight_sum) weight_sum[i] += __uint_as_float(slab[r * kSlot + 0]);
        if (weight_max) weight_max[i] = fmaxf(weight_max[i], __uint_as_float(slab[r * kSlot + 1]));
        if (pixels) pixels[i] += cnt;
        if (views) views[i] += 1u;
    }
}

__global__ void __launch_bounds__(256) k_contrib_classify(int64_t P, ContribRule rule, const float* __restrict__ weight_sum,
                                                          const float* __restrict__ weight_max,
                                                          const uint32_t* __restrict__ pixels, const uint32_t* __restrict__ views,
                                                          uint32_t* __restrict__ emit, uint8_t* __restrict__ action)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < P; i += (int64_t)gridDim.x * 256) {
        bool keep = true;
        if (rule.min_weight_max != 0.0f) keep &= weight_max[i] >= rule.min_weight_max;
        if (rule.min_weight_sum != 0.0f) keep &= weight_sum[i] >= rule.min_weight_sum;
        if (rule.min_pixels != 0u) keep &= (uint64_t)pixels[i] >= rule.min_pixels;
        if (rule.min_views != 0u) keep &= (uint64_t)views[i] >= rule.min_views;
        action[i] = keep ? 1 : 0;
        if (emit) emit[i] = keep ? 1u : 0u;
    }
}
} // namespace

size_t contrib_slab_bytes(int64_t rows) { return (size_t)std::max<int64_t>(rows, 1) * kSlot * sizeof(uint32_t); }

void launch_contrib_zero(int64_t v_hint, const uint32_t* d_counts, uint32_t* slab, hipStream_t stream)
{
    hipLaunchKernelGGL(k_contrib_zero, dim3(grid_256(std::max<int64_t>(v_hint, 1) * kSlot)), dim3(256), 0, stream, d_counts, slab);
}

void launch_contrib_walk(const CamParams& cp, const uint32_t* ranges, const uint32_t* point_list, const SplatRecord* recs,
                         const uint32_t* n_contrib, const uint8_t* strip_masks, const uint32_t* d_counts,
                         const uint32_t* tile_order, uint32_t* slab, hipStream_t stream)
{
    if (cp.grid_x * cp.grid_y == 0) return;
    hipLaunchKernelGGL(k_contrib_walk, dim3(maps_grid(cp, tile_order)), dim3(256), 0, stream, cp, ranges, point_list, recs, n_contrib, strip_masks,
                       d_counts, tile_order, slab);
}

void launch_contrib_fold(int64_t v_hint, int64_t P, const uint32_t* vis_index, const uint32_t* d_counts, const uint32_t* slab,
                         float* weight_sum, float* weight_max, uint32_t* pixels, uint32_t* views, hipStream_t stream)
{
    hipLaunchKernelGGL(k_contrib_fold, dim3(grid_256(std::max<int64_t>(v_hint, 1))), dim3(256), 0, stream, vis_index, d_counts, P,
                       slab, weight_sum, weight_max, pixels, views);
}

void launch_contrib_classify(int64_t P, const ContribRule& rule, const float* weight_sum, const float* weight_max,
                             const uint32_t* pixels, const uint32_t* views, uint32_t* emit, uint8_t* action, hipStream_t stream)
{
    hipLaunchKernelGGL(k_contrib_classify, dim3(grid_256(P)), dim3(256), 0, stream, P, rule, weight_sum, weight_max, pixels,
                       views, emit, action);
}

} // namespace lcgs
