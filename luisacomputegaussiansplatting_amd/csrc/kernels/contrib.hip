// contrib.hip -- per-splat blend-weight statistics of the last keep-state frame, and the keep / drop rule on them (DESIGN.md 9;
// the contract is in include/lcgs_hip.h).  No reference counterpart: its renderer composites colour only.
//
//   k_contrib_zero     one lane per on-screen row: clears the row's slab slot {sum, max bits, count}.
//   k_contrib_walk     kept_walk.hpp's walk, front to back like k_render_maps (maps.hip): power and alpha are its restatement of
//                      the forward's and the T update is the forward's expression too (-ffp-contract=off) -- so w = T alpha is
//                      the weight the frame blended with, bit for bit.  What this kernel adds is its body and its flush:
//                      instead of per-pixel accumulators each entry is reduced over the PIXELS: the count is the popcount of
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
#include "kept_rows.hpp"
#include "kept_walk.hpp"

namespace lcgs
{
using namespace kept_walk;
namespace
{
constexpr int kSlot = 3; // words of a slab slot: the sum, the max's bits, the count

__global__ void __launch_bounds__(256) k_contrib_zero(const uint32_t* __restrict__ d_counts, uint32_t* __restrict__ slab)
{
    const int64_t n = (int64_t)d_counts[0] * kSlot;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) slab[i] = 0u;
}

__global__ void __launch_bounds__(256) k_contrib_walk(KeptFrame f, uint32_t* __restrict__ slab)
{
    __shared__ WalkShared s_walk;
    __shared__ uint32_t   s_acc[kSlot][256]; // the round's {sum, max bits, count} over the tile's pixels, per entry

    if (f.d_counts[1] == 0u) return; // nothing drawn: n_contrib is not this frame's, nothing was blended
    TileWalk t;
    if (!tile_prologue(f, s_walk, t)) return;
    const uint32_t acc_base = (uint32_t)(uintptr_t)&s_acc[0][0]; // low half of a flat LDS address = LDS offset
    const bool     row_head = (t.lane & 15u) == 0u;
    const uint32_t row_bit  = t.lane & 48u; // first bit of the lane's 16-lane row in a wave ballot

    float    T      = 1.0f;
    uint32_t my_vid = 0u; // the splat this lane staged for the round
    walk_rounds<false>(
        f, s_walk, t, kDepthZ, // (the value the walk stages is not used here)
        [&](uint32_t vid) {
            my_vid = vid;
#pragma unroll
            for (int g = 0; g < kSlot; ++g) s_acc[g][t.tid] = 0u;
        },
        [&](uint32_t idx, uint32_t pos, const float4& ea, const float4& eb) {
            const EntryEval v = eval_entry(ea, eb, t.pxf, t.pyf, pos, t.last);
            if (__builtin_amdgcn_ballot_w64(v.cand) == 0ull) return;
            const EntryBlend         b  = blend_entry(eb, v);
            const unsigned long long bl = __builtin_amdgcn_ballot_w64(b.blended);
            if (bl == 0ull) return; // nobody in the strip blends it
            const float wgt = b.blended ? T * b.alpha : 0.0f;
            if (b.blended) T = T * (1.0f - b.alpha);
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
        },
        [&] {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the raw LDS atomics above have landed
            __syncthreads();
            // ---- flush the round: the lane that staged an entry owns its slot
            const uint32_t cnt = s_acc[2][t.tid];
            if (cnt != 0u) {
                uint32_t* slot = slab + (size_t)my_vid * kSlot;
                atomicAdd(reinterpret_cast<float*>(slot), __uint_as_float(s_acc[0][t.tid]));
                atomicMax(slot + 1, s_acc[1][t.tid]);
                atomicAdd(slot + 2, cnt);
            }
        });
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

void launch_contrib_zero(const KeptRows& r, uint32_t* slab, hipStream_t stream)
{
    hipLaunchKernelGGL(k_contrib_zero, dim3(grid_256(r.hint * kSlot)), dim3(256), 0, stream, r.d_counts, slab);
}

void launch_contrib_walk(const KeptFrame& f, uint32_t* slab, hipStream_t stream)
{
    if (f.cp.grid_x * f.cp.grid_y == 0) return;
    hipLaunchKernelGGL(k_contrib_walk, dim3(maps_grid(f.cp, f.tile_order)), dim3(256), 0, stream, f, slab);
}

void launch_contrib_fold(const KeptRows& r, const uint32_t* slab, float* weight_sum, float* weight_max, uint32_t* pixels,
                         uint32_t* views, hipStream_t stream)
{
    hipLaunchKernelGGL(k_contrib_fold, dim3(grid_256(r.hint)), dim3(256), 0, stream, r.vis_index, r.d_counts, r.P, slab, weight_sum,
                       weight_max, pixels, views);
}

void launch_contrib_classify(int64_t P, const ContribRule& rule, const float* weight_sum, const float* weight_max,
                             const uint32_t* pixels, const uint32_t* views, uint32_t* emit, uint8_t* action, hipStream_t stream)
{
    hipLaunchKernelGGL(k_contrib_classify, dim3(grid_256(P)), dim3(256), 0, stream, P, rule, weight_sum, weight_max, pixels,
                       views, emit, action);
}

} // namespace lcgs
