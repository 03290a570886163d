// maps.hip -- depth and alpha maps of the last keep-state frame, and their backward (the contract is in
// include/lcgs_hip.h).  Neither map exists in the reference: its renderer composites colour only.
//
//   k_render_maps           one workgroup per 16x16 tile, wave k = the tile's 8x8 quadrant k (unit_px / unit_py), one pixel per
//                           lane, the renderer's tile schedule.  The KEPT per-tile list is walked front to back in rounds of 256,
//                           up to the tile's largest n_contrib: a lane stages one entry -- not fetched at all when the forward
//                           left it a zero strip-mask byte -- and every wave walks the set bits of its own strip's ballots,
//                           reading the entry back as wave-uniform LDS broadcasts.  A pixel takes entries up to its own
//                           n_contrib, so the forward's saturation test is not repeated (the saturating entry lies past it);
//                           power, alpha, the two skips and the T update are the forward's expressions operation for operation
//                           (-ffp-contract=off), which makes alpha = sum w and depth = sum fl(w v) the tests' binary32 CPU restatement's bit for bit.
//   k_render_maps_backward  the same geometry walked back to front like k_render_backward, with the two channels (v, dL/dD) and
//                           (1, dL/dA) folded into one per-entry scalar.  Seven per-pixel terms per entry (q dx, q dy, q dx dx,
//                           q dx dy, q dy dy, q, w dL/dD) are summed over the strip's 64 lanes -- four DPP butterfly steps inside
//                           each 16-lane row, then one LDS add per row -- and over the four waves in a per-round LDS
//                           accumulator; the round's totals leave as at most seven global float atomics per (tile, splat), eight
//                           consecutive lanes per splat row.  It ADDS to grads2d slots 0-5 and 9.
//   k_maps_depth_to_pos     one lane per on-screen row: dL/dpos += slot 9 x dv/dz x front.
// Thresholds are constants for the derivative, exactly as in backward.hip: the 0.99 cap passes nothing, a saturated pixel stops.
#include "kept_walk.hpp"

namespace lcgs
{
using namespace kept_walk;
namespace
{

__global__ void __launch_bounds__(256) k_render_maps(CamParams cp, const uint32_t* __restrict__ ranges,
                                                     const uint32_t* __restrict__ point_list,
                                                     const SplatRecord* __restrict__ recs,
                                                     const uint32_t* __restrict__ n_contrib,
                                                     const uint8_t* __restrict__ strip_masks,
                                                     const uint32_t* __restrict__ d_counts,
                                                     const uint32_t* __restrict__ tile_order, int mode,
                                                     float* __restrict__ depth_map, float* __restrict__ alpha_map)
{
    __shared__ float4             s_rows[2][256];
    __shared__ unsigned long long s_mask[4][4]; // [staging wave][strip]
    __shared__ uint32_t           s_max[4];

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t       tx, ty;
    if (!tile_of_slot(cp, tile_order, blockIdx.x, tx, ty)) return;
    const uint32_t tile = ty * cp.grid_x + tx;
    const uint32_t px = unit_px(tx, wave, lane), py = unit_py(ty, wave, lane);
    const bool     inside = (px < cp.width) && (py < cp.height);
    const size_t   pix    = (size_t)px + (size_t)cp.width * py;
    // a frame that drew nothing left n_contrib untouched: both maps are zero
    const bool     drawn = d_counts[1] != 0u;
    const uint32_t last  = (inside && drawn) ? n_contrib[pix] : 0u; // 1-based list position of the pixel's last contributor
    const uint32_t range_start = drawn ? ranges[2 * (size_t)tile + 0] : 0u;
    const uint32_t len         = drawn ? ranges[2 * (size_t)tile + 1] - range_start : 0u;
    const uint32_t hi          = tile_walk_length(last, len, s_max, lane, wave);
    const float    pxf = (float)px, pyf = (float)py;

    float T = 1.0f, A = 0.0f, D = 0.0f;
    for (uint32_t base = 0u; base < hi; base += 256u) {
        const uint32_t e = base + tid;
        uint32_t       kmask = 0u;
        StagedEntry    se;
        se.a = se.b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (e < hi) {
            kmask = strip_masks ? strip_masks[range_start + e] : 0xFu;
            if (kmask != 0u) se = stage_entry(recs, point_list[range_start + e], mode); // (a zero byte: not fetched)
        }
        __syncthreads(); // the previous round's readers are done with the slab and the masks
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned long long m = __ballot((kmask >> k) & 1u);
            if (lane == 0) s_mask[wave][k] = m;
        }
        if (kmask != 0u) {
            s_rows[0][tid] = se.a;
            s_rows[1][tid] = se.b;
        }
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
                const float4   ea = s_rows[0][idx];
                const float4   eb = s_rows[1][idx];
                // power = -0.5 (ca dx dx + cc dy dy) - cb dx dy, products left to right: render.hip's expression
                const float dx = ea.x - pxf, dy = ea.y - pyf;
                const float qx = (ea.z * dx) * dx, cross = eb.x * dx;
                const float qy = (ea.w * dy) * dy;
                const float half  = qx + qy;
                const float power = half - cross * dy;
                const bool  cand  = (base + idx < last) & !(power > 0.0f) & (power >= eb.y);
                if (__builtin_amdgcn_ballot_w64(cand) == 0ull) continue;
                const float alpha = __builtin_fminf(0.99f, eb.z * blend_exp(power));
                if (cand && !(alpha < 1.0f / 255.0f)) {
                    const float wgt = T * alpha;
                    A               = A + wgt;
                    D               = D + wgt * eb.w;
                    T               = T * (1.0f - alpha);
                }
            }
        }
    }
    if (inside) {
        if (depth_map) depth_map[pix] = D;
        if (alpha_map) alpha_map[pix] = A;
    }
}

// (five waves per SIMD asked for; see DESIGN.md 9 for what the build reports)
__global__ void __launch_bounds__(256) k_render_maps_backward(CamParams cp, const uint32_t* __restrict__ ranges,
                                                              const uint32_t* __restrict__ point_list,
                                                              const SplatRecord* __restrict__ recs,
                                                              const float* __restrict__ final_T,
                                                              const uint32_t* __restrict__ n_contrib,
                                                              const uint8_t* __restrict__ strip_masks,
                                                              const uint32_t* __restrict__ d_counts,
                                                              const uint32_t* __restrict__ tile_order, int mode,
                                                              const float* __restrict__ dL_ddepth,
                                                              const float* __restrict__ dL_dalpha,
                                                              float* __restrict__ grads2d)
{
    constexpr int                 kSums = 7;
    __shared__ float4             s_rows[2][256];
    __shared__ float              s_acc[kSums][256]; // the round's sums over the tile's pixels, per entry
    __shared__ uint32_t           s_vid[256];        // the entry's splat (dense id); ~0: nothing staged
    __shared__ unsigned long long s_mask[4][4];      // [staging wave][strip]
    __shared__ uint32_t           s_max[4];

    if (d_counts[1] == 0u) return; // nothing drawn: final_T / n_contrib are not this frame's, every gradient is zero
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t       tx, ty;
    if (!tile_of_slot(cp, tile_order, blockIdx.x, tx, ty)) return;
    const uint32_t tile = ty * cp.grid_x + tx;
    const uint32_t px = unit_px(tx, wave, lane), py = unit_py(ty, wave, lane);
    const bool     inside = (px < cp.width) && (py < cp.height);
    const size_t   pix    = (size_t)px + (size_t)cp.width * py;
    const float    pxf = (float)px, pyf = (float)py;

    const uint32_t last    = inside ? n_contrib[pix] : 0u;
    const float    T_final = inside ? final_T[pix] : 0.0f;
    const float    gd = (inside && dL_ddepth) ? dL_ddepth[pix] : 0.0f;
    const float    ga = (inside && dL_dalpha) ? dL_dalpha[pix] : 0.0f;
    const uint32_t range_start = ranges[2 * (size_t)tile + 0];
    uint32_t       hi = tile_walk_length(last, ranges[2 * (size_t)tile + 1] - range_start, s_max, lane, wave);

    // per-pixel recurrences, back to front (backward.hip): Qr = prod (1 - alpha) over the entries walked so far, over T_final;
    // Bd = (value composited behind the current splat) . dL/dpixel over the two channels -- nothing lies behind the last entry
    float          Qr = 1.0f / T_final, Bd = 0.0f;
    const uint32_t acc_base = (uint32_t)(uintptr_t)&s_acc[0][0]; // low half of a flat LDS address = LDS offset
    const bool     row_head = (lane & 15u) == 0u;

    while (hi > 0u) {
        const uint32_t lo = hi > 256u ? hi - 256u : 0u;
        const uint32_t e  = lo + tid;
        uint32_t       kmask = 0u, vid = 0xFFFFFFFFu;
        StagedEntry    se;
        se.a = se.b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (e < hi) {
            kmask = strip_masks ? strip_masks[range_start + e] : 0xFu;
            if (kmask != 0u) {
                vid = point_list[range_start + e];
                se  = stage_entry(recs, vid, mode);
            }
        }
        __syncthreads(); // the previous round is flushed
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned long long m = __ballot((kmask >> k) & 1u);
            if (lane == 0) s_mask[wave][k] = m;
        }
        s_rows[0][tid] = se.a;
        s_rows[1][tid] = se.b;
        s_vid[tid]     = vid;
#pragma unroll
        for (int g = 0; g < kSums; ++g) s_acc[g][tid] = 0.0f;
        __syncthreads();

        for (int w = 3; w >= 0; --w) {
            if (__builtin_amdgcn_ballot_w64(lo + (uint32_t)w * 64u < last) == 0ull) continue; // past every pixel of the strip
            unsigned long long m = s_mask[w][wave];
            m = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(m >> 32)) << 32) |
                (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m);
            while (m != 0ull) { // scalar loop control, highest position first
                const uint32_t l = 63u - (uint32_t)__builtin_clzll(m);
                m &= ~(1ull << l);
                const uint32_t idx = (uint32_t)w * 64u + l;
                const float4   ea = s_rows[0][idx];
                const float4   eb = s_rows[1][idx];
                // the forward's own expression and order: the same entries pass the same thresholds
                const float dx = ea.x - pxf, dy = ea.y - pyf;
                const float qx = (ea.z * dx) * dx, cross = eb.x * dx;
                const float qy = (ea.w * dy) * dy;
                const float half  = qx + qy;
                const float power = half - cross * dy;
                const bool  cand  = (lo + idx < last) & !(power > 0.0f) & (power >= eb.y);
                if (__builtin_amdgcn_ballot_w64(cand) == 0ull) continue;
                const float G     = blend_exp(power);
                const float oG    = eb.z * G;
                const float alpha = __builtin_fminf(0.99f, oG);
                const bool  valid = cand & !(alpha < 1.0f / 255.0f);
                const float a     = valid ? alpha : 0.0f;
                // T in front of this splat = T_final / prod (1 - a) over this entry and everything behind it
                Qr = Qr * (1.0f - a);
                const float Tn  = __builtin_amdgcn_rcpf(Qr);
                const float wgt = a * Tn;
                const float d   = __builtin_fmaf(eb.w, gd, ga) - Bd; // (value - what lies behind) . dL/dpixel
                const float dLa = d * Tn;
                Bd              = __builtin_fmaf(a, d, Bd);
                // the 0.99 cap passes no gradient; selected behind the product (G is arbitrary bits off the candidate lanes)
                const float q = (valid & (oG < 0.99f)) ? G * dLa : 0.0f; // dL/dopacity
                float       v[kSums];
                v[0] = q * dx;
                v[1] = q * dy;
                v[2] = v[0] * dx;
                v[3] = v[0] * dy;
                v[4] = v[1] * dy;
                v[5] = q;
                v[6] = wgt * gd; // dL/dvalue
#pragma unroll
                for (int g = 0; g < kSums; ++g) v[g] = row16_sum(v[g]);
                if (row_head) {
                    // (a raw ds_add_f32, as in backward.hip: the compiler would wrap atomicAdd in a per-lane scan loop)
                    const uint32_t addr = acc_base + idx * 4u;
#pragma unroll
                    for (int g = 0; g < kSums; ++g)
                        asm volatile("ds_add_f32 %0, %1 offset:%2" ::"v"(addr), "v"(v[g]), "n"(g * 256 * 4) : "memory");
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the raw LDS adds above have landed
        __syncthreads();
        // ---- flush the round: eight consecutive lanes own one entry's row (seven of them add), so a wave instruction covers
        // contiguous bytes of a few rows instead of 64 different rows
        for (uint32_t cidx = tid; cidx < 256u * 8u; cidx += 256u) {
            const uint32_t g = cidx & 7u, idx = cidx >> 3;
            const uint32_t v = s_vid[idx];
            if (g < (uint32_t)kSums && v != 0xFFFFFFFFu) {
                // sums -> gradients: d/dmean = -opacity conic (S q dx, S q dy), d/dconic = opacity (-1/2, -1, -1/2) (S q dx dx, ...)
                const float4 ea = s_rows[0][idx], eb = s_rows[1][idx];
                float        s  = s_acc[g][idx];
                if (g < 5u) {
                    if (g < 2u) {
                        const float ca = -2.0f * ea.z, cc = -2.0f * ea.w, s0 = s_acc[0][idx], s1 = s_acc[1][idx];
                        s = (g == 0u) ? -(ca * s0 + eb.x * s1) : -(cc * s1 + eb.x * s0);
                    } else {
                        s *= (g == 3u) ? -1.0f : -0.5f;
                    }
                    s *= eb.z;
                }
                if (s != 0.0f) atomicAdd(&grads2d[(size_t)v * kG2D + (g < 6u ? g : (uint32_t)kG2DValueSlot)], s);
            }
        }
        hi = lo;
    }
}

__global__ void __launch_bounds__(256) k_maps_depth_to_pos(CamParams cp, const uint32_t* __restrict__ vis_index,
                                                           const uint32_t* __restrict__ d_counts,
                                                           const SplatRecord* __restrict__ recs,
                                                           const float* __restrict__ grads2d, int mode,
                                                           float* __restrict__ dL_dpos)
{
    const uint32_t V = d_counts[0];
    for (uint32_t vid = blockIdx.x * 256u + threadIdx.x; vid < V; vid += gridDim.x * 256u) {
        const float gv = grads2d[(size_t)vid * kG2D + kG2DValueSlot];
        if (gv == 0.0f) continue;
        const float  z  = recs[vid].depth;
        const float  gz = mode == kDepthInvZ ? -gv / (z * z) : gv; // view z = front . pos + tz
        const size_t o  = 3 * (size_t)vis_index[vid];
        dL_dpos[o + 0] += gz * cp.front[0];
        dL_dpos[o + 1] += gz * cp.front[1];
        dL_dpos[o + 2] += gz * cp.front[2];
    }
}

} // namespace

void launch_render_maps(const CamParams& cp, const uint32_t* ranges, const uint32_t* point_list, const SplatRecord* recs,
                        const uint32_t* n_contrib, const uint8_t* strip_masks, const uint32_t* d_counts,
                        const uint32_t* tile_order, int mode, float* depth, float* alpha, hipStream_t stream)
{
    if (cp.grid_x * cp.grid_y == 0) return;
    hipLaunchKernelGGL(k_render_maps, dim3(maps_grid(cp, tile_order)), dim3(256), 0, stream, cp, ranges, point_list, recs,
                       n_contrib, strip_masks, d_counts, tile_order, mode, depth, alpha);
}

void launch_render_maps_backward(const CamParams& cp, const uint32_t* ranges, const uint32_t* point_list,
                                 const SplatRecord* recs, const float* final_T, const uint32_t* n_contrib,
                                 const uint8_t* strip_masks, const uint32_t* d_counts, const uint32_t* tile_order, int mode,
                                 const float* dL_ddepth, const float* dL_dalpha, float* grads2d, hipStream_t stream)
{
    if (cp.grid_x * cp.grid_y == 0) return;
    hipLaunchKernelGGL(k_render_maps_backward, dim3(maps_grid(cp, tile_order)), dim3(256), 0, stream, cp, ranges, point_list,
                       recs, final_T, n_contrib, strip_masks, d_counts, tile_order, mode, dL_ddepth, dL_dalpha, grads2d);
}

void launch_maps_depth_to_pos(int64_t v_hint, const CamParams& cp, const uint32_t* vis_index, const uint32_t* d_counts,
                              const SplatRecord* recs, const float* grads2d, int mode, float* dL_dpos, hipStream_t stream)
{
    hipLaunchKernelGGL(k_maps_depth_to_pos, dim3(grid_256(v_hint)), dim3(256), 0, stream, cp, vis_index, d_counts, recs,
                       grads2d, mode, dL_dpos);
}

} // namespace lcgs
