// absgrad.hip -- AbsGS densification statistics of the last keep-state frame (the contract is in
// include/lcgs_hip.h): per on-screen row the sum over PIXELS of the absolute per-pixel gradient of the pixel-space mean,
//     a_i = ( sum_p |g_x(p, i)| , sum_p |g_y(p, i)| ),
// of L = <dL_dimg, img> + <dL_ddepth, depth> + <dL_dalpha, alpha>.  No reference counterpart.  The render-backward and the
// maps-backward form dL/dmean from per-(tile, splat) sums of q dx, q dy at their flush: the per-pixel gradients exist only inside a
// walk, so this is one more walk of the kept lists (kept_walk.hpp) with its own accumulators and flush.
//
//   k_absgrad_zero   one lane per float of the workspace (two per on-screen row, count on the device): clears it.
//   k_absgrad_walk   back to front like k_render_maps_backward (maps.hip), with its recurrences: Qr = prod (1 - alpha) over
//                    T_final, Tn = rcp(Qr), ONE carried Bd = (what lies behind the entry) . dL/dpixel over all the channels --
//                    it starts at bg . dL_dimg[p] (the frame's background is the last colour layer; nothing lies behind the map
//                    channels).  The per-entry scalar is colour_i . dL_dimg[p] + value_i dL_ddepth[p] + dL_dalpha[p]: the channels
//                    are summed per pixel FIRST.  From q = G dL/dalpha (0 under the 0.99 cap or when not blended) the lane
//                    forms the two components of its pixel's mean gradient over the opacity,
//                        ca (q dx) + cb (q dy),   cc (q dy) + cb (q dx)
//                    (their sign does not matter) BEFORE any reduction, takes fabs, THEN sums over the strip: four DPP butterfly
//                    steps inside each 16-lane row, one raw LDS add per row into the round's accumulator.  The opacity is
//                    non-negative and entry-uniform: it is applied once per entry at the flush.  The conic terms are not -- they
//                    mix the two signed sums -- so they are applied per pixel.
//                    The flush: two consecutive lanes own one entry's two sums and add them to the entry's workspace slot, so
//                    a wave instruction covers 8-byte segments instead of 64 single floats (the slot is all a row has here).
//                    COL: dL_dimg is given -- the entry's colour is staged in the `before` hook next to the walk's own rows;
//                    MAP: dL_ddepth or dL_dalpha is.  The maps-only variant stages no colour.
//   k_absgrad_rows   one lane per on-screen row, no atomics: the workspace slot goes to the caller's arrays at vis_index[row] --
//                    d_absgrad += (a_x, a_y); grad_accum += |(a_x W/2, a_y H/2)|, denom and max_radii as k_densify_stats does
//                    (densify_row.hpp: the same code).
// Thresholds are constants for the derivative, exactly as in backward.hip: the 0.99 cap passes nothing, a saturated pixel stops.
// The sums are binary32 sums of non-negative terms in an order that differs from run to run (float atomics across tiles).
#include "densify_row.hpp"
#include "kept_rows.hpp"
#include "kept_walk.hpp"

namespace lcgs
{
using namespace kept_walk;
namespace
{

__global__ void __launch_bounds__(256) k_absgrad_zero(const uint32_t* __restrict__ d_counts, float* __restrict__ ws)
{
    const int64_t n = (int64_t)d_counts[0] * 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) ws[i] = 0.0f;
}

template <bool COL, bool MAP>
__global__ void __launch_bounds__(256) k_absgrad_walk(KeptFrame f, int mode, float bg0, float bg1, float bg2,
                                                      const float* __restrict__ dL_dimg, const float* __restrict__ dL_ddepth,
                                                      const float* __restrict__ dL_dalpha, float* __restrict__ ws)
{
    __shared__ WalkShared s_walk;
    __shared__ float      s_acc[2][256];        // the round's two sums over the tile's pixels, per entry
    __shared__ uint32_t   s_vid[256];           // the entry's splat (dense id); ~0: nothing staged
    __shared__ float4     s_col[COL ? 256 : 1]; // COL: the entry's colour

    if (f.d_counts[1] == 0u) return; // nothing drawn: final_T / n_contrib are not this frame's, every gradient is zero
    TileWalk t;
    if (!tile_prologue(f, s_walk, t)) return;
    const float T_final = t.inside ? f.final_T[t.pix] : 0.0f;
    float       dpr = 0.0f, dpg = 0.0f, dpb = 0.0f, gd = 0.0f, ga = 0.0f;
    if constexpr (COL) {
        if (t.inside) {
            const size_t plane = (size_t)f.cp.width * f.cp.height;
            dpr = dL_dimg[t.pix], dpg = dL_dimg[plane + t.pix], dpb = dL_dimg[2 * plane + t.pix];
        }
    }
    if constexpr (MAP) {
        gd = (t.inside && dL_ddepth) ? dL_ddepth[t.pix] : 0.0f;
        ga = (t.inside && dL_dalpha) ? dL_dalpha[t.pix] : 0.0f;
    }

    // per-pixel recurrences, back to front (backward.hip, maps.hip): Qr = prod (1 - alpha) over the entries walked so far, over
    // T_final; Bd = (what is composited behind the current splat) . dL/dpixel -- the background behind the colour channels only
    float          Qr = 1.0f / T_final, Bd = __builtin_fmaf(bg0, dpr, __builtin_fmaf(bg1, dpg, bg2 * dpb));
    const uint32_t acc_base = (uint32_t)(uintptr_t)&s_acc[0][0]; // low half of a flat LDS address = LDS offset
    const bool     row_head = (t.lane & 15u) == 0u;

    walk_rounds<true>(
        f, s_walk, t, mode,
        [&](uint32_t vid) {
            s_vid[t.tid]    = vid;
            s_acc[0][t.tid] = 0.0f;
            s_acc[1][t.tid] = 0.0f;
            if constexpr (COL) {
                if (vid != 0xFFFFFFFFu) {
                    const SplatRecord* r = f.recs + vid;
                    s_col[t.tid]         = make_float4(r->r, r->g, r->b, 0.0f);
                }
            }
        },
        [&](uint32_t idx, uint32_t pos, const float4& ea, const float4& eb) {
            const EntryEval v = eval_entry(ea, eb, t.pxf, t.pyf, pos, t.last);
            if (__builtin_amdgcn_ballot_w64(v.cand) == 0ull) return;
            const EntryBlend b = blend_entry(eb, v);
            const float      a = b.blended ? b.alpha : 0.0f; // (carried as a zero, not skipped: the sums below are over the strip)
            // T in front of this splat = T_final / prod (1 - a) over this entry and everything behind it
            Qr = Qr * (1.0f - a);
            const float Tn  = __builtin_amdgcn_rcpf(Qr);
            float       val = 0.0f; // (colour, value, 1) . dL/dpixel: the channels are summed per pixel first
            if constexpr (MAP) val = __builtin_fmaf(eb.w, gd, ga);
            if constexpr (COL) {
                const float4 c = s_col[idx];
                val            = val + __builtin_fmaf(c.x, dpr, __builtin_fmaf(c.y, dpg, c.z * dpb));
            }
            const float d   = val - Bd; // (entry - what lies behind) . dL/dpixel
            const float dLa = d * Tn;
            Bd              = __builtin_fmaf(a, d, Bd);
            // the 0.99 cap passes no gradient; selected behind the product (G is arbitrary bits off the candidate lanes)
            const float q = (b.blended & (b.oG < 0.99f)) ? b.G * dLa : 0.0f; // dL/dopacity of this pixel
            // this pixel's d/dmean over the opacity: conic . (q dx, q dy) -- formed per pixel, THEN the absolute value
            const float qx = q * v.dx, qy = q * v.dy;
            const float ca = -2.0f * ea.z, cc = -2.0f * ea.w;
            float       sx = __builtin_fabsf(ca * qx + eb.x * qy);
            float       sy = __builtin_fabsf(cc * qy + eb.x * qx);
            sx             = row16_sum(sx);
            sy             = row16_sum(sy);
            if (row_head) {
                // (a raw ds_add_f32, as in maps.hip / backward.hip: the compiler would wrap atomicAdd in a per-lane scan loop)
                const uint32_t addr = acc_base + idx * 4u;
                asm volatile("ds_add_f32 %0, %1" ::"v"(addr), "v"(sx) : "memory");
                asm volatile("ds_add_f32 %0, %1 offset:1024" ::"v"(addr), "v"(sy) : "memory");
            }
        },
        [&] {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the raw LDS adds above have landed
            __syncthreads();
            // ---- flush the round: two consecutive lanes own one entry's slot, so a wave instruction covers whole 8-byte slots
            for (uint32_t cidx = t.tid; cidx < 512u; cidx += 256u) {
                const uint32_t g = cidx & 1u, idx = cidx >> 1;
                const uint32_t vid = s_vid[idx];
                if (vid == 0xFFFFFFFFu) continue;
                const float s = s_acc[g][idx] * s_walk.s_rows[1][idx].z; // x the opacity: non-negative, entry-uniform
                if (s != 0.0f) atomicAdd(&ws[(size_t)vid * 2u + g], s);
            }
        });
}

__global__ void __launch_bounds__(256) k_absgrad_rows(const uint32_t* __restrict__ vis_index, const uint32_t* __restrict__ d_counts,
                                                      int64_t P, CamParams cp, float scale_modifier,
                                                      const float* __restrict__ pos, const float* __restrict__ scale,
                                                      const float* __restrict__ rotq, const float* __restrict__ ws,
                                                      float* __restrict__ absgrad, float* __restrict__ grad_accum,
                                                      uint32_t* __restrict__ denom, int32_t* __restrict__ max_radii)
{
    const int64_t V  = (int64_t)d_counts[0];
    const float   hw = 0.5f * (float)cp.width, hh = 0.5f * (float)cp.height;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < V; r += (int64_t)gridDim.x * 256) {
        const int64_t i = (int64_t)vis_index[r];
        if (i >= P) continue;
        const float ax = ws[2 * r + 0], ay = ws[2 * r + 1];
        if (absgrad) {
            absgrad[2 * i + 0] += ax;
            absgrad[2 * i + 1] += ay;
        }
        if (grad_accum) { // (the three statistics come together or not at all)
            const float gx = ax * hw, gy = ay * hh;
            grad_accum[i] += sqrtf(gx * gx + gy * gy);
            densify_count_row(cp, scale_modifier, pos, scale, rotq, i, denom, max_radii);
        }
    }
}

} // namespace

size_t absgrad_ws_bytes(int64_t rows) { return (size_t)(rows > 1 ? rows : 1) * 2 * sizeof(float); }

void launch_absgrad_zero(const KeptRows& r, float* ws, hipStream_t stream)
{
    hipLaunchKernelGGL(k_absgrad_zero, dim3(grid_256(r.hint * 2)), dim3(256), 0, stream, r.d_counts, ws);
}

void launch_absgrad_walk(const KeptFrame& f, int mode, const float bg[3], const float* dL_dimg, const float* dL_ddepth,
                         const float* dL_dalpha, float* ws, hipStream_t stream)
{
    if (f.cp.grid_x * f.cp.grid_y == 0) return;
    const dim3 grid(maps_grid(f.cp, f.tile_order));
    const bool maps = dL_ddepth || dL_dalpha;
    if (dL_dimg && maps)
        hipLaunchKernelGGL((k_absgrad_walk<true, true>), grid, dim3(256), 0, stream, f, mode, bg[0], bg[1], bg[2], dL_dimg, dL_ddepth,
                           dL_dalpha, ws);
    else if (dL_dimg)
        hipLaunchKernelGGL((k_absgrad_walk<true, false>), grid, dim3(256), 0, stream, f, mode, bg[0], bg[1], bg[2], dL_dimg, nullptr,
                           nullptr, ws);
    else if (maps) // (no colour staged, no background)
        hipLaunchKernelGGL((k_absgrad_walk<false, true>), grid, dim3(256), 0, stream, f, mode, 0.0f, 0.0f, 0.0f, nullptr, dL_ddepth,
                           dL_dalpha, ws);
}

void launch_absgrad_rows(const KeptRows& r, const float* ws, float* absgrad, float* grad_accum, uint32_t* denom, int32_t* max_radii,
                         hipStream_t stream)
{
    hipLaunchKernelGGL(k_absgrad_rows, dim3(grid_256(r.hint)), dim3(256), 0, stream, r.vis_index, r.d_counts, r.P, r.cp,
                       r.scale_modifier, r.pos, r.scale, r.rotq, ws, absgrad, grad_accum, denom, max_radii);
}

} // namespace lcgs
