// backward.hip -- the backward of the fused forward frame.  The reference has no backward (README.md:70: "only
// forward code"); its only backward artefacts are the unused per-band dL/dSH helpers of
// lcgs/include/lcgs/util/sh.hpp:37-40,53-65,87-117,141-165.  What is differentiated here is exactly the forward of
// render.hip / gs_math.hpp (= gs_tile_splatter/shader.cpp:171-288, gs_projector/shader.cpp:82-158,
// sh_preprocessor.cpp:27-157); the specification is DESIGN.md "Backward" (SURVEY Appendix B).
//
//   k_render_backward      one workgroup per tile, wave k = "strip" k (the tile's 8x8 quadrant k, 16x4 strip k until round 5;
//                          unit_px / unit_py in tile_common.hpp), one pixel per lane (same geometry as the
//                          forward renderer).  The tile list is walked BACK TO FRONT in rounds of 256 entries; per
//                          round a wave lists the entries the forward BLENDED in its strip and walks that list four
//                          entries at a time with no data-dependent branch: six per-pixel terms per entry (the sums'
//                          algebra: see reduce_quad_and_add) go through two permlane-swap folds, become the nine sums
//                          w.r.t. {pixel mean, conic, opacity, rgb} behind them, are finished with DPP row shifts and
//                          added to a per-round LDS accumulator; after the round 16 lanes per entry flush the
//                          workgroup's totals with global float atomics -- 9 atomics per (tile, splat) instead of per
//                          (pixel, splat).  VALU-bound: DESIGN.md 5, profiles/r05_bwd_list_walk_ab.txt.
//   k_preprocess_backward  one lane per surviving splat: 2-D gradients -> dL/d{pos, scale, rotq, sh, opacity};
//                          the 192-byte SH gradient rows leave through LDS as coalesced 16-byte stores.
// Thresholds are constants for the derivative: near cull, alpha < 1/255 skip, T < 1e-4 stop and power > 0 gate the
// sums; the 0.99 alpha cap, the colour clamp and a saturated cam_clamp axis pass no gradient.
#include "adam_rows.hpp"
#include "kept_rows.hpp"
#include "kept_walk.hpp"
#include "splat_backward.hpp"
#include "stream_access.hpp"
#include "tile_common.hpp"

namespace lcgs
{

namespace
{
using namespace tile; // tile_of_workgroup / render_grid_size / splat_strip_mask: shared with render.hip

// ---------------------------------------------------------------------------------------------------------------
// Wave reduction of the per-pixel gradient terms, four list entries at a time.
// Every entry yields per-lane values that must be summed over the 64 pixels of the strip.  Reducing each entry on its
// own costs 6 cross-lane adds per value; instead the sums of FOUR entries (A, B, C, D) are folded together so that
// each cross-lane step works on registers that are full of useful data (costs from tools/microbench/issue_rates):
//   1. v_permlane32_swap + add on (A, B): lanes 0-31 now hold A summed over lane pairs (l, l+32), lanes 32-63 hold B;
//      the same on (C, D)                                                   2 x N x (8.1 + 2.3) cycles
//   2. v_permlane16_swap + add on (AB, CD): the four 16-lane rows hold A, C, B, D, each summed over rows   N x 10.4
//   3. four DPP row-shift adds: lane 15 of every row holds that entry's total                               9 x 4 x 4.2
// and one LDS add instruction per value and FOUR entries (lanes 15, 31, 47 and 63, each to its own entry's accumulator
// row) instead of one per value and entry.  N = 6 values go through steps 1-2, nine through step 3 (reduce_quad_and_add).
// ---------------------------------------------------------------------------------------------------------------
// (inline asm rather than __builtin_amdgcn_permlane32_swap: the builtin returns fresh values, and the compiler copies
// both operands first -- two extra moves per swap; x and y are dead after the call, the swap may clobber them.  The
// s_nop covers the 2-wait-state VALU-write -> permlane-read hazard, which nothing pads inside asm.)
template <int N>
__device__ __forceinline__ void swap32_add(float x[N], float y[N], float out[N])
{
#pragma unroll
    for (int g = 0; g < N; ++g) {
        // lanes 0-31: x = own x, y = partner's x;  lanes 32-63: x = partner's y, y = own y
        asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(x[g]), "+v"(y[g]));
        out[g] = x[g] + y[g];
    }
}
template <int N>
__device__ __forceinline__ void swap16_add(float x[N], float y[N], float out[N])
{
#pragma unroll
    for (int g = 0; g < N; ++g) {
        // rows 1 and 3 of x trade places with rows 0 and 2 of y: after the add the rows hold x.lo, y.lo, x.hi, y.hi
        asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(x[g]), "+v"(y[g]));
        out[g] = x[g] + y[g];
    }
}
// sums over each 16-lane row, result in lane 15 of the row.  The nine chains advance in lockstep, one DPP step each
// per round, so the 2-wait-state VALU-write -> DPP-read hazard of a chain is covered by the eight other chains'
// instructions (hipcc pads nothing inside asm; the leading s_nop covers the producers of v[]).
__device__ __forceinline__ void row_sum9_to_lane15(float v[9])
{
    asm volatile("s_nop 1" ::: "memory");
#define LCGS_DPP_STEP(ctrl)                                                                                         \
    asm volatile("v_add_f32_dpp %0, %0, %0 " ctrl "\n\t"                                                             \
                 "v_add_f32_dpp %1, %1, %1 " ctrl "\n\t"                                                             \
                 "v_add_f32_dpp %2, %2, %2 " ctrl "\n\t"                                                             \
                 "v_add_f32_dpp %3, %3, %3 " ctrl "\n\t"                                                             \
                 "v_add_f32_dpp %4, %4, %4 " ctrl "\n\t"                                                             \
                 "v_add_f32_dpp %5, %5, %5 " ctrl "\n\t"                                                             \
                 "v_add_f32_dpp %6, %6, %6 " ctrl "\n\t"                                                             \
                 "v_add_f32_dpp %7, %7, %7 " ctrl "\n\t"                                                             \
                 "v_add_f32_dpp %8, %8, %8 " ctrl                                                                    \
                 : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]),   \
                   "+v"(v[8]))
    LCGS_DPP_STEP("row_shr:1 row_mask:0xf bank_mask:0xf");
    LCGS_DPP_STEP("row_shr:2 row_mask:0xf bank_mask:0xf");
    LCGS_DPP_STEP("row_shr:4 row_mask:0xf bank_mask:0xe");
    LCGS_DPP_STEP("row_shr:8 row_mask:0xf bank_mask:0xc"); // lane 15 of each row holds the row sum
#undef LCGS_DPP_STEP
    asm volatile("s_nop 1" ::: "memory");
}

// Steps 2 and 3 on (AB, CD) and the LDS adds.  rows: lanes 15 / 31 / 47 / 63 hold the LDS byte address of the
// accumulator row (&s_grad[0][idx]) of entry A / C / B / D; value g goes to row + g * 1028 (kRows floats).
// The five geometry sums separate: with q = dL/dopacity per pixel (G dL/dG = opacity x q, the opacity applied at the flush), dx depends
// on the pixel's COLUMN only, and steps 1-2 sum over the strip's four rows of one column, so only (q, q dy, q dy dy) go through
// them; behind step 2 a lane holds those three summed over its column for the entry of its 16-lane row, multiplies by THAT entry's
// dx (dx_row) and step 3 sums the products over the columns:
//   S hx = S_c dx (S_r q)   S hx dx = S_c dx dx (S_r q)   S hx dy = S_c dx (S_r q dy)   S hy = S_c S_r q dy   S hy dy = S_c S_r q dy dy
// and S_c S_r q is dL/dopacity itself -- SIX values through the permlane steps instead of nine, two multiplications per entry
// instead of six.
__device__ __forceinline__ void reduce_quad_and_add(float pair[6], float quad[6], float dx_row, uint32_t rows,
                                                    bool is_row_end)
{
    float c[6], r[9];
    swap16_add<6>(pair, quad, c);
    r[0] = dx_row * c[0]; // S hx     (all five / opacity)
    r[1] = c[1];          // S hy
    r[2] = dx_row * r[0]; // S hx dx
    r[3] = dx_row * c[1]; // S hx dy
    r[4] = c[2];          // S hy dy
    r[5] = c[0];          // dL/dopacity
    r[6] = c[3];
    r[7] = c[4];
    r[8] = c[5];
    row_sum9_to_lane15(r);
    if (is_row_end) {
        // a raw ds_add_f32: hipcc's atomic optimiser would wrap a C++ atomicAdd in a per-lane scan loop
#pragma unroll
        for (int g = 0; g < 9; ++g)
            asm volatile("ds_add_f32 %0, %1 offset:%2" ::"v"(rows), "v"(r[g]), "n"(g * 257 * 4) : "memory");
    }
}

constexpr uint32_t kNullEntry  = 256u;                // LDS row of the entry that blends nowhere
constexpr uint32_t kRows       = 257u;                // rows per slab / accumulator columns: a round's 256 entries + the null entry
constexpr uint32_t kSlab       = kRows * 16u;         // bytes per slab of s_rows
constexpr uint32_t kListStride = 264u;                // 256 entries + 3 of padding, a multiple of four (8-byte rows)

// (six waves per SIMD: 80 VGPRs with 8 spilled registers per lane instead of 92 and five waves -- render-backward 0.71 ->
//  0.67 ms, +1.6 % on the whole forward+backward step in same-box A/B runs; seven waves spill 19 and lose it again)
// KNOWN: the forward kept every entry's strip bits (it always does when it keeps backward state; the other instantiation
// repeats the four strip tests and exists for callers of the launcher that pass no masks)
// PERSIST: a bounded grid pulling tiles from *work_counter (zeroed by k_zero_grads2d), as in render.hip: while another view's
// forward is in flight (lcgs_fit_views) the cap leaves wave slots, registers and LDS free on every CU for its sort chain.
#ifndef LCGS_BWD_WAVES
#define LCGS_BWD_WAVES 6
#endif
// fill: the dense per-splat gradient rows' zero-fill as a side job (launch.hpp DenseFill): slot s clears its share of the five
// arrays' 16-byte-aligned interiors with fire-and-forget stores before it turns to its tile -- 1.45 GB through a memory
// system this VALU-bound kernel leaves idle, instead of 0.33 ms of memset kernels beside it that cost it 0.13 ms.
template <bool KNOWN, bool PERSIST>
__global__ void __launch_bounds__(256, LCGS_BWD_WAVES) k_render_backward(CamParams cp, float bg0, float bg1, float bg2,
                                                           const uint32_t* __restrict__ ranges,
                                                           const uint32_t* __restrict__ point_list,
                                                           const SplatRecord* __restrict__ recs,
                                                           const float* __restrict__ final_T,
                                                           const uint32_t* __restrict__ n_contrib,
                                                           const float* __restrict__ dL_dimg,
                                                           float* __restrict__ grads2d,
                                                           const uint32_t* __restrict__ tile_order,
                                                           const uint8_t* __restrict__ strip_masks,
                                                           const uint32_t* __restrict__ d_counts,
                                                           uint32_t* __restrict__ work_counter, DenseFill fill)
{
    // one 16-byte row per entry in each of three slabs (ONE address register serves an entry's three reads, as in the forward):
    // [0] mean.x, mean.y, -conic.x / 2, conic.y   [1] -conic.z / 2, opacity, r, g   [2] b, power floor, -, -
    // (the halved, negated diagonal: `power` then needs no multiplication by -1/2 -- a power of two commutes with rounding, so
    //  the value is the forward's bit for bit)
    // (row kNullEntry of every slab is the null entry that pads a strip's list to a multiple of four: opacity 0, blends nowhere;
    //  its accumulator column is never read)
    __shared__ float4             s_rows[3][kRows];
    __shared__ uint2              s_flush[256]; // the round's entries that reach a strip at all, compacted: (LDS row, splat)
    __shared__ uint32_t           s_fcnt[4];    // ... how many of them each staging wave holds
    __shared__ float              s_grad[9][kRows];
    __shared__ __attribute__((aligned(8))) uint16_t s_list[4][kListStride]; // [strip]: the round's entries to walk, back to front
    __shared__ unsigned long long s_mask[4][4]; // [staging wave][strip]
    __shared__ uint32_t           s_max[4];
    __shared__ uint32_t           s_slot;

    // a frame that drew nothing left final_T / n_contrib untouched (the forward returns before writing them, like
    // gs_tile_splatter/impl.cpp:109): there is nothing to differentiate, and nothing valid to read
    const bool     nothing_drawn = d_counts && d_counts[1] == 0u;
    if (nothing_drawn && fill.n[3] == 0u) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t slots = tile_order ? cp.grid_x * cp.grid_y : render_grid_size(cp.grid_x, cp.grid_y);
    uint32_t       slot  = blockIdx.x;
  for (;;) { // (one pass unless PERSIST)
    if (PERSIST) {
        __syncthreads(); // the previous tile's last flush has read s_flush / s_grad; nobody still reads s_slot
        if (tid == 0) s_slot = atomicAdd(work_counter, 1u);
        __syncthreads();
        slot = s_slot;
    }
    if (slot >= slots) return; // persistent grids: the exit every workgroup reaches
    if (fill.n[3] != 0u) { // (wave-uniform) the dense rows' zero-fill: this slot's share of each array
        // (streaming stores: 1.45 GB that nothing reads before the preprocess pass overwrites 39 % of it -- together with
        //  that pass's streaming row stores +2.2 % forward+backward in same-box A/B, profiles/r04_nt_accesses_ab.txt)
        typedef float v4f __attribute__((ext_vector_type(4)));
        const v4f z = { 0.0f, 0.0f, 0.0f, 0.0f };
#define LCGS_FILL_STORE(P) __builtin_nontemporal_store(z, reinterpret_cast<v4f*>(P))
        // per array: up to 3 floats in front of the first 16-byte boundary and behind the last one go to slot 0, the aligned
        // interior is shared out as float4 stores
#define LCGS_FILL(A)                                                                                     \
    {                                                                                                    \
        float*         base = fill.b##A;                                                                 \
        const uint32_t n    = fill.n[A];                                                                 \
        uint32_t       head = (uint32_t)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(base) & 15u)) & 15u) >> 2; \
        head                = head < n ? head : n;                                                       \
        const uint32_t n4 = (n - head) >> 2, tail = n - head - 4u * n4;                                   \
        float4*        mid = reinterpret_cast<float4*>(base + head);                                     \
        for (uint32_t i = slot * 256u + tid; i < n4; i += slots * 256u) LCGS_FILL_STORE(mid + i); /* 4 KB per slot and step */ \
        if (slot == 0u) {                                                                                \
            if (tid < head) base[tid] = 0.0f;                                                            \
            if (tid < tail) base[head + 4u * n4 + tid] = 0.0f;                                           \
        }                                                                                                \
    }
        LCGS_FILL(0) LCGS_FILL(1) LCGS_FILL(2) LCGS_FILL(3) LCGS_FILL(4)
#undef LCGS_FILL
#undef LCGS_FILL_STORE
    }
    if (nothing_drawn) {
        if (PERSIST) continue;
        return;
    }
    uint32_t tx, ty;
    if (tile_order) { // longest-list-first schedule of the forward (scheduling hint only)
        const uint32_t t = tile_order[slot];
        tx = t % cp.grid_x;
        ty = t / cp.grid_x;
    } else if (!tile_of_workgroup(slot, cp.grid_x, cp.grid_y, tx, ty)) {
        if (PERSIST) continue;
        return;
    }
    const uint32_t tile = ty * cp.grid_x + tx;
    const uint32_t px = unit_px(tx, wave, lane);
    const uint32_t py = unit_py(ty, wave, lane);
    const float    pxf = (float)px, pyf = (float)py;
    const bool     inside = (px < cp.width) && (py < cp.height);
    const size_t   hw  = (size_t)cp.width * cp.height;
    const size_t   pix = (size_t)px + (size_t)cp.width * py;

    const uint32_t last    = inside ? n_contrib[pix] : 0u; // 1-based list position of the last contributor
    const float    T_final = inside ? final_T[pix] : 0.0f;
    float          dpr = 0.0f, dpg = 0.0f, dpb = 0.0f;
    if (inside) {
        dpr = dL_dimg[pix];
        dpg = dL_dimg[pix + hw];
        dpb = dL_dimg[pix + 2 * hw];
    }

    uint32_t wmax = last;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = __shfl_xor(wmax, off, 64);
        wmax             = o > wmax ? o : wmax;
    }
    if (lane == 0) s_max[wave] = wmax;
    __syncthreads();
    uint32_t hi = s_max[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) hi = s_max[w] > hi ? s_max[w] : hi;
    const uint32_t range_start = ranges[2 * (size_t)tile + 0];
    {   // never walk past the tile's own list, whatever n_contrib holds
        const uint32_t len = ranges[2 * (size_t)tile + 1] - range_start;
        hi                 = hi < len ? hi : len;
    }
    hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)hi); // (uniform by construction: keeps the round bounds on the scalar side)

    // per-pixel recurrences, walked back to front
    // Qr: product of (1 - alpha) over the entries walked so far, over T_final (a pixel outside the image: infinity, T = 0)
    // Bd: (colour composited behind the current splat) . dL/dpixel, the background being the last layer
    float             Qr = 1.0f / T_final, Bd = bg0 * dpr + bg1 * dpg + bg2 * dpb;
    const bool        is_row_end = (lane & 15u) == 15u;
    const uint32_t    grad_base  = (uint32_t)(uintptr_t)&s_grad[0][0]; // low half of a flat LDS address = LDS offset

    if (tid == 0u) { // the null entry (visible to every wave behind the first round's barriers)
        s_rows[0][kNullEntry] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        s_rows[1][kNullEntry] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        s_rows[2][kNullEntry] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    while (hi > 0u) {
        const uint32_t lo   = hi > 256u ? hi - 256u : 0u;
        const uint32_t e    = lo + tid;
        const bool     have = e < hi;
        // ---- stage entries [lo, hi): strip tests, per-strip ballots, slab; clear the round's accumulators
        float4   a = make_float4(0, 0, 0, 0), b = a;
        float    c = 0.0f, t = -1.0f;
        uint32_t vid = 0, kmask = 0;
        if (have) {
            vid = point_list[range_start + e];
            // the forward kept every entry's strip bits: entries that reach no strip are not even fetched
            if (KNOWN) kmask = strip_masks[range_start + e];
            if (!KNOWN || kmask != 0u) {
                const float4* p = reinterpret_cast<const float4*>(recs + vid);
                a = p[0];                                           // mx, my, ca, cb
                b = p[1];                                           // cc, opacity, r, g
                c = reinterpret_cast<const float*>(recs + vid)[8];  // b
                t = (2.0f * __logf(255.0f * b.y)) * 1.0001f + 2e-4f;
            }
            if (!KNOWN) {
                const float rx0 = (float)(tx * kBlockX), ry0 = (float)(ty * kBlockY), rx1 = rx0 + (float)(kBlockX - 1);
                kmask = splat_unit_mask(a.x, a.y, a.z, a.w, b.x, t, rx0, ry0, rx1);
            }
        }
        __syncthreads(); // previous round fully flushed
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned long long m = __ballot((kmask >> k) & 1u);
            if (lane == 0) s_mask[wave][k] = m;
        }
        s_rows[0][tid] = make_float4(a.x, a.y, -0.5f * a.z, a.w);
        s_rows[1][tid] = make_float4(-0.5f * b.x, b.y, b.z, b.w);
        *reinterpret_cast<float2*>(&s_rows[2][tid]) = make_float2(c, fmax_(-0.5f * t, kBlendExpMin));
        const unsigned long long fm = __ballot(have && kmask != 0u); // entries with something to flush
        if (lane == 0) s_fcnt[wave] = (uint32_t)__popcll(fm);
#pragma unroll
        for (int g = 0; g < 9; ++g) s_grad[g][tid] = 0.0f;
        __syncthreads();

        // ---- the flush list: the entries some strip will add to, compacted (a round holds ~150 of 256 on the bench frames, and
        // the flush spends 16 lanes on each)
        uint32_t n_flush;
        {
            const uint32_t c0 = s_fcnt[0], c1 = s_fcnt[1], c2 = s_fcnt[2], c3 = s_fcnt[3];
            const uint32_t before = (wave > 0u ? c0 : 0u) + (wave > 1u ? c1 : 0u) + (wave > 2u ? c2 : 0u);
            n_flush               = c0 + c1 + c2 + c3;
            if (have && kmask != 0u) {
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(fm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)fm, 0u));
                s_flush[before + rank] = make_uint2(tid, vid);
            }
        }

        // ---- this strip's entries of the round as a list, back to front: the four ballots' set bits, highest first, padded to
        // a multiple of four with the null entry.  The walk below then has no data-dependent branch at all: one 8-byte LDS
        // read names four entries, their evaluations are straight-line code the scheduler can overlap (what a scalar bit
        // walk with a branch per entry cost: profiles/r05_bwd_list_walk_ab.txt).
        uint32_t n_walk = 0u; // (scalar)
        {
            uint16_t* list = &s_list[wave][0];
#pragma unroll
            for (int w = 3; w >= 0; --w) {
                const unsigned long long mm  = s_mask[w][wave];
                const uint32_t           mlo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)mm);
                const uint32_t           mhi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(mm >> 32));
                const uint32_t below = __builtin_amdgcn_mbcnt_hi(mhi, __builtin_amdgcn_mbcnt_lo(mlo, 0u)); // set bits under my lane
                const uint32_t total = (uint32_t)__builtin_popcount(mlo) + (uint32_t)__builtin_popcount(mhi);
                const uint32_t mine  = lane < 32u ? mlo >> lane : mhi >> (lane - 32u);
                if (mine & 1u) list[n_walk + (total - 1u - below)] = (uint16_t)((uint32_t)w * 64u + lane);
                n_walk += total;
            }
            if (lane < 4u) list[n_walk + lane] = (uint16_t)kNullEntry;
            asm volatile("" ::: "memory"); // (the list is read back as 8-byte words below)
        }

        // ---- walk them, four at a time (see the reduction notes above)
        {
            // the nine per-pixel terms of entry idx (an LDS row of this round, or the null entry)
            // (q = dL/dopacity = G dL/dalpha; q dy; q dy dy; the three colour terms.  G dL/dG = opacity x q: the entry-uniform
            //  opacity joins the other entry-uniform factors at the flush)
            auto evaluate = [&](const uint32_t idx, float v[6], uint32_t& row) {
                const uint32_t pos = lo + idx; // 0-based list position (the null entry: >= hi, never below `last`)
                uint32_t roff = idx * 16u; // (byte offset of the entry's row in every slab; pinned: one scalar-to-vector move)
                asm("" : "+v"(roff));
                const char*    rows = reinterpret_cast<const char*>(&s_rows[0][0]) + roff;
                const float4   ea = *reinterpret_cast<const float4*>(rows);
                const float4   eb = *reinterpret_cast<const float4*>(rows + kSlab);
                const float2   ec = *reinterpret_cast<const float2*>(rows + 2 * kSlab);
                // the forward's own expression and evaluation order: the same splats pass the same thresholds
                const float dx    = ea.x - pxf;
                const float dy    = ea.y - pyf;
                const float power = (ea.z * dx * dx + eb.x * dy * dy) - ea.w * dx * dy; // (ea.z, eb.x: -ca / 2, -cc / 2)
                const bool  c_pos = pos < last, c_neg = !(power > 0.0f), c_flr = power >= ec.y;
                const bool  cand  = c_pos & c_neg & c_flr;
                // (three ballots of plain compares are the compares' own lane masks; a ballot of the conjunction costs a
                //  select and another compare -- two vector instructions per walked entry)
                // exp(power): the hardware's v_exp_f32 (1 ulp; two instructions) since round 5, not the forward's DEFINED
                // function (ten).  The forward needs that one for bit-identical images; here the tolerance is 1e-3 and what
                // the two differ by -- ~1e-7 relative in alpha, an entry within that of alpha = 1/255 blended on one side
                // only (its weight is <= T / 255) -- is far inside it in the norm.  Row by row, tests/gpu_util.py::check_gradient_rows
                // holds every gradient row to its own bound, whose flip term counts each entry within a few 1e-6 of 1/255,
                // 0.99 or power = 0 in full.  On a frame whose opacities are constructed to put o G within 2 ulp of both
                // thresholds (tests/test_gpu_gradient_rows.py; the flip term fires on 2 613 rows there) one SH row lands
                // at 1.000 of its bound -- what one near-threshold entry decided apart from the forward and counted in full
                // looks like (not yet A/B'd against the defined exp) -- the others <= 0.79; ordinary frames <= 0.51.  render-backward 0.66-0.68 -> 0.63-0.64 ms, forward+backward
                // +2.2 % in same-box A/B (profiles/r05_bwd_hw_exp_ab.txt; -DLCGS_BWD_DEFINED_EXP builds the old form).
#ifdef LCGS_BWD_DEFINED_EXP
                const float G     = blend_exp(power);
#else
                const float G     = __builtin_amdgcn_exp2f(power * kExpLog2e);
#endif
                const float oG    = eb.y * G;
                const float alpha = __builtin_fminf(0.99f, oG);
                const bool  valid = cand & !(alpha < 1.0f / 255.0f);
                // A lane that does not blend this entry carries alpha 0 through the recurrences: the product keeps its
                // value, Bd + 0 * d leaves the colour behind alone, all terms come out 0.
                // (No second wave-level skip: the staging floor already implies alpha >= 1/255 somewhere.)
                const float a   = valid ? alpha : 0.0f;
                // T in front of this splat = T_final / prod(1 - a) over this entry and everything behind it.  The product (over
                // T_final: Qr) is carried (one rounded multiplication per entry: errors of either sign, ~sqrt(n) half-ulps at the front of
                // n entries) and divided out ONCE per entry with v_rcp_f32 (1 ulp, not carried).  Dividing T itself entry
                // by entry with v_rcp_f32 is what drifted in round 3 (its bias was seen by every splat in front: a
                // screen-filling splat, whose geometry gradients are sums of ~1e5 cancelling per-pixel terms, amplified it
                // to a few 1e-3); rounds 4-5 paid a Newton step on that quotient (two FMAs) -- this form needs neither.
                Qr = Qr * (1.0f - a);
                const float Tn  = __builtin_amdgcn_rcpf(Qr); // the forward's T in front of this splat
                const float wgt = a * Tn;
                // colour behind this splat (B, the background included: it is the last layer, with weight T_final) enters
                // dL/dalpha = T (c - B) . dL/dpixel, then B absorbs the splat: B <- B + a (c - B).  Only B . dL/dpixel is ever
                // used, and the recurrence is linear: ONE carried value (Bd) instead of three colours
                const float d         = __builtin_fmaf(eb.z, dpr, __builtin_fmaf(eb.w, dpg, ec.x * dpb)) - Bd; // (c - B) . dL/dpixel
                const float dL_dalpha = d * Tn;
                Bd                    = __builtin_fmaf(a, d, Bd);
                // the 0.99 cap passes no gradient to G / opacity
                // (selected AFTER the product: on a lane that is not a candidate `power` lies outside blend_exp's
                //  domain and G is arbitrary bits, possibly NaN -- it must not meet a multiplication by 0)
                v[0] = (valid & (oG < 0.99f)) ? G * dL_dalpha : 0.0f; // q = dL/dopacity
                v[1] = v[0] * dy;             // the entry-uniform factors (opacity, conic, -1, -0.5) are applied once per entry
                v[2] = v[1] * dy;             // when the round is flushed, dx behind the row sums (reduce_quad_and_add)
                v[3] = wgt * dpr;
                v[4] = wgt * dpg;
                v[5] = wgt * dpb;
                row  = grad_base + idx * 4u;
            };
            uint32_t rows = grad_base;
            // rows 0 .. 3 of the wave hold entries A, C, B, D of a group = list slots 0, 2, 1, 3 (bytes into the group's four u16)
            const uint32_t my_slot = 2u * ((((lane >> 4) & 1u) << 1) | (lane >> 5));
            for (uint32_t i = 0u; i < n_walk; i += 4u) {
                const uint2    four = *reinterpret_cast<const uint2*>(&s_list[wave][i]);
                const uint32_t p0   = (uint32_t)__builtin_amdgcn_readfirstlane((int)four.x);
                const uint32_t p1   = (uint32_t)__builtin_amdgcn_readfirstlane((int)four.y);
                float          A[6], B[6], pair[6], quad[6];
                uint32_t       row;
                // the entry my 16-lane row will hold behind the two swaps, and its dx at my column
                const uint32_t mine   = *reinterpret_cast<const uint16_t*>(reinterpret_cast<const char*>(&s_list[wave][i]) + my_slot);
                const float    dx_row = s_rows[0][mine].x - pxf;
                evaluate(p0 & 0xFFFFu, A, row);
                asm("v_writelane_b32 %0, %1, 15" : "+v"(rows) : "s"(row));
                evaluate(p0 >> 16, B, row);
                asm("v_writelane_b32 %0, %1, 47" : "+v"(rows) : "s"(row));
                swap32_add<6>(A, B, pair);
                evaluate(p1 & 0xFFFFu, A, row);
                asm("v_writelane_b32 %0, %1, 31" : "+v"(rows) : "s"(row));
                evaluate(p1 >> 16, B, row);
                asm("v_writelane_b32 %0, %1, 63" : "+v"(rows) : "s"(row));
                swap32_add<6>(A, B, quad);
                reduce_quad_and_add(pair, quad, dx_row, rows, is_row_end);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the raw LDS adds above have landed
        __syncthreads();
        // ---- flush the round.  Global float atomics run at full rate only when a wave instruction covers
        // contiguous bytes (MI355X_MICROARCH "Global float atomics": 64 lanes in 64 different rows are ~17x
        // slower), so consecutive lanes own one entry's gradient row instead of one lane per entry: 16 lanes per
        // entry (9 of them active; shifts and masks instead of a division by 12 in a loop that runs every round).
        for (uint32_t cidx = tid; cidx < n_flush * 16u; cidx += 256u) {
            const uint32_t g   = cidx & 15u;
            const uint2    fe  = s_flush[cidx >> 4];
            const uint32_t idx = fe.x, v = fe.y;
            if (g < 9u) {
                // sums -> gradients: d/dmean = -(conic . (S hx, S hy)), d/dconic = (-1/2, -1, -1/2) (S hx dx, ...), the five of them
                // times the opacity (the sums were formed from q = h / opacity)
                float s = s_grad[g][idx];
                if (g < 5u) {
                    const float4 eb = s_rows[1][idx]; // -cc / 2, opacity, ..
                    if (g < 2u) {
                        const float4 ea = s_rows[0][idx];
                        const float  ca = -2.0f * ea.z, cc = -2.0f * eb.x, s0 = s_grad[0][idx], s1 = s_grad[1][idx];
                        s = (g == 0u) ? -(ca * s0 + ea.w * s1) : -(cc * s1 + ea.w * s0);
                    } else {
                        s *= (g == 3u) ? -1.0f : -0.5f;
                    }
                    s *= eb.y;
                }
                if (s != 0.0f) atomicAdd(&grads2d[(size_t)v * kG2D + g], s);
            }
        }
        hi = lo;
    }
    if (!PERSIST) break;
  }
}

// (the per-splat expressions -- geom_backward, the operands' loads, the two colour steps -- are splat_backward.hpp's)
// One lane per surviving splat (dense ids).  The splat's 48 SH coefficients arrive through the wave's LDS slab
// (cooperative 16-byte loads, 12 lanes per 192-byte row), the SH gradient row is written back IN PLACE into the
// slab as it is produced (so it never lives in registers next to the geometry Jacobians) and leaves as coalesced
// 16-byte stores.
// the four geometry rows of one splat; accumulate: add to what the arrays hold (a further view of a multi-view batch)
__device__ __forceinline__ void store_geometry_rows(size_t orow, bool accumulate, const float gp[3], const float gs[3],
                                                    float4 gq, float gop, float* __restrict__ dL_dpos,
                                                    float* __restrict__ dL_dscale, float* __restrict__ dL_drotq,
                                                    float* __restrict__ dL_dopacity)
{
    float4* rq = reinterpret_cast<float4*>(dL_drotq + 4 * orow); // (r,x,y,z)
    if (accumulate) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            dL_dpos[3 * orow + i] += gp[i];
            dL_dscale[3 * orow + i] += gs[i];
        }
        const float4 o = *rq;
        *rq            = make_float4(o.x + gq.x, o.y + gq.y, o.z + gq.z, o.w + gq.w);
        dL_dopacity[orow] += gop;
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            dL_dpos[3 * orow + i]   = gp[i];
            dL_dscale[3 * orow + i] = gs[i];
        }
        *rq               = gq;
        dL_dopacity[orow] = gop;
    }
}

template <bool AA>
__global__ void __launch_bounds__(256)
k_preprocess_backward(int sh_deg, CamParams cp, float scale_modifier, const float* __restrict__ pos,
                      const float* __restrict__ scale, const float* __restrict__ rotq, const float* __restrict__ sh,
                      const uint32_t* __restrict__ vis_index, const uint32_t* __restrict__ d_counts,
                      const float* __restrict__ grads2d, float* __restrict__ dL_dpos, float* __restrict__ dL_dscale,
                      float* __restrict__ dL_drotq, float* __restrict__ dL_dsh, float* __restrict__ dL_dopacity,
                      int mode, const uint32_t* __restrict__ slice_bounds, int slice, const float* __restrict__ opacity)
{
    __shared__ float4 s_sh[4][64 * 13];
    const bool compact = (mode & 1) != 0, accumulate = (mode & 2) != 0; // (see launch_preprocess_backward)
    // the survivors (dense ids) this launch covers: all of them, or slice `slice` of a splat-range split (k_slice_bounds)
    const uint32_t v0 = slice_bounds ? slice_bounds[slice] : 0u;
    const uint32_t V  = slice_bounds ? slice_bounds[slice + 1] : d_counts[0];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int feat = (sh_deg + 1) * (sh_deg + 1);
    const bool staged = sh_deg == 3 && ((reinterpret_cast<uintptr_t>(sh) & 15) == 0) &&
                        ((reinterpret_cast<uintptr_t>(dL_dsh) & 15) == 0);
    for (uint32_t blk = blockIdx.x; v0 + blk * 256u < V; blk += gridDim.x) {
        const RowBlock b   = row_block(v0, V, blk, vis_index);
        float*         row = reinterpret_cast<float*>(&s_sh[wave][lane * 13]); // this lane's 48 floats (+4 pad)
        const SplatOperands in = load_splat_operands<AA>(b.vsafe, b.idx, grads2d, pos, scale, rotq, opacity); // (with the SH rows below)

        // ---- stage the SH rows (coalesced), or fetch them lane-wise for other degrees
        __syncthreads();
        // (its own copy of the 12-lane loop: through row_part_step the kernel's SGPR spills change)
        if (staged) {
#pragma unroll
            for (int i = 0; i < 12; ++i) {
                const uint32_t c    = (uint32_t)i * 64u + lane;
                const uint32_t slot = c / 12u, part = c - slot * 12u;
                const int      sidx = __shfl(b.idx, (int)slot, 64);
                if (slot < b.nvalid) s_sh[wave][slot * 13u + part] = reinterpret_cast<const float4*>(sh + (size_t)sidx * 48)[part];
            }
        } else if (b.valid) {
            const float* s = sh + (size_t)b.idx * feat * 3;
            for (int k = 0; k < 48; ++k) row[k] = k < feat * 3 ? s[k] : 0.0f;
        }
        __syncthreads();

        if (b.valid) {
            float gp[3] = { 0.0f, 0.0f, 0.0f };

            // ---- colour -> SH coefficients and position (through the view direction)
            sh_colour_step<true>(cp, in, feat, row, gp);

            float  gs[3], gop;
            float4 gq;
            geom_backward<AA>(cp, scale_modifier, in, gp, gs, gq, gop);

            const size_t orow = compact ? (size_t)b.vid : (size_t)b.idx; // compact: row = dense id (see launch.hpp)
            store_geometry_rows(orow, accumulate, gp, gs, gq, gop, dL_dpos, dL_dscale, dL_drotq, dL_dopacity);
        }

        // ---- SH gradient rows: 12 consecutive lanes write one splat's 192 contiguous bytes
        __syncthreads();
        if (staged) {
#pragma unroll
            for (int i = 0; i < 12; ++i)
                row_part_step(b, lane, i, [&](uint32_t slot, uint32_t part, int sidx) {
                    const size_t orow = compact ? (size_t)(b.wave_first + slot) : (size_t)sidx;
                    float4*      dst  = reinterpret_cast<float4*>(dL_dsh + orow * 48) + part;
                    float4       v    = s_sh[wave][slot * 13u + part];
                    if (accumulate) {
                        const float4 o = *dst;
                        v = make_float4(o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w);
                    }
                    *dst = v;
                });
        } else if (b.valid) {
            float* o = dL_dsh + (compact ? (size_t)b.vid : (size_t)b.idx) * feat * 3;
            for (int k = 0; k < feat * 3; ++k) o[k] = accumulate ? o[k] + row[k] : row[k];
        }
    }
}

// The same step for frames whose forward kept the colour Jacobian (build_records<.., JAC>; degree 3): nothing of the
// 192-byte coefficient row is read again.  dL/dsh[k][c] = basis_k(direction) * dL/dcolour[c] (clamp-masked) is an
// outer product of 16 + 3 numbers per splat: each lane parks those 19 floats in LDS and the wave writes the 192-byte
// gradient rows cooperatively (12 lanes x 16 B per row), forming the products on the way out.  The direction part of
// dL/dpos comes from the kept 3x3 Jacobian.  No 53 KB slab, a third of the registers: more workgroups in flight on
// a kernel that is bound by bytes in flight.
constexpr int kJacPitch = 19; // floats per splat in the LDS slab (odd: conflict-free per-lane writes)

// float4 `part` (0..11) of a splat's 16 x 3 SH gradient row, formed from the 19 floats of its slab slot
__device__ __forceinline__ float4 jac_outer_part(const float* slot, uint32_t part)
{
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const uint32_t f = part * 4u + (uint32_t)e, k = f / 3u, ch = f - 3u * k; // row[k * 3 + ch]
        v[e]             = slot[k] * slot[16u + ch];
    }
    return make_float4(v[0], v[1], v[2], v[3]);
}

template <bool AA>
__global__ void __launch_bounds__(256)
k_preprocess_backward_jac(CamParams cp, float scale_modifier, const float* __restrict__ pos,
                          const float* __restrict__ scale, const float* __restrict__ rotq,
                          const uint32_t* __restrict__ vis_index, const uint32_t* __restrict__ d_counts,
                          const float* __restrict__ grads2d, const float4* __restrict__ shjac,
                          float* __restrict__ dL_dpos, float* __restrict__ dL_dscale, float* __restrict__ dL_drotq,
                          float* __restrict__ dL_dsh, float* __restrict__ dL_dopacity, int mode,
                          const uint32_t* __restrict__ slice_bounds, int slice, const float* __restrict__ opacity)
{
    __shared__ float s_outer[4][64 * kJacPitch];
    const bool compact = (mode & 1) != 0, accumulate = (mode & 2) != 0;
    const uint32_t v0 = slice_bounds ? slice_bounds[slice] : 0u; // (see k_preprocess_backward)
    const uint32_t V  = slice_bounds ? slice_bounds[slice + 1] : d_counts[0];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t blk = blockIdx.x; v0 + blk * 256u < V; blk += gridDim.x) {
        const RowBlock      b  = row_block(v0, V, blk, vis_index);
        const SplatOperands in = load_splat_operands<AA>(b.vsafe, b.idx, grads2d, pos, scale, rotq, opacity);
        const float4 j0 = shjac[(size_t)b.vsafe * 3 + 0], j1 = shjac[(size_t)b.vsafe * 3 + 1], j2 = shjac[(size_t)b.vsafe * 3 + 2];
        if (b.valid) {
            float  gp[3], gs[3], gop;
            float4 gq;
            jac_colour_step(cp, in, j0, j1, j2, &s_outer[wave][lane * kJacPitch], gp);
            geom_backward<AA>(cp, scale_modifier, in, gp, gs, gq, gop);
            const size_t orow = compact ? (size_t)b.vid : (size_t)b.idx; // compact: row = dense id (see launch.hpp)
            store_geometry_rows(orow, accumulate, gp, gs, gq, gop, dL_dpos, dL_dscale, dL_drotq, dL_dopacity);
        }
        __syncthreads();
        // ---- SH gradient rows: 12 consecutive lanes write one splat's 192 contiguous bytes
#pragma unroll 1
        for (int i = 0; i < 12; ++i)
            row_part_step(b, lane, i, [=](uint32_t slot, uint32_t part, int sidx) { // (by value: by reference costs two SGPRs)
                float4       v    = jac_outer_part(&s_outer[wave][slot * kJacPitch], part);
                const size_t orow = compact ? (size_t)(b.wave_first + slot) : (size_t)sidx;
                float4*      dst  = reinterpret_cast<float4*>(dL_dsh + orow * 48) + part;
                if (accumulate) {
                    const float4 o = *dst;
                    v = make_float4(v.x + o.x, v.y + o.y, v.z + o.z, v.w + o.w);
                }
                // written once, read by the optimiser / the all-reduce a kernel later: a streaming store
                st_stream(dst, v);
            });
        __syncthreads(); // the slab is reused by the next iteration
    }
}

// The same per-splat pass with the optimiser folded in (single-GPU training steps: lcgs_render_backward_adam).  The
// gradients of a splat exist only in this lane's registers (geometry, opacity) and in the wave's LDS slab (the 16 + 3
// factors of the SH outer product): the on-screen-only Adam update of train.hip is applied right here -- through the
// functions of adam_rows.hpp that train.hip's kernels call, on gradients formed by the functions k_preprocess_backward_jac
// calls, so the result is the two calls' bit for bit -- and NO gradient row is ever written or read back (2 x 236 bytes
// per on-screen splat less; the separate step was 0.56 GB written by this kernel + 0.56 GB read by the optimiser's on the
// bicycle stand-in).  Each lane owns its splat's rows in raw / m / v / activated: read, updated, written by the same lane,
// so the in-place update of the arrays this very kernel reads (the activated pos / scale / rotq are the renderer's scene
// arrays) needs no synchronisation.
template <bool AA>
__global__ void __launch_bounds__(256)
k_preprocess_backward_adam(CamParams cp, float scale_modifier, const float* pos, const float* scale, const float* rotq,
                           const float* opacity,
                           const uint32_t* __restrict__ vis_index, const uint32_t* __restrict__ d_counts,
                           const float* __restrict__ grads2d, const float4* __restrict__ shjac, AdamArrays raw, AdamArrays am,
                           AdamArrays av, AdamArrays act, AdamRates lr, AdamStep a)
{
    __shared__ float s_outer[4][64 * kJacPitch];
    const uint32_t V = d_counts[0];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t blk = blockIdx.x; blk * 256u < V; blk += gridDim.x) {
        const RowBlock b   = row_block(0u, V, blk, vis_index);
        const int      idx = b.idx;
        // (an antialiased frame's raw opacity is read here, before this lane's update of the activated row below)
        const SplatOperands in = load_splat_operands<AA>(b.vsafe, idx, grads2d, pos, scale, rotq, opacity);
        const float4 j0 = shjac[(size_t)b.vsafe * 3 + 0], j1 = shjac[(size_t)b.vsafe * 3 + 1], j2 = shjac[(size_t)b.vsafe * 3 + 2];
        if (b.valid) {
            float  gp[3], gs[3], gop;
            float4 gq;
            jac_colour_step(cp, in, j0, j1, j2, &s_outer[wave][lane * kJacPitch], gp);
            geom_backward<AA>(cp, scale_modifier, in, gp, gs, gq, gop);
            // ---- Adam on this splat's geometry rows (train.hip: k_adam_rows<3,0>, <3,1>, k_adam_rot, <1,2>)
            const size_t i3 = 3 * (size_t)idx;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float x = raw.pos[i3 + c], mm = am.pos[i3 + c], vv = av.pos[i3 + c];
                adam_plain(gp[c], x, mm, vv, lr.pos, a);
                am.pos[i3 + c]  = mm;
                av.pos[i3 + c]  = vv;
                raw.pos[i3 + c] = x;
                if (act.pos != raw.pos) act.pos[i3 + c] = x;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float x = raw.scale[i3 + c], mm = am.scale[i3 + c], vv = av.scale[i3 + c], sa = act.scale[i3 + c];
                adam_scale(gs[c], x, mm, vv, sa, lr.scale, a);
                am.scale[i3 + c]  = mm;
                av.scale[i3 + c]  = vv;
                raw.scale[i3 + c] = x;
                act.scale[i3 + c] = sa;
            }
            { // (gq is (r,x,y,z), like the rows)
                float4* rr = reinterpret_cast<float4*>(raw.rotq) + idx;
                float4* rm = reinterpret_cast<float4*>(am.rotq) + idx;
                float4* rv = reinterpret_cast<float4*>(av.rotq) + idx;
                float4* ra = reinterpret_cast<float4*>(act.rotq) + idx;
                float4  x = *rr, mm = *rm, vv = *rv, qa = *ra;
                adam_quat(gq, x, mm, vv, qa, lr.rot, a);
                *rr = x;
                *rm = mm;
                *rv = vv;
                *ra = qa;
            }
            {
                float x = raw.opacity[idx], mm = am.opacity[idx], vv = av.opacity[idx], o = act.opacity[idx];
                adam_opacity(gop, x, mm, vv, o, lr.opacity, a);
                am.opacity[idx]  = mm;
                av.opacity[idx]  = vv;
                raw.opacity[idx] = x;
                act.opacity[idx] = o;
            }
        }
        __syncthreads();
        // ---- SH rows: 12 consecutive lanes own one splat's 192 contiguous bytes of raw / m / v (train.hip: k_adam_sh48)
#pragma unroll 1
        // (its own copy of the 12-lane loop: through row_part_step the kernel's register counts change)
        for (int i = 0; i < 12; ++i) {
            const uint32_t cidx = (uint32_t)i * 64u + lane;
            const uint32_t slot = cidx / 12u, part = cidx - slot * 12u;
            const int      sidx = __shfl(idx, (int)slot, 64);
            if (slot < b.nvalid) {
                const float4 g  = jac_outer_part(&s_outer[wave][slot * kJacPitch], part);
                const size_t r4 = (size_t)sidx * 12 + part;
                float4*      xr = reinterpret_cast<float4*>(raw.sh) + r4;
                float4*      xm = reinterpret_cast<float4*>(am.sh) + r4;
                float4*      xv = reinterpret_cast<float4*>(av.sh) + r4;
                float4       x = *xr, mm = *xm, vv = *xv;
                adam_sh4(g, x, mm, vv, part, lr.sh_dc, lr.sh_rest, a);
                *xr = x;
                *xm = mm;
                *xv = vv;
                if (act.sh != raw.sh) reinterpret_cast<float4*>(act.sh)[r4] = x;
            }
        }
        __syncthreads(); // the slab is reused by the next iteration
    }
}

} // namespace

size_t grads2d_bytes(int64_t V_cap) { return (size_t)V_cap * kG2D * sizeof(float); }

namespace
{
__global__ void __launch_bounds__(256) k_zero_grads2d(const uint32_t* __restrict__ d_counts, float4* __restrict__ g,
                                                      uint32_t* __restrict__ bwd_counter)
{
    if (bwd_counter && blockIdx.x == 0 && threadIdx.x == 0) *bwd_counter = 0u; // the persistent render-backward's tile counter
    const size_t n = (size_t)d_counts[0] * (kG2D / 4);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        g[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}
} // namespace

void launch_zero_grads2d(const uint32_t* d_counts, float* grads2d, hipStream_t stream, uint32_t* bwd_counter)
{
    hipLaunchKernelGGL(k_zero_grads2d, dim3(2048), dim3(256), 0, stream, d_counts, reinterpret_cast<float4*>(grads2d), bwd_counter);
}

void launch_render_backward(const KeptFrame& f, const float bg[3], const float* dL_dimg, float* grads2d, hipStream_t stream,
                            uint32_t* work_counter, uint32_t persistent_wgs, const DenseFill* fill_)
{
    if (f.cp.grid_x * f.cp.grid_y == 0) return;
    const DenseFill fill = fill_ ? *fill_ : DenseFill{};
    const uint32_t full = render_grid_size(f.cp.grid_x, f.cp.grid_y);
#define LCGS_LAUNCH_BWD(KNOWN_, PERSIST_, GRID_)                                                                             \
    hipLaunchKernelGGL((k_render_backward<KNOWN_, PERSIST_>), dim3(GRID_), dim3(256), 0, stream, f.cp, bg[0], bg[1], bg[2],    \
                       f.ranges, f.point_list, f.recs, f.final_T, f.n_contrib, dL_dimg, grads2d, f.tile_order, f.strip_masks, \
                       f.d_counts, work_counter, fill)
    if (work_counter && persistent_wgs > 0 && persistent_wgs < full) {
        if (f.strip_masks) LCGS_LAUNCH_BWD(true, true, persistent_wgs);
        else LCGS_LAUNCH_BWD(false, true, persistent_wgs);
    } else {
        work_counter = nullptr;
        if (f.strip_masks) LCGS_LAUNCH_BWD(true, false, full);
        else LCGS_LAUNCH_BWD(false, false, full);
    }
#undef LCGS_LAUNCH_BWD
}

// Splat-range slices of the survivors (for the chunked gradient all-reduce, lcgs_grads_allreduce): the dense ids are
// handed out in ascending splat index, so the survivors whose splat index lies in [k P / K, (k + 1) P / K) are the
// dense ids [bounds[k], bounds[k + 1]).  One lane per boundary: lower_bound over vis_index[0, V).
__global__ void __launch_bounds__(64) k_slice_bounds(const uint32_t* __restrict__ vis_index,
                                                     const uint32_t* __restrict__ d_counts, uint32_t P, int slices,
                                                     uint32_t* __restrict__ bounds)
{
    const int k = threadIdx.x;
    if (k > slices) return;
    const uint32_t V = d_counts[0];
    uint32_t       lo = 0, hi = V; // first dense id whose splat index >= target
    if (k == slices) lo = V;
    else {
        const uint32_t target = (uint32_t)(((uint64_t)P * (uint64_t)k) / (uint64_t)slices);
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (vis_index[mid] < target) lo = mid + 1;
            else hi = mid;
        }
    }
    bounds[k] = lo;
}

void launch_slice_bounds(const KeptRows& r, int slices, uint32_t* bounds, hipStream_t stream)
{
    hipLaunchKernelGGL(k_slice_bounds, dim3(1), dim3(64), 0, stream, r.vis_index, r.d_counts, (uint32_t)r.P, slices, bounds);
}

void launch_preprocess_backward(const KeptRows& r, float* dL_dpos, float* dL_dscale, float* dL_drotq, float* dL_dsh,
                                float* dL_dopacity, const RowsOut& out, hipStream_t stream)
{
    const int mode = (out.compact ? 1 : 0) | (out.accumulate ? 2 : 0);
    // (a slice's launch is sized for its share of the hint; larger live counts are strided)
    const unsigned blocks = grid_256(r.hint / (out.slice_bounds ? out.slices : 1));
    const bool aa = r.cp.raster_mode != 0; // (one instantiation per raster mode: the classic pass carries none of the other's code)
    if (r.shjac && r.sh_deg == 3 && (reinterpret_cast<uintptr_t>(dL_dsh) & 15) == 0) {
#define LCGS_LAUNCH_JAC(AA_)                                                                                                   \
    hipLaunchKernelGGL((k_preprocess_backward_jac<AA_>), dim3(blocks), dim3(256), 0, stream, r.cp, r.scale_modifier, r.pos, r.scale, \
                       r.rotq, r.vis_index, r.d_counts, r.grads2d, r.shjac, dL_dpos, dL_dscale, dL_drotq, dL_dsh, dL_dopacity, \
                       mode, out.slice_bounds, out.slice, r.opacity)
        if (aa) LCGS_LAUNCH_JAC(true);
        else LCGS_LAUNCH_JAC(false);
#undef LCGS_LAUNCH_JAC
        return;
    }
#define LCGS_LAUNCH_ROWS(AA_)                                                                                                  \
    hipLaunchKernelGGL((k_preprocess_backward<AA_>), dim3(blocks), dim3(256), 0, stream, r.sh_deg, r.cp, r.scale_modifier, r.pos,  \
                       r.scale, r.rotq, r.sh, r.vis_index, r.d_counts, r.grads2d, dL_dpos, dL_dscale, dL_drotq, dL_dsh,        \
                       dL_dopacity, mode, out.slice_bounds, out.slice, r.opacity)
    if (aa) LCGS_LAUNCH_ROWS(true);
    else LCGS_LAUNCH_ROWS(false);
#undef LCGS_LAUNCH_ROWS
}

void launch_preprocess_backward_adam(const KeptRows& r, const AdamArrays& raw, const AdamArrays& m, const AdamArrays& v,
                                     const AdamArrays& act, const AdamRates& lr, const AdamStep& a, hipStream_t stream)
{
#define LCGS_LAUNCH_ADAM(AA_)                                                                                                  \
    hipLaunchKernelGGL((k_preprocess_backward_adam<AA_>), dim3(grid_256(r.hint)), dim3(256), 0, stream, r.cp, r.scale_modifier,   \
                       r.pos, r.scale, r.rotq, r.opacity, r.vis_index, r.d_counts, r.grads2d, r.shjac, raw, m, v, act, lr, a)
    if (r.cp.raster_mode != 0) LCGS_LAUNCH_ADAM(true);
    else LCGS_LAUNCH_ADAM(false);
#undef LCGS_LAUNCH_ADAM
}

} // namespace lcgs

