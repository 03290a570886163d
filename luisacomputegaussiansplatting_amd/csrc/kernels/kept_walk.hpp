// kept_walk.hpp -- the walk of a keep-state frame's KEPT per-tile lists, once, for every kernel that takes it again (maps.hip:
// depth and alpha maps and their backward; contrib.hip: per-splat blend-weight statistics).  KeptFrame is what such a walk reads
// (host and device: the launchers take it).  On the device: the tile prologue (workgroup -> tile in the renderer's schedule,
// the lane's pixel, the tile's walk length), walk_rounds -- rounds of 256 staged entries in either direction, strip-mask
// ballots, the entries read back as wave-uniform LDS broadcasts -- and the ONE restatement of the renderer's per-entry power and
// alpha (eval_entry, blend_entry).  A kernel adds its accumulators, its per-entry body and its flush.
#pragma once

#include "launch.hpp"
#include "tile_common.hpp"

namespace lcgs
{
// the last keep-state frame as the walks read it (final_T: the backwards only; strip_masks NULL: every entry is fetched);
// kept_rows.hpp has the counterpart for the passes with one lane per on-screen row
struct KeptFrame {
    CamParams          cp;
    const uint32_t*    ranges;
    const uint32_t*    point_list;
    const SplatRecord* recs;
    const float*       final_T;
    const uint32_t*    n_contrib;
    const uint8_t*     strip_masks;
    const uint32_t*    d_counts;
    const uint32_t*    tile_order;
};

namespace kept_walk
{
using namespace tile;

// the value a splat contributes to the depth map, and dL/dz from dL/dvalue = gv
__device__ __forceinline__ float depth_value(float z, int mode) { return mode == kDepthInvZ ? 1.0f / z : z; }
__device__ __forceinline__ float depth_value_backward(float z, int mode, float gv) { return mode == kDepthInvZ ? -gv / (z * z) : gv; }

// butterfly over each 16-lane row (every lane of the row ends with the row's total): xor 1, xor 2 inside the quads,
// then the half-row and the row mirrors.  row16_sum: float sum; row16_max: max on unsigned bits
__device__ __forceinline__ float row16_sum(float x)
{
#define LCGS_DPP_ADD(CTRL) x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, true))
    LCGS_DPP_ADD(0xB1);  // quad_perm:[1,0,3,2]
    LCGS_DPP_ADD(0x4E);  // quad_perm:[2,3,0,1]
    LCGS_DPP_ADD(0x141); // row_half_mirror
    LCGS_DPP_ADD(0x140); // row_mirror
#undef LCGS_DPP_ADD
    return x;
}
__device__ __forceinline__ uint32_t row16_max(uint32_t x)
{
#define LCGS_DPP_MAX(CTRL)                                                                     \
    {                                                                                          \
        const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, true); \
        x                = o > x ? o : x;                                                      \
    }
    LCGS_DPP_MAX(0xB1);
    LCGS_DPP_MAX(0x4E);
    LCGS_DPP_MAX(0x141);
    LCGS_DPP_MAX(0x140);
#undef LCGS_DPP_MAX
    return x;
}

// workgroup -> tile (the renderer's schedule); false: a padding slot of the XCD-aware map
__device__ __forceinline__ bool tile_of_slot(const CamParams& cp, const uint32_t* tile_order, uint32_t slot, uint32_t& tx, uint32_t& ty)
{
    if (tile_order) {
        if (slot >= cp.grid_x * cp.grid_y) return false;
        const uint32_t t = tile_order[slot];
        tx = t % cp.grid_x;
        ty = t / cp.grid_x;
        return true;
    }
    return tile_of_workgroup(slot, cp.grid_x, cp.grid_y, tx, ty);
}

// the tile's walk length: its largest n_contrib, never past its own list (uniform over the workgroup)
__device__ __forceinline__ uint32_t tile_walk_length(uint32_t last, uint32_t len, uint32_t* s_max, uint32_t lane, uint32_t wave)
{
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
    hi = hi < len ? hi : len;
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)hi);
}

// one staged entry: [0] mean.x, mean.y, -conic.x / 2, -conic.z / 2   [1] conic.y, power floor, opacity, value
// (the halved, negated diagonal and the floor are the renderer's own staging: same bits in `power`)
struct StagedEntry {
    float4 a, b;
};
__device__ __forceinline__ StagedEntry stage_entry(const SplatRecord* __restrict__ recs, uint32_t vid, int mode)
{
    const float4* p  = reinterpret_cast<const float4*>(recs + vid);
    const float4  r0 = p[0], r1 = p[1]; // mx, my, ca, cb | cc, opacity, r, g
    const float   z  = recs[vid].depth;
    const float   t  = (2.0f * __logf(255.0f * r1.y)) * 1.0001f + 2e-4f;
    StagedEntry   e;
    e.a = make_float4(r0.x, r0.y, -0.5f * r0.z, -0.5f * r1.x);
    e.b = make_float4(r0.w, fmax_(-0.5f * t, kBlendExpMin), r1.y, depth_value(z, mode));
    return e;
}

// The renderer's per-entry expressions, restated HERE ONLY for the kept walks: power = -0.5 (ca dx dx + cc dy dy) - cb dx dy with
// the products left to right, the two skips and alpha = min(0.99, opacity exp(power)) are render.hip's operation for operation
// (the build does not contract: -ffp-contract=off), so the same entries pass the same thresholds with the same bits -- what the
// bit-for-bit contracts of lcgs_render_maps and of weight_max / pixels rest on.  Change nothing here that render.hip does not.
struct EntryEval {
    float dx, dy, power;
    bool  cand; // the pixel has not ended before list position `pos`, and the entry passes the power tests
};
__device__ __forceinline__ EntryEval eval_entry(const float4& ea, const float4& eb, float pxf, float pyf, uint32_t pos, uint32_t last)
{
    EntryEval   v;
    v.dx              = ea.x - pxf;
    v.dy              = ea.y - pyf;
    const float qx    = (ea.z * v.dx) * v.dx, cross = eb.x * v.dx;
    const float qy    = (ea.w * v.dy) * v.dy;
    const float half  = qx + qy;
    v.power           = half - cross * v.dy;
    v.cand            = (pos < last) & !(v.power > 0.0f) & (v.power >= eb.y);
    return v;
}
struct EntryBlend {
    float G, oG, alpha; // exp(power), opacity exp(power), its 0.99 cap (arbitrary bits off the candidate lanes)
    bool  blended;      // a candidate whose alpha is not below 1 / 255: the forward blended it
};
__device__ __forceinline__ EntryBlend blend_entry(const float4& eb, const EntryEval& v)
{
    EntryBlend b;
    b.G       = blend_exp(v.power);
    b.oG      = eb.z * b.G;
    b.alpha   = __builtin_fminf(0.99f, b.oG);
    b.blended = v.cand & !(b.alpha < 1.0f / 255.0f);
    return b;
}

// the LDS every walk needs; a kernel declares it once, next to its own accumulators
struct WalkShared {
    float4             s_rows[2][256]; // the round's staged entries (StagedEntry a / b)
    unsigned long long s_mask[4][4];   // [staging wave][strip]
    uint32_t           s_max[4];
};

// what the prologue leaves a lane: its tile and pixel, the 1-based list position of the pixel's last contributor (0 outside
// the image), and the tile's list start and walk length (both uniform)
struct TileWalk {
    uint32_t tid, lane, wave, tile, px, py;
    bool     inside;
    size_t   pix;
    uint32_t last, range_start, hi;
    float    pxf, pyf;
};
// false: a padding slot.  A frame that drew nothing left n_contrib untouched: every length is zero and nothing of it is read
// (k_render_maps then writes its zeros; the other kernels return before they come here)
__device__ __forceinline__ bool tile_prologue(const KeptFrame& f, WalkShared& s, TileWalk& t)
{
    t.tid  = threadIdx.x;
    t.lane = t.tid & 63u;
    t.wave = t.tid >> 6;
    uint32_t tx, ty;
    if (!tile_of_slot(f.cp, f.tile_order, blockIdx.x, tx, ty)) return false;
    t.tile   = ty * f.cp.grid_x + tx;
    t.px     = unit_px(tx, t.wave, t.lane);
    t.py     = unit_py(ty, t.wave, t.lane);
    t.inside = (t.px < f.cp.width) && (t.py < f.cp.height);
    t.pix    = (size_t)t.px + (size_t)f.cp.width * t.py;
    const bool drawn   = f.d_counts[1] != 0u;
    t.last             = (t.inside && drawn) ? f.n_contrib[t.pix] : 0u;
    t.range_start      = drawn ? f.ranges[2 * (size_t)t.tile + 0] : 0u;
    const uint32_t len = drawn ? f.ranges[2 * (size_t)t.tile + 1] - t.range_start : 0u;
    t.hi               = tile_walk_length(t.last, len, s.s_max, t.lane, t.wave);
    t.pxf              = (float)t.px;
    t.pyf              = (float)t.py;
    return true;
}

// The walk.  BACK = false: front to back (the renderer's direction), rounds from the list's start, and a wave is done with a
// round at the first staging wave that lies past every pixel of its strip.  BACK = true: back to front, the first round the
// partial one, and such a staging wave is passed over.  Per round: a lane stages one entry (not fetched at all when the
// forward left it a zero strip-mask byte), `before(vid)` runs between the round's two barriers (vid: the splat the lane
// staged, ~0: none) -- the place to clear accumulators -- every wave then walks the set bits of its own strip's ballots in
// walk order and calls `body(idx, pos, ea, eb)` (idx: the entry's LDS row, pos: its 0-based list position) with the entry as
// wave-uniform LDS broadcasts, and `after()` ends the round (the flush, with whatever barrier it needs in front).
template <bool BACK, class Before, class Body, class After>
__device__ __forceinline__ void walk_rounds(const KeptFrame& f, WalkShared& s, const TileWalk& t, int mode, Before&& before,
                                            Body&& body, After&& after)
{
    for (uint32_t done = 0u; done < t.hi; done += 256u) {
        const uint32_t end = BACK ? t.hi - done : t.hi;                       // this round: list positions [lo, min(lo + 256, end))
        const uint32_t lo  = BACK ? (end > 256u ? end - 256u : 0u) : done;
        const uint32_t e   = lo + t.tid;
        uint32_t       kmask = 0u, vid = 0xFFFFFFFFu;
        StagedEntry    se;
        se.a = se.b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (e < end) {
            kmask = f.strip_masks ? f.strip_masks[t.range_start + e] : 0xFu;
            if (kmask != 0u) { // (a zero byte: not fetched)
                vid = f.point_list[t.range_start + e];
                se  = stage_entry(f.recs, vid, mode);
            }
        }
        __syncthreads(); // the previous round's readers are done with the slab and the masks
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned long long m = __ballot((kmask >> k) & 1u);
            if (t.lane == 0) s.s_mask[t.wave][k] = m;
        }
        if (kmask != 0u) { // (rows nobody reaches are never read)
            s.s_rows[0][t.tid] = se.a;
            s.s_rows[1][t.tid] = se.b;
        }
        before(vid);
        __syncthreads();
        for (uint32_t i = 0; i < 4u; ++i) {
            const uint32_t w = BACK ? 3u - i : i;
            if (__builtin_amdgcn_ballot_w64(lo + w * 64u < t.last) == 0ull) { // past every pixel of the strip
                if (BACK) continue;
                break;
            }
            unsigned long long m = s.s_mask[w][t.wave];
            m = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(m >> 32)) << 32) |
                (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m);
            while (m != 0ull) { // scalar loop control; the next position in walk order
                const uint32_t l = BACK ? 63u - (uint32_t)__builtin_clzll(m) : (uint32_t)__ffsll((long long)m) - 1u;
                m &= ~(1ull << l);
                const uint32_t idx = w * 64u + l;
                const float4   ea = s.s_rows[0][idx], eb = s.s_rows[1][idx];
                body(idx, lo + idx, ea, eb);
            }
        }
        after();
    }
}

inline uint32_t maps_grid(const CamParams& cp, const uint32_t* tile_order)
{
    return tile_order ? cp.grid_x * cp.grid_y : render_grid_size(cp.grid_x, cp.grid_y);
}
} // namespace kept_walk
} // namespace lcgs
