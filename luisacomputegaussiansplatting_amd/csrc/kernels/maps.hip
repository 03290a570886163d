// maps.hip -- depth, alpha and depth-distortion maps of the last keep-state frame, and their backward (the
// contract is in include/lcgs_hip.h).  None of the maps exists in the reference: its renderer composites colour only.
//
// The walk kernels are kept_walk.hpp's walk -- one workgroup per 16x16 tile in the renderer's schedule, wave k = the tile's
// 8x8 quadrant k, one pixel per lane, the KEPT per-tile list in rounds of 256 staged entries up to the tile's largest n_contrib
// -- with their own accumulators, per-entry body and flush:
//   k_render_maps           front to back.  A pixel takes entries up to its own n_contrib, so the forward's saturation test is
//                           not repeated (the saturating entry lies past it); power, alpha and the two skips are the walk's
//                           restatement of the forward's, and the T update is its expression too (-ffp-contract=off), which
//                           makes alpha = sum w and depth = sum fl(w v) the tests' binary32 CPU restatement's bit for bit.
//   k_render_distortion     the same walk with three accumulators: with u = fl(v - center), A = sum w, M1 = sum fl(w u),
//                           M2 = sum fl(w fl(u u)) and one store fl(fl(A M2) - fl(M1 M1)) per pixel -- the closed form of
//                           sum_{i<j} w_i w_j (v_i - v_j)^2, three accumulated channels the CPU restatement composites as the
//                           colour (u, 1, u u).
//   k_render_maps_backward  back to front like k_render_backward, with the two channels (v, dL/dD) and (1, dL/dA) folded into
//                           one per-entry scalar.  Seven per-pixel terms per entry (q dx, q dy, q dx dx, q dx dy, q dy dy, q,
//                           w dL/dD) are summed over the strip's 64 lanes -- four DPP butterfly steps inside each 16-lane row,
//                           then one LDS add per row -- and over the four waves in a per-round LDS accumulator; the round's
//                           totals leave as at most seven global float atomics per (tile, splat), eight consecutive lanes per
//                           splat row.  It ADDS to grads2d slots 0-5 and 9.
//                           DIST = true adds the distortion channel: the pixel's A, M1, M2 are first re-derived in registers
//                           by the forward's own front-to-back walk over the same LDS (walk_distortion_sums: the forward's
//                           bits, nothing cached, nothing taken as input), then d dist / d w_i = M2 + u_i (A u_i - 2 M1) joins
//                           the per-entry scalar as a third per-pixel "value" and 2 w_i (A u_i - M1) dL/ddist joins the
//                           w dL/dD sum.  Still seven sums per (tile, splat) and the same flush.  DIST = false is the
//                           two-channel kernel, operation for operation.
//                           NRM = true adds the normal channel: n_i . dL/dN[p] joins the per-entry scalar as one more
//                           per-pixel value, and three more sums w_i dL/dN_c[p] join the seven -- ten per (tile, splat), the
//                           same butterfly, LDS accumulator and flush (sixteen lanes per entry instead of eight); the three
//                           leave as float atomics into the per-row dL/dn workspace, not into grads2d.
//   k_maps_depth_to_pos     one lane per on-screen row: dL/dpos += slot 9 x dv/dz x front.
//   k_splat_normals         one lane per on-screen row: the row's view-space normal (include/lcgs_hip.h: the shortest axis'
//                           column of rot_from_quat, turned to face the camera, taken to view space), the axis and the flip in
//                           the fourth word; clears the row's dL/dn slot when the backward asks.  Every row a walk reads is written.
//   k_render_normals        k_render_maps' walk with three accumulators N_c = sum fl(w n_c); the entry's normal is staged into
//                           LDS in the round's `before` hook.
//   k_normals_to_rot        one lane per on-screen row: dL/drotq += (dc/dq)^T (+-)(right gn0 + up gn1 + front gn2).
// Thresholds are constants for the derivative, exactly as in backward.hip: the 0.99 cap passes nothing, a saturated pixel stops.
#include "kept_rows.hpp"
#include "kept_walk.hpp"

namespace lcgs
{
using namespace kept_walk;
namespace
{

__global__ void __launch_bounds__(256) k_render_maps(KeptFrame f, int mode, float* __restrict__ depth_map,
                                                     float* __restrict__ alpha_map)
{
    __shared__ WalkShared s_walk;
    TileWalk              t;
    if (!tile_prologue(f, s_walk, t)) return; // (a frame that drew nothing walks nothing: both maps are zero)

    float T = 1.0f, A = 0.0f, D = 0.0f;
    walk_rounds<false>(
        f, s_walk, t, mode, [](uint32_t) {},
        [&](uint32_t, uint32_t pos, const float4& ea, const float4& eb) {
            const EntryEval v = eval_entry(ea, eb, t.pxf, t.pyf, pos, t.last);
            if (__builtin_amdgcn_ballot_w64(v.cand) == 0ull) return;
            const EntryBlend b = blend_entry(eb, v);
            if (b.blended) {
                const float wgt = T * b.alpha;
                A               = A + wgt;
                D               = D + wgt * eb.w;
                T               = T * (1.0f - b.alpha);
            }
        },
        [] {});
    if (t.inside) {
        if (depth_map) depth_map[t.pix] = D;
        if (alpha_map) alpha_map[t.pix] = A;
    }
}

// the distortion map's three accumulated channels of the lane's pixel, front to back in list order from 0 (k_render_maps'
// walk); ONE statement of them for the forward and for the backward's pre-walk, which must reproduce the forward's bits
__device__ __forceinline__ void walk_distortion_sums(const KeptFrame& f, WalkShared& s_walk, const TileWalk& t, int mode,
                                                     float center, float& A, float& M1, float& M2)
{
    float T = 1.0f, a0 = 0.0f, m1 = 0.0f, m2 = 0.0f;
    walk_rounds<false>(
        f, s_walk, t, mode, [](uint32_t) {},
        [&](uint32_t, uint32_t pos, const float4& ea, const float4& eb) {
            const EntryEval v = eval_entry(ea, eb, t.pxf, t.pyf, pos, t.last);
            if (__builtin_amdgcn_ballot_w64(v.cand) == 0ull) return;
            const EntryBlend b = blend_entry(eb, v);
            if (b.blended) {
                const float wgt = T * b.alpha, u = eb.w - center;
                a0              = a0 + wgt;
                m1              = m1 + wgt * u;
                m2              = m2 + wgt * (u * u);
                T               = T * (1.0f - b.alpha);
            }
        },
        [] {});
    A = a0, M1 = m1, M2 = m2;
}

__global__ void __launch_bounds__(256) k_render_distortion(KeptFrame f, int mode, float center, float* __restrict__ dist_map)
{
    __shared__ WalkShared s_walk;
    TileWalk              t;
    if (!tile_prologue(f, s_walk, t)) return; // (a frame that drew nothing walks nothing: the map is zero)
    float A, M1, M2;
    walk_distortion_sums(f, s_walk, t, mode, center, A, M1, M2);
    if (t.inside) dist_map[t.pix] = A * M2 - M1 * M1;
}

// the fourth word of a row's normal: bits 0-1 the axis k, bit 2 the flip
constexpr uint32_t kNrmFlipBit = 4u;

__global__ void __launch_bounds__(256) k_splat_normals(CamParams cp, const uint32_t* __restrict__ vis_index,
                                                       const uint32_t* __restrict__ d_counts, const float* __restrict__ pos,
                                                       const float* __restrict__ scale, const float* __restrict__ rotq,
                                                       float4* __restrict__ normals, float4* __restrict__ dL_dn)
{
    const uint32_t V = d_counts[0];
    for (uint32_t vid = blockIdx.x * 256u + threadIdx.x; vid < V; vid += gridDim.x * 256u) {
        const size_t i = vis_index[vid];
        const float  s[3] = { scale[3 * i + 0], scale[3 * i + 1], scale[3 * i + 2] };
        uint32_t     k = 0u;
        if (s[1] < s[k]) k = 1u;
        if (s[2] < s[k]) k = 2u;
        float R[3][3];
        rot_from_quat(rotq[4 * i + 1], rotq[4 * i + 2], rotq[4 * i + 3], rotq[4 * i + 0], R); // stored (w, x, y, z)
        float       c0 = R[k][0], c1 = R[k][1], c2 = R[k][2];
        const float d0 = pos[3 * i + 0] - cp.campos[0], d1 = pos[3 * i + 1] - cp.campos[1], d2 = pos[3 * i + 2] - cp.campos[2];
        const float t  = (c0 * d0 + c1 * d1) + c2 * d2;
        const bool  flip = t > 0.0f; // (0 and NaN: unflipped)
        if (flip) c0 = -c0, c1 = -c1, c2 = -c2;
        float4 n;
        n.x = (cp.right[0] * c0 + cp.right[1] * c1) + cp.right[2] * c2;
        n.y = (cp.up[0] * c0 + cp.up[1] * c1) + cp.up[2] * c2;
        n.z = (cp.front[0] * c0 + cp.front[1] * c1) + cp.front[2] * c2;
        n.w = __uint_as_float(k | (flip ? kNrmFlipBit : 0u));
        normals[vid] = n;
        if (dL_dn) dL_dn[vid] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

__global__ void __launch_bounds__(256) k_render_normals(KeptFrame f, const float4* __restrict__ normals,
                                                        float* __restrict__ normal_map)
{
    __shared__ WalkShared s_walk;
    __shared__ float4     s_nrm[256]; // the round's staged entries' normals
    TileWalk              t;
    if (!tile_prologue(f, s_walk, t)) return; // (a frame that drew nothing walks nothing: the map is zero)

    float T = 1.0f, N0 = 0.0f, N1 = 0.0f, N2 = 0.0f;
    walk_rounds<false>(
        f, s_walk, t, kDepthZ,
        [&](uint32_t vid) {
            if (vid != 0xFFFFFFFFu) s_nrm[t.tid] = normals[vid];
        },
        [&](uint32_t idx, uint32_t pos, const float4& ea, const float4& eb) {
            const EntryEval v = eval_entry(ea, eb, t.pxf, t.pyf, pos, t.last);
            if (__builtin_amdgcn_ballot_w64(v.cand) == 0ull) return;
            const EntryBlend b = blend_entry(eb, v);
            if (b.blended) {
                const float4 n   = s_nrm[idx];
                const float  wgt = T * b.alpha;
                N0               = N0 + wgt * n.x;
                N1               = N1 + wgt * n.y;
                N2               = N2 + wgt * n.z;
                T                = T * (1.0f - b.alpha);
            }
        },
        [] {});
    if (t.inside) {
        const size_t plane = (size_t)f.cp.width * f.cp.height;
        normal_map[t.pix]             = N0;
        normal_map[plane + t.pix]     = N1;
        normal_map[2 * plane + t.pix] = N2;
    }
}

template <bool DIST, bool NRM>
__global__ void __launch_bounds__(256) k_render_maps_backward(KeptFrame f, int mode, float center,
                                                              const float* __restrict__ dL_ddepth,
                                                              const float* __restrict__ dL_dalpha,
                                                              const float* __restrict__ dL_ddist, float* __restrict__ grads2d,
                                                              const float* __restrict__ dL_dnormal,
                                                              const float4* __restrict__ normals, float* __restrict__ dL_dn)
{
    constexpr int         kSums  = NRM ? 10 : 7;
    constexpr uint32_t    kLanes = NRM ? 16u : 8u; // the flush's lanes per entry
    __shared__ WalkShared s_walk;
    __shared__ float      s_acc[kSums][256]; // the round's sums over the tile's pixels, per entry
    __shared__ uint32_t   s_vid[256];        // the entry's splat (dense id); ~0: nothing staged
    __shared__ float4     s_nrm[NRM ? 256 : 1]; // NRM: the entry's normal

    if (f.d_counts[1] == 0u) return; // nothing drawn: final_T / n_contrib are not this frame's, every gradient is zero
    TileWalk t;
    if (!tile_prologue(f, s_walk, t)) return;
    const float T_final = t.inside ? f.final_T[t.pix] : 0.0f;
    const float gd = (t.inside && dL_ddepth) ? dL_ddepth[t.pix] : 0.0f;
    const float ga = (t.inside && dL_dalpha) ? dL_dalpha[t.pix] : 0.0f;
    // the distortion channel: the pixel's own sums, as the forward accumulated them, before anything is walked backwards
    float gq = 0.0f, dA = 0.0f, dM1 = 0.0f, dM2 = 0.0f;
    if constexpr (DIST) {
        gq = (t.inside && dL_ddist) ? dL_ddist[t.pix] : 0.0f;
        walk_distortion_sums(f, s_walk, t, mode, center, dA, dM1, dM2);
    }
    float gn0 = 0.0f, gn1 = 0.0f, gn2 = 0.0f;
    if constexpr (NRM) {
        if (t.inside) {
            const size_t plane = (size_t)f.cp.width * f.cp.height;
            gn0 = dL_dnormal[t.pix], gn1 = dL_dnormal[plane + t.pix], gn2 = dL_dnormal[2 * plane + t.pix];
        }
    }

    // per-pixel recurrences, back to front (backward.hip): Qr = prod (1 - alpha) over the entries walked so far, over T_final;
    // Bd = (value composited behind the current splat) . dL/dpixel over the two channels -- nothing lies behind the last entry
    float          Qr = 1.0f / T_final, Bd = 0.0f;
    const uint32_t acc_base = (uint32_t)(uintptr_t)&s_acc[0][0]; // low half of a flat LDS address = LDS offset
    const bool     row_head = (t.lane & 15u) == 0u;

    walk_rounds<true>(
        f, s_walk, t, mode,
        [&](uint32_t vid) {
            s_vid[t.tid] = vid;
#pragma unroll
            for (int g = 0; g < kSums; ++g) s_acc[g][t.tid] = 0.0f;
            if constexpr (NRM) {
                if (vid != 0xFFFFFFFFu) s_nrm[t.tid] = normals[vid];
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
            const float wgt = a * Tn;
            float       val = __builtin_fmaf(eb.w, gd, ga), gv = wgt * gd; // value . dL/dpixel; dL/dvalue
            if constexpr (DIST) { // d dist / d w_i as a third per-pixel value, d dist / d u_i beside w dL/dD
                const float u = eb.w - center, au = dA * u;
                val = val + gq * (dM2 + u * (au - 2.0f * dM1));
                gv  = gv + (2.0f * gq) * (wgt * (au - dM1));
            }
            if constexpr (NRM) { // n_i . dL/dN[p] as one more per-pixel value
                const float4 n = s_nrm[idx];
                val            = val + ((n.x * gn0 + n.y * gn1) + n.z * gn2);
            }
            const float d   = val - Bd; // (value - what lies behind) . dL/dpixel
            const float dLa = d * Tn;
            Bd              = __builtin_fmaf(a, d, Bd);
            // the 0.99 cap passes no gradient; selected behind the product (G is arbitrary bits off the candidate lanes)
            const float q = (b.blended & (b.oG < 0.99f)) ? b.G * dLa : 0.0f; // dL/dopacity
            float       s[kSums];
            s[0] = q * v.dx;
            s[1] = q * v.dy;
            s[2] = s[0] * v.dx;
            s[3] = s[0] * v.dy;
            s[4] = s[1] * v.dy;
            s[5] = q;
            s[6] = gv;
            if constexpr (NRM) s[7] = wgt * gn0, s[8] = wgt * gn1, s[9] = wgt * gn2; // dL/dn_i
#pragma unroll
            for (int g = 0; g < kSums; ++g) s[g] = row16_sum(s[g]);
            if (row_head) {
                // (a raw ds_add_f32, as in backward.hip: the compiler would wrap atomicAdd in a per-lane scan loop)
                const uint32_t addr = acc_base + idx * 4u;
#pragma unroll
                for (int g = 0; g < kSums; ++g)
                    asm volatile("ds_add_f32 %0, %1 offset:%2" ::"v"(addr), "v"(s[g]), "n"(g * 256 * 4) : "memory");
            }
        },
        [&] {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the raw LDS adds above have landed
            __syncthreads();
            // ---- flush the round: eight consecutive lanes own one entry's row (seven of them add), so a wave instruction covers
            // contiguous bytes of a few rows instead of 64 different rows
            for (uint32_t cidx = t.tid; cidx < 256u * kLanes; cidx += 256u) {
                const uint32_t g = cidx & (kLanes - 1u), idx = cidx / kLanes;
                const uint32_t vid = s_vid[idx];
                if (g < (uint32_t)kSums && vid != 0xFFFFFFFFu) {
                    // sums -> gradients: d/dmean = -opacity conic (S q dx, S q dy), d/dconic = opacity (-1/2, -1, -1/2) (S q dx dx, ...)
                    const float4 ea = s_walk.s_rows[0][idx], eb = s_walk.s_rows[1][idx];
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
                    if (NRM && g >= 7u) { // the normal channel's sums: the per-row dL/dn workspace, not a grads2d slot
                        if (s != 0.0f) atomicAdd(&dL_dn[(size_t)vid * 4u + (g - 7u)], s);
                        continue;
                    }
                    if (s != 0.0f) atomicAdd(&grads2d[(size_t)vid * kG2D + (g < 6u ? g : (uint32_t)kG2DValueSlot)], s);
                }
            }
        });
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
        const float  gz = depth_value_backward(recs[vid].depth, mode, gv); // view z = front . pos + tz
        const size_t o  = 3 * (size_t)vis_index[vid];
        dL_dpos[o + 0] += gz * cp.front[0];
        dL_dpos[o + 1] += gz * cp.front[1];
        dL_dpos[o + 2] += gz * cp.front[2];
    }
}

__global__ void __launch_bounds__(256) k_normals_to_rot(CamParams cp, const uint32_t* __restrict__ vis_index,
                                                        const uint32_t* __restrict__ d_counts, const float* __restrict__ rotq,
                                                        const float4* __restrict__ normals, const float4* __restrict__ dL_dn,
                                                        float* __restrict__ dL_drotq)
{
    const uint32_t V = d_counts[0];
    for (uint32_t vid = blockIdx.x * 256u + threadIdx.x; vid < V; vid += gridDim.x * 256u) {
        const float4 gn = dL_dn[vid];
        if (gn.x == 0.0f && gn.y == 0.0f && gn.z == 0.0f) continue;
        const uint32_t bits = __float_as_uint(normals[vid].w), k = bits & 3u;
        const float    sg   = (bits & kNrmFlipBit) ? -1.0f : 1.0f;
        // dL/dc = +-(right gn0 + up gn1 + front gn2): the view rotation's transpose, the flip a constant
        const float g0 = sg * ((cp.right[0] * gn.x + cp.up[0] * gn.y) + cp.front[0] * gn.z);
        const float g1 = sg * ((cp.right[1] * gn.x + cp.up[1] * gn.y) + cp.front[1] * gn.z);
        const float g2 = sg * ((cp.right[2] * gn.x + cp.up[2] * gn.y) + cp.front[2] * gn.z);
        const size_t o = 4 * (size_t)vis_index[vid];
        const float  w = rotq[o + 0], x = rotq[o + 1], y = rotq[o + 2], z = rotq[o + 3];
        float        gw, gx, gy, gz; // (dc/dq)^T dL/dc from column k of rot_from_quat
        if (k == 0u) {      // (1 - 2yy - 2zz, 2xy + 2zw, 2xz - 2yw)
            gx = 2.0f * (y * g1 + z * g2);
            gy = 2.0f * ((x * g1 - w * g2) - 2.0f * y * g0);
            gz = 2.0f * ((w * g1 + x * g2) - 2.0f * z * g0);
            gw = 2.0f * (z * g1 - y * g2);
        } else if (k == 1u) { // (2xy - 2zw, 1 - 2xx - 2zz, 2yz + 2xw)
            gx = 2.0f * ((y * g0 + w * g2) - 2.0f * x * g1);
            gy = 2.0f * (x * g0 + z * g2);
            gz = 2.0f * ((y * g2 - w * g0) - 2.0f * z * g1);
            gw = 2.0f * (x * g2 - z * g0);
        } else {              // (2xz + 2yw, 2yz - 2xw, 1 - 2xx - 2yy)
            gx = 2.0f * ((z * g0 - w * g1) - 2.0f * x * g2);
            gy = 2.0f * ((w * g0 + z * g1) - 2.0f * y * g2);
            gz = 2.0f * (x * g0 + y * g1);
            gw = 2.0f * (y * g0 - x * g1);
        }
        dL_drotq[o + 0] += gw;
        dL_drotq[o + 1] += gx;
        dL_drotq[o + 2] += gy;
        dL_drotq[o + 3] += gz;
    }
}

} // namespace

void launch_render_maps(const KeptFrame& f, int mode, float* depth, float* alpha, hipStream_t stream)
{
    if (f.cp.grid_x * f.cp.grid_y == 0) return;
    hipLaunchKernelGGL(k_render_maps, dim3(maps_grid(f.cp, f.tile_order)), dim3(256), 0, stream, f, mode, depth, alpha);
}

void launch_render_distortion(const KeptFrame& f, int mode, float center, float* dist, hipStream_t stream)
{
    if (f.cp.grid_x * f.cp.grid_y == 0) return;
    hipLaunchKernelGGL(k_render_distortion, dim3(maps_grid(f.cp, f.tile_order)), dim3(256), 0, stream, f, mode, center, dist);
}

void launch_render_maps_backward(const KeptFrame& f, int mode, const float* dL_ddepth, const float* dL_dalpha, float* grads2d,
                                 hipStream_t stream, float center, const float* dL_ddist, const NormalChannel* nrm)
{
    if (f.cp.grid_x * f.cp.grid_y == 0) return;
    const dim3 grid(maps_grid(f.cp, f.tile_order));
    if (nrm) { // the normal channel: ten sums per (tile, splat)
        if (dL_ddist)
            hipLaunchKernelGGL((k_render_maps_backward<true, true>), grid, dim3(256), 0, stream, f, mode, center, dL_ddepth,
                               dL_dalpha, dL_ddist, grads2d, nrm->dL_dnormal, nrm->normals, nrm->dL_dn);
        else
            hipLaunchKernelGGL((k_render_maps_backward<false, true>), grid, dim3(256), 0, stream, f, mode, 0.0f, dL_ddepth,
                               dL_dalpha, nullptr, grads2d, nrm->dL_dnormal, nrm->normals, nrm->dL_dn);
    } else if (dL_ddist)
        hipLaunchKernelGGL((k_render_maps_backward<true, false>), grid, dim3(256), 0, stream, f, mode, center, dL_ddepth,
                           dL_dalpha, dL_ddist, grads2d, nullptr, nullptr, nullptr);
    else // (the two-channel kernel: no pre-walk, lcgs_render_backward_maps' arithmetic)
        hipLaunchKernelGGL((k_render_maps_backward<false, false>), grid, dim3(256), 0, stream, f, mode, 0.0f, dL_ddepth,
                           dL_dalpha, nullptr, grads2d, nullptr, nullptr, nullptr);
}

size_t splat_normals_bytes(int64_t rows) { return (size_t)(rows > 1 ? rows : 1) * sizeof(float4); }

void launch_splat_normals(const KeptRows& r, float4* normals, float4* dL_dn, hipStream_t stream)
{
    hipLaunchKernelGGL(k_splat_normals, dim3(grid_256(r.hint)), dim3(256), 0, stream, r.cp, r.vis_index, r.d_counts, r.pos,
                       r.scale, r.rotq, normals, dL_dn);
}

void launch_render_normals(const KeptFrame& f, const float4* normals, float* normal_map, hipStream_t stream)
{
    if (f.cp.grid_x * f.cp.grid_y == 0) return;
    hipLaunchKernelGGL(k_render_normals, dim3(maps_grid(f.cp, f.tile_order)), dim3(256), 0, stream, f,
                       normals, normal_map);
}

void launch_normals_to_rot(const KeptRows& r, const float4* normals, const float4* dL_dn, float* dL_drotq, hipStream_t stream)
{
    hipLaunchKernelGGL(k_normals_to_rot, dim3(grid_256(r.hint)), dim3(256), 0, stream, r.cp, r.vis_index, r.d_counts, r.rotq,
                       normals, dL_dn, dL_drotq);
}

void launch_maps_depth_to_pos(const KeptRows& r, int mode, float* dL_dpos, hipStream_t stream)
{
    hipLaunchKernelGGL(k_maps_depth_to_pos, dim3(grid_256(r.hint)), dim3(256), 0, stream, r.cp, r.vis_index, r.d_counts, r.recs,
                       r.grads2d, mode, dL_dpos);
}

} // namespace lcgs
