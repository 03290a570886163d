// features.hip -- caller-supplied per-splat feature channels of the last keep-state frame, blended like colour, and their
// backward (the contract is in include/lcgs_hip.h).  The general case of maps.hip's normal channel: the vector
// comes from the caller (P x K floats, row-major, the context's row order), has K components, and its own gradient goes back
// to the caller.  The reference has nothing of the kind: its renderer composites colour only.
//
// Both kernels are kept_walk.hpp's walk, CH channels at a time: blockIdx.y is the chunk, channels [CH y, CH y + CH) of the K,
// the tail chunk padded with zeros inside the kernel (nothing is read past a row's K floats, nothing past plane K - 1 of a
// map; a row of odd K is not 16-byte aligned, so rows are read float by float).
//   k_render_features<CH>                    k_render_normals' walk with CH accumulators F_c = sum fl(w f_c), the multiply
//                                            and the add separate operations (-ffp-contract=off) in list order from 0.  The
//                                            round's entries' chunk is staged into LDS in the `before` hook and read back as
//                                            wave-uniform broadcasts in the body.  No MFMA: an f32 MFMA is an fmaf chain.
//   k_render_features_backward<CH, GEOM, FGRAD>
//                                            back to front, Qr / Bd as in k_render_maps_backward.  val = sum_c f_c g_c[p] with
//                                            the lane's CH incoming gradients in registers.  GEOM: the six geometry sums,
//                                            flushed with k_render_maps_backward's arithmetic for slots 0-5 and ADDED to
//                                            grads2d (no value slot is written).  FGRAD: CH sums w g_c[p], flushed by float
//                                            atomics to dL_dfeatures[row K + c].  GEOM = false (the geometry is frozen) drops
//                                            Bd, q, the six sums and the staged features; FGRAD = false drops the CH sums.
// Thresholds are constants for the derivative, exactly as in backward.hip: the 0.99 cap passes nothing, a saturated pixel stops.
#include "kept_walk.hpp"

namespace lcgs
{
using namespace kept_walk;
namespace
{

// the chunk of the staged entry's feature row into LDS row `dst` (CH floats), zeros past channel K - 1
template <int CH>
__device__ __forceinline__ void stage_feature_chunk(const float* __restrict__ features, size_t row, uint32_t K, uint32_t c0,
                                                    float* __restrict__ dst)
{
    const float* src = features + row * K + c0;
#pragma unroll
    for (int c = 0; c < CH; ++c) dst[c] = (c0 + (uint32_t)c < K) ? src[c] : 0.0f;
}

template <int CH>
__global__ void __launch_bounds__(256) k_render_features(KeptFrame f, const uint32_t* __restrict__ vis_index, uint32_t K,
                                                         const float* __restrict__ features, float* __restrict__ feature_map)
{
    __shared__ WalkShared s_walk;
    __shared__ __attribute__((aligned(16))) float s_feat[256][CH]; // the round's staged entries' chunk
    TileWalk t;
    if (!tile_prologue(f, s_walk, t)) return; // (a frame that drew nothing walks nothing: the map is zero)
    const uint32_t c0 = blockIdx.y * (uint32_t)CH;

    float T = 1.0f, F[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) F[c] = 0.0f;
    walk_rounds<false>(
        f, s_walk, t, kDepthZ,
        [&](uint32_t vid) {
            if (vid != 0xFFFFFFFFu) stage_feature_chunk<CH>(features, vis_index[vid], K, c0, s_feat[t.tid]);
        },
        [&](uint32_t idx, uint32_t pos, const float4& ea, const float4& eb) {
            const EntryEval v = eval_entry(ea, eb, t.pxf, t.pyf, pos, t.last);
            if (__builtin_amdgcn_ballot_w64(v.cand) == 0ull) return;
            const EntryBlend b = blend_entry(eb, v);
            if (b.blended) {
                const float wgt = T * b.alpha;
#pragma unroll
                for (int c = 0; c < CH; ++c) F[c] = F[c] + wgt * s_feat[idx][c];
                T = T * (1.0f - b.alpha);
            }
        },
        [] {});
    if (t.inside) {
        const size_t plane = (size_t)f.cp.width * f.cp.height;
#pragma unroll
        for (int c = 0; c < CH; ++c)
            if (c0 + (uint32_t)c < K) feature_map[(size_t)(c0 + c) * plane + t.pix] = F[c];
    }
}

constexpr uint32_t pow2_at_least(uint32_t n)
{
    uint32_t p = 1u;
    while (p < n) p <<= 1;
    return p;
}

template <int CH, bool GEOM, bool FGRAD>
__global__ void __launch_bounds__(256) k_render_features_backward(KeptFrame f, const uint32_t* __restrict__ vis_index, uint32_t K,
                                                                  const float* __restrict__ features,
                                                                  const float* __restrict__ dL_dfeature_map,
                                                                  float* __restrict__ grads2d, float* __restrict__ dL_dfeatures)
{
    static_assert(GEOM || FGRAD, "a walk with nothing to sum");
    constexpr int         kGeom  = GEOM ? 6 : 0;
    constexpr int         kSums  = kGeom + (FGRAD ? CH : 0);
    constexpr uint32_t    kLanes = pow2_at_least((uint32_t)kSums); // the flush's lanes per entry
    __shared__ WalkShared s_walk;
    __shared__ float      s_acc[kSums][256]; // the round's sums over the tile's pixels, per entry
    __shared__ uint32_t   s_vid[256];        // the entry's splat (dense id); ~0: nothing staged
    __shared__ uint32_t   s_row[FGRAD ? 256 : 1]; // FGRAD: its scene row
    __shared__ __attribute__((aligned(16))) float s_feat[GEOM ? 256 : 1][CH]; // GEOM: the entry's chunk

    if (f.d_counts[1] == 0u) return; // nothing drawn: final_T / n_contrib are not this frame's, every gradient is zero
    TileWalk t;
    if (!tile_prologue(f, s_walk, t)) return;
    const uint32_t c0      = blockIdx.y * (uint32_t)CH;
    const float    T_final = t.inside ? f.final_T[t.pix] : 0.0f;
    float          g[CH]; // the lane's incoming gradients of the chunk, zeros past channel K - 1 and outside the image
    {
        const size_t plane = (size_t)f.cp.width * f.cp.height;
#pragma unroll
        for (int c = 0; c < CH; ++c)
            g[c] = (t.inside && c0 + (uint32_t)c < K) ? dL_dfeature_map[(size_t)(c0 + c) * plane + t.pix] : 0.0f;
    }

    // per-pixel recurrences, back to front (backward.hip): Qr = prod (1 - alpha) over the entries walked so far, over T_final;
    // Bd = (feature chunk composited behind the current splat) . dL/dpixel -- nothing lies behind the last entry
    float          Qr = 1.0f / T_final, Bd = 0.0f;
    const uint32_t acc_base = (uint32_t)(uintptr_t)&s_acc[0][0]; // low half of a flat LDS address = LDS offset
    const bool     row_head = (t.lane & 15u) == 0u;

    walk_rounds<true>(
        f, s_walk, t, kDepthZ,
        [&](uint32_t vid) {
            s_vid[t.tid] = vid;
#pragma unroll
            for (int k = 0; k < kSums; ++k) s_acc[k][t.tid] = 0.0f;
            if (vid != 0xFFFFFFFFu) {
                const uint32_t row = vis_index[vid];
                if constexpr (FGRAD) s_row[t.tid] = row;
                if constexpr (GEOM) stage_feature_chunk<CH>(features, row, K, c0, s_feat[t.tid]);
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
            float       s[kSums];
            if constexpr (GEOM) {
                float val = 0.0f; // f_i . dL/dF[p] over the chunk: the per-pixel value of entry i
#pragma unroll
                for (int c = 0; c < CH; ++c) val = val + s_feat[idx][c] * g[c];
                const float d   = val - Bd; // (value - what lies behind) . dL/dpixel
                const float dLa = d * Tn;
                Bd              = __builtin_fmaf(a, d, Bd);
                // the 0.99 cap passes no gradient; selected behind the product (G is arbitrary bits off the candidate lanes)
                const float q = (b.blended & (b.oG < 0.99f)) ? b.G * dLa : 0.0f; // dL/dopacity
                s[0] = q * v.dx;
                s[1] = q * v.dy;
                s[2] = s[0] * v.dx;
                s[3] = s[0] * v.dy;
                s[4] = s[1] * v.dy;
                s[5] = q;
            }
            if constexpr (FGRAD) {
#pragma unroll
                for (int c = 0; c < CH; ++c) s[kGeom + c] = wgt * g[c]; // dL/df_i,c
            }
#pragma unroll
            for (int k = 0; k < kSums; ++k) s[k] = row16_sum(s[k]);
            if (row_head) {
                // (a raw ds_add_f32, as in backward.hip: the compiler would wrap atomicAdd in a per-lane scan loop)
                const uint32_t addr = acc_base + idx * 4u;
#pragma unroll
                for (int k = 0; k < kSums; ++k)
                    asm volatile("ds_add_f32 %0, %1 offset:%2" ::"v"(addr), "v"(s[k]), "n"(k * 256 * 4) : "memory");
            }
        },
        [&] {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the raw LDS adds above have landed
            __syncthreads();
            // ---- flush the round: kLanes consecutive lanes own one entry's sums, so a wave instruction covers contiguous bytes
            // of a few rows instead of 64 different rows
            for (uint32_t cidx = t.tid; cidx < 256u * kLanes; cidx += 256u) {
                const uint32_t k = cidx & (kLanes - 1u), idx = cidx / kLanes;
                const uint32_t vid = s_vid[idx];
                if (k >= (uint32_t)kSums || vid == 0xFFFFFFFFu) continue;
                float s = s_acc[k][idx];
                if (GEOM && k < 6u) {
                    // sums -> gradients: d/dmean = -opacity conic (S q dx, S q dy), d/dconic = opacity (-1/2, -1, -1/2) (S q dx dx, ...)
                    const float4 ea = s_walk.s_rows[0][idx], eb = s_walk.s_rows[1][idx];
                    if (k < 5u) {
                        if (k < 2u) {
                            const float ca = -2.0f * ea.z, cc = -2.0f * ea.w, s0 = s_acc[0][idx], s1 = s_acc[1][idx];
                            s = (k == 0u) ? -(ca * s0 + eb.x * s1) : -(cc * s1 + eb.x * s0);
                        } else {
                            s *= (k == 3u) ? -1.0f : -0.5f;
                        }
                        s *= eb.z;
                    }
                    if (s != 0.0f) atomicAdd(&grads2d[(size_t)vid * kG2D + k], s);
                    continue;
                }
                if constexpr (FGRAD) { // the chunk's own sums: the caller's rows (channels past K - 1 are padding)
                    const uint32_t c = c0 + (k - (uint32_t)kGeom);
                    if (c < K && s != 0.0f) atomicAdd(&dL_dfeatures[(size_t)s_row[idx] * K + c], s);
                }
            }
        });
}

template <int CH>
void launch_forward(const KeptFrame& f, const FeatureChannel& fc, float* feature_map, hipStream_t stream)
{
    const dim3 grid(maps_grid(f.cp, f.tile_order), ((uint32_t)fc.K + CH - 1) / CH);
    hipLaunchKernelGGL((k_render_features<CH>), grid, dim3(256), 0, stream, f, fc.vis_index, (uint32_t)fc.K, fc.features,
                       feature_map);
}

template <int CH>
void launch_backward(const KeptFrame& f, const FeatureChannel& fc, float* grads2d, hipStream_t stream)
{
    const dim3 grid(maps_grid(f.cp, f.tile_order), ((uint32_t)fc.K + CH - 1) / CH);
    const uint32_t K = (uint32_t)fc.K;
    if (grads2d && fc.dL_dfeatures)
        hipLaunchKernelGGL((k_render_features_backward<CH, true, true>), grid, dim3(256), 0, stream, f, fc.vis_index, K,
                           fc.features, fc.dL_dfeature_map, grads2d, fc.dL_dfeatures);
    else if (grads2d)
        hipLaunchKernelGGL((k_render_features_backward<CH, true, false>), grid, dim3(256), 0, stream, f, fc.vis_index, K,
                           fc.features, fc.dL_dfeature_map, grads2d, nullptr);
    else
        hipLaunchKernelGGL((k_render_features_backward<CH, false, true>), grid, dim3(256), 0, stream, f, fc.vis_index, K,
                           fc.features, fc.dL_dfeature_map, nullptr, fc.dL_dfeatures);
}

} // namespace

int features_chunk_width(int K, int forced)
{
    if (forced == 4 || forced == 8 || forced == 16) return forced;
    return K <= 4 ? 4 : (K <= 8 ? 8 : 16);
}

void launch_render_features(const KeptFrame& f, const FeatureChannel& fc, float* feature_map, int ch, hipStream_t stream)
{
    if (f.cp.grid_x * f.cp.grid_y == 0) return;
    switch (ch) {
    case 4: launch_forward<4>(f, fc, feature_map, stream); break;
    case 8: launch_forward<8>(f, fc, feature_map, stream); break;
    default: launch_forward<16>(f, fc, feature_map, stream); break;
    }
}

void launch_render_features_backward(const KeptFrame& f, const FeatureChannel& fc, float* grads2d, int ch, hipStream_t stream)
{
    if (f.cp.grid_x * f.cp.grid_y == 0 || (!grads2d && !fc.dL_dfeatures)) return;
    switch (ch) {
    case 4: launch_backward<4>(f, fc, grads2d, stream); break;
    case 8: launch_backward<8>(f, fc, grads2d, stream); break;
    default: launch_backward<16>(f, fc, grads2d, stream); break;
    }
}

} // namespace lcgs
