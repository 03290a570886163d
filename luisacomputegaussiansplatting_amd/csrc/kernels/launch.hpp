// launch.hpp -- host-callable launchers of every HIP kernel in the library.
// All launchers only enqueue work on `stream`; none allocates or synchronises.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gs_math.hpp"

namespace lcgs
{
struct KeptFrame; // kept_walk.hpp: what a walk of the last keep-state frame's kept lists reads
struct KeptRows;  // kept_rows.hpp: what a pass with one lane per on-screen row of a kept frame reads

// workgroups of 256 lanes for `elements` items: one item per lane, at least one workgroup, at most 65536 (kernels stride beyond)
inline unsigned grid_256(int64_t elements)
{
    const int64_t b = (elements + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

// ---- stage_kernels.hip : one kernel per reference shader (buffers in the reference's layouts) ----
void launch_sh_process(int P, int deg, const CamParams& cp, const float* pos, const float* sh, float* color,
                       hipStream_t stream);
void launch_project(int P, const CamParams& cp, bool use_focal, const float* pos, const float* scale,
                    const float* rotq, float scale_modifier, float* means_2d, float* depth, float* covs_2d,
                    hipStream_t stream);
// hole_flag (optional, device word, cleared by the caller): set when a splat claims pair slots that copy_with_keys leaves
// unwritten (radius <= 0 with tiles > 0: a NaN covariance) -- only then does the reference's zero-fill of the pair buffers matter
// hole_flag (nullable): set to hole_mark (a value the caller has not used before: no zero-fill per frame) when a splat claims pair
// slots its copy_with_keys will not write.  flags (nullable, flags_len >= P bytes): flags[i] = splat i claims pair slots
// (tiles_touched[i] > 0), zeros behind P -- the splatter's compaction input
void launch_allocate_tiles(int P, const CamParams& cp, bool use_focal, const float* depth, float* means_2d,
                           float* covs_2d, uint32_t* tiles_touched, int32_t* radii, hipStream_t stream,
                           uint32_t* hole_flag = nullptr, uint32_t hole_mark = 1u, uint8_t* flags = nullptr, size_t flags_len = 0);
void launch_copy_with_keys(int P, const CamParams& cp, const float* means_2d, const uint32_t* offsets,
                           const int32_t* radii, const float* depth, uint64_t* keys, uint32_t* values,
                           hipStream_t stream);
// the splatter's sort-before-duplicate (abi_stages.cpp lcgs_tile_splat_forward): which splats claim pair slots, their depth
// keys, a gather through the sorted order, and copy_with_keys over the splats IN THAT ORDER
void launch_gather_depth_keys(int n, const uint32_t* vis, const float* depth, uint32_t* keys, uint32_t* vals, hipStream_t stream);
void launch_gather_u32(int n, const uint32_t* order, const uint32_t* src, uint32_t* dst, hipStream_t stream);
void launch_copy_with_keys_ordered(int n, const CamParams& cp, const float* means_2d, const uint32_t* offsets_sorted,
                                   const int32_t* radii, const float* depth, const uint32_t* order, uint64_t* keys,
                                   uint32_t* values, hipStream_t stream);
// the same pairs as launch_copy_with_keys_ordered (with order = the ascending list of the splats that claim slots: as
// launch_copy_with_keys), written by workgroups that own 1024 consecutive OUTPUT slots (coalesced stores, bounded work per
// workgroup).  The n sources are the splats that CLAIM slots (tiles > 0, radius > 0), source e = splat order[e]; offsets: the
// inclusive sums of their tile counts, L = offsets[n - 1] (known on the host).  win_first: copy_with_keys_windows_bytes(L).
void   launch_copy_with_keys_balanced(int n, const CamParams& cp, const float* means_2d, const uint32_t* offsets,
                                      const int32_t* radii, const float* depth, const uint32_t* order, uint64_t* keys,
                                      uint32_t* values, uint32_t L, uint32_t* win_first, hipStream_t stream,
                                      const uint32_t* dbits_of_source = nullptr); // (nullable) source e's depth bits, in source order
size_t copy_with_keys_windows_bytes(uint32_t L);
void launch_get_ranges_u64(int64_t L, const uint64_t* keys, uint32_t* ranges, hipStream_t stream);

// ---- scan.hip : DeviceScan::InclusiveSum<uint> ----
size_t scan_temp_bytes(int64_t n); // of `temp`, for either sum type
void   launch_inclusive_sum_u32(const uint32_t* in, uint32_t* out, int64_t n, void* temp, hipStream_t stream);
// out[i] = in[0] + ... + in[i] in u64
void   launch_inclusive_sum_u64(const uint32_t* in, uint64_t* out, int64_t n, void* temp, hipStream_t stream);
// element count read from device memory (*d_n <= n_cap)
void   launch_inclusive_sum_u32_dyn(const uint32_t* in, uint32_t* out, int64_t n_cap, const uint32_t* d_n, void* temp,
                                    hipStream_t stream);

// ---- render.hip : per-tile front-to-back compositing (gs_tile_splatter/shader.cpp:171-288) ----
// Reference-layout inputs (means_2d[2P] pixel, conic[3P], opacity[P], color[3P]).
void launch_render_forward_aos(const CamParams& cp, const float bg[3], const uint32_t* ranges,
                               const uint32_t* point_list, const float* means_2d, const float* conic,
                               const float* opacity, const float* color, float* img, float* final_T,
                               uint32_t* n_contrib, hipStream_t stream);

// ---- fused_forward.hip : the one-submission frame ----
// Packed per-visible-splat record written by the fused preprocess and gathered by the renderer.
struct __attribute__((aligned(16))) SplatRecord {
    float    mx, my;   // pixel mean                       (float4 #0)
    float    ca, cb;   // conic xx, xy
    float    cc, opac; // conic yy, opacity                (float4 #1)
    float    r, g;     // colour
    float    b;        //                                  (float4 #2)
    float    depth;    // view-space z
    uint32_t rect_xy;  // rect_min.x | rect_min.y << 16    (tile units)
    uint32_t rect_wh;  // width | height << 16             (tile units); tiles touched = w * h
};
static_assert(sizeof(SplatRecord) == 48, "SplatRecord must be 48 bytes");

// ---- the cull pass and the depth sort it feeds
// Where the cull pass leaves the depth sort's first per-chunk digit counts (pair_sort.hip depth_sort_first_pass).
// splats per cull workgroup = slots per slab = keys per chunk of the depth sort's first pass (both files assert it)
constexpr int kCullChunkSplats = 2048;
struct TieOrder; // tie_order.hpp
struct DepthSortFirstPass {
    uint32_t  mask;       // first digit = key & mask
    uint32_t  row_stride; // counts[digit * row_stride + chunk]
    uint32_t* counts;
};
// table: the start of the sort's workspace, or a table of depth_sort_first_counts_bytes(P) that only the cull pass and the
// sort's first pass touch (launch_depth_sort_from_chunks first_counts) -- a cull pass may then run beside the later passes
DepthSortFirstPass depth_sort_first_pass(int64_t P, void* table);
size_t depth_sort_first_counts_bytes(int64_t P);
int    cull_chunk_count(int P); // 2048-splat chunks: slab = 2048 x 16 B per chunk, chunk_info / chunk_base one entry each
void launch_set_frame_params(const FrameParams& fp, FrameParams* d_fp, hipStream_t stream);
// d_fp (nullable): when non-NULL the kernels take camera / bg / scale_modifier from device memory (graph replay)
// slab[chunk * 2048 + r] = {depth bits, splat index, pruned rect} of the chunk's r-th survivor (index order);
// chunk_info[chunk] = {survivors, reference tiles_touched}
// bound4 (nullable; ignored when radii are asked for): the scene's {position, extent bound} rows (launch_cull_bound) --
// phase 1 then reads 16 instead of 40 bytes per splat; same survivors, same slabs
void launch_cull_compact(int P, const CamParams& cp, float scale_modifier, const FrameParams* d_fp, const float* pos,
                         const float* scale, const float* rotq, const float* opacity, int32_t* radii, uint4* slab,
                         uint2* chunk_info, const DepthSortFirstPass& first, hipStream_t stream,
                         const float4* bound4 = nullptr);
// out[i] = {pos[i], |R(q_i)|-bound x max |scale_i|}: the camera-independent inputs of the cull pass's phase-1 test
void launch_cull_bound(int64_t P, const float* pos, const float* scale, const float* rotq, float4* out, hipStream_t stream);
// diagnostics: *mismatches += rows of `rows` that are not what launch_cull_bound would write for the arrays now (bit compare)
void launch_cull_bound_verify(int64_t P, const float* pos, const float* scale, const float* rotq, const float4* rows,
                              unsigned long long* mismatches, hipStream_t stream);
// d_counts: [0] V (splats emitting >= 1 pair), [1] reference num_rendered (both written by the depth sort's first
//           row-scan launch), [2] pairs emitted, [3] overflow flag, [4] pairs wanted (before clamping to capacity)
void launch_depth_sort_from_chunks(int64_t P, int64_t v_hint, const uint4* slab, const uint2* chunk_info,
                                   uint32_t* chunk_base, uint32_t* keys_a, uint32_t* keys_b, uint32_t* vals_a,
                                   uint32_t* vals_b, uint32_t* vis_index, uint2* rects, uint32_t* d_counts, void* sort_ws,
                                   hipStream_t stream, hipEvent_t fork = nullptr,
                                   // re-ordered scenes: equal depths come out in FILE order (tie_order.hpp); the sorted
                                   // values then carry a file-index tag above their id_bits -- readers mask it off
                                   const TieOrder* tie = nullptr,
                                   // first_pass_only: stop behind the compaction (vis_index, rects, V, num_rendered)
                                   bool first_pass_only = false,
                                   // the cull pass's digit counts when they are not at the start of sort_ws
                                   uint32_t* first_counts = nullptr);
void launch_fix_equal_depth_order(uint32_t* keys, uint32_t* vals, uint32_t* scratch_k, uint32_t* scratch_v, int64_t n_cap,
                                  int64_t v_hint, const TieOrder& tie, hipStream_t stream);
// ---- splat ownership: a frame from RECEIVED records instead of the context's own cull pass
// rows_out[i] = vis[i] + row_first for i < *d_count
void launch_rows_global(const uint32_t* vis, const uint32_t* d_count, uint32_t row_first, uint32_t* rows_out, int64_t hint,
                        hipStream_t stream);
// n records (ascending global row order) -> the depth sort's input (keys = depth bits, vals = position [| file-index tag]),
// rects, vis_index = rows; d_counts[0] = n, [1] = the sum of the pruned rects' tiles (non-zero iff anything is drawn)
void launch_unpack_records(int64_t n, const SplatRecord* recs, const uint32_t* rows, const uint32_t* perm, uint32_t id_bits,
                           uint32_t tag_shift, uint32_t* keys, uint32_t* vals, uint2* rects, uint32_t* vis_index,
                           uint32_t* d_counts, uint32_t P, uint32_t grid_x, uint32_t grid_y, hipStream_t stream);
// ... the same from PADDED per-owner segments whose true counts are on the device (fused_forward.hip k_unpack_records_seg)
constexpr int kMaxOwnerSegs = 16; // = LCGS_MAX_OWNER_VIEWS (one view slot per rank of an ownership step)
struct OwnerSegs {
    uint32_t n = 0;                      // owners
    uint32_t off[kMaxOwnerSegs + 1] = {}; // owner o's segment = positions [off[o], off[o + 1])
};
void launch_unpack_records_seg(const OwnerSegs& segs, const uint32_t* table, uint32_t view, const SplatRecord* recs,
                               const uint32_t* rows, const uint32_t* perm, uint32_t id_bits, uint32_t tag_shift, uint32_t* keys,
                               uint32_t* vals, uint2* rects, uint32_t* vis_index, uint32_t* d_counts, uint32_t* overflow, uint32_t P,
                               uint32_t grid_x, uint32_t grid_y, hipStream_t stream);
// *overflow |= 2 when the frame's pair buffers were too small (d_counts[3])
void launch_owner_pair_verdict(const uint32_t* d_counts, uint32_t* overflow, hipStream_t stream);
struct PairSortFirstPass;
size_t expand_ws_bytes(int P_cap);
// v_hint: expected survivor count (bounds the launch; larger live counts are handled by chunk striding)
// returns true iff the first-pass counts were written
bool launch_expand(int P_cap, int64_t v_hint, int64_t l_hint, uint32_t* d_counts, uint32_t grid_x,
                   const uint32_t* order, const uint2* rects, uint2* rects_sorted, uint32_t* pair_keys,
                   uint32_t* pair_vals, uint32_t capacity, uint32_t* ws, hipStream_t stream,
                   const PairSortFirstPass* first_pass = nullptr, // non-NULL: also leave the tile sort's first counts
                   uint32_t id_mask = 0xFFFFFFFFu); // the bits of an `order` entry that are the dense id

// ---- pair_sort.hip : stable radix sort of (u32 key, u32 value) pairs, count in device memory ----
size_t pair_sort_ws_bytes(int64_t n_cap);
// ping-pongs a -> b -> a ...; returns 0 if the result ended in (keys_a, vals_a), 1 if in (keys_b, vals_b)
// first_hist_done: pass 0's chunk counts are already in ws (see pair_sort_first_pass)
int launch_pair_sort_u32(uint32_t* keys_a, uint32_t* keys_b, uint32_t* vals_a, uint32_t* vals_b, const uint32_t* d_n,
                         int64_t n_cap, int64_t grid_hint, int begin_bit, int end_bit, void* ws, hipStream_t stream,
                         bool first_hist_done = false);
// Lets the kernel that writes the keys also count them: counts[digit * row_stride + chunk] over all 256 digits,
// chunk = position / keys_per_chunk, digit = (key >> shift) & mask -- exactly what the sort's first k_hist would write
// for the same (n_cap, grid_hint, begin_bit, end_bit, ws).
struct PairSortFirstPass {
    int       shift;
    uint32_t  mask;
    int       keys_per_chunk; // 2048 or 4096
    uint32_t* counts;
    uint32_t  row_stride;
    bool      valid;
};
PairSortFirstPass pair_sort_first_pass(int64_t n_cap, int64_t grid_hint, int begin_bit, int end_bit, void* ws);
// stage-level 64-bit sort on the same kernels: n host-known, inputs intact, (keys_tmp, vals_tmp) = scratch of n elements,
// ws = pair_sort_ws_bytes(n)
void launch_pair_sort_u64_preserve(const uint64_t* keys_in, const uint32_t* vals_in, uint64_t* keys_out,
                                   uint32_t* vals_out, uint64_t* keys_tmp, uint32_t* vals_tmp, int64_t n, int begin_bit,
                                   int end_bit, void* ws, hipStream_t stream);
void launch_build_records(int P_cap, int sh_deg, const CamParams& cp, float scale_modifier, const FrameParams* d_fp,
                          const float* pos,
                          const float* scale, const float* rotq, const float* sh, const float* opacity,
                          const uint32_t* vis_index, const uint32_t* d_counts, SplatRecord* recs, hipStream_t stream,
                          const uint16_t* sh_half = nullptr, // non-NULL: f16 coefficient rows (degree 3 only)
                          float4* shjac = nullptr);          // non-NULL: 3 x float4 per survivor for the backward
bool build_records_writes_jacobian(int sh_deg, const float* sh, bool half);
void launch_sh_to_half(int64_t n, const float* src, uint16_t* dst, hipStream_t stream);
// L_hint sizes the launch (larger live counts are strided); l_cap = entries the key buffer holds
void launch_get_ranges_u32(int64_t L_hint, uint32_t l_cap, uint32_t* d_counts, const uint32_t* keys, uint32_t* ranges,
                           const uint32_t* scan_error_flag, hipStream_t stream, hipEvent_t done = nullptr,
                           // (non-NULL: d_counts[0] and [1] are copied there, for a renderer that outlives the counter block)
                           uint32_t* frame_words = nullptr);
void launch_map_to_index(int64_t L_cap, const uint32_t* d_counts, const uint32_t* list_vid, const uint32_t* vis_index,
                         uint32_t* list_idx, hipStream_t stream);

// optimiser step (train.hip): five attribute arrays each for gradients, raw parameters, Adam moments, activated values
struct AdamArrays {
    float *pos, *scale, *rotq, *sh, *opacity;
};
struct AdamRates {
    float pos, sh_dc, sh_rest, opacity, scale, rot;
};
// the step's scalars (the update itself and the per-attribute chain rules: adam_rows.hpp)
struct AdamStep {
    float b1, b2, eps, inv_bc1, inv_sqrt_bc2;
};
AdamStep make_adam_step(float beta1, float beta2, float eps, int step);
// row_list != NULL: only rows row_list[0 .. *d_row_count) are updated (launch sized for row_hint rows)
// grad_compact (row_list only): gradient row r belongs to splat row_list[r] (lcgs_render_backward_compact's layout)
void launch_adam_step(int64_t P, int sh_floats, const uint32_t* row_list, const uint32_t* d_row_count, int64_t row_hint,
                      const AdamArrays& grad, const AdamArrays& raw, const AdamArrays& m, const AdamArrays& v,
                      const AdamArrays& act, const AdamRates& lr, float beta1, float beta2, float eps, int step,
                      hipStream_t stream, bool grad_compact = false);
// ---- densify.hip : adaptive density control (statistics of a step, the clone / split / prune rewrite, opacity reset) ----
// one thread per on-screen row of the last keep-state frame (KeptRows, kept_rows.hpp): the screen-space positional gradient
// (grads2d rows, pixel units -> NDC), the visit count and the largest reference radius
void launch_densify_stats(const KeptRows& r, float* grad_accum, uint32_t* denom, int32_t* max_radii, hipStream_t stream);
struct DensifyRule {
    float   grad_threshold, dense_extent /* percent_dense x scene_extent */, huge_extent /* 0.1 x scene_extent */, min_opacity;
    int32_t max_screen_size;
};
// emit[i] = output rows of source row i (0, 1, 2), action[i] = 0 prune, 1 keep, 2 clone, 3 split
void launch_densify_classify(int64_t P, const DensifyRule& rule, const float* raw_scale, const float* raw_opacity,
                             const float* grad_accum, const uint32_t* denom, const int32_t* max_radii, uint32_t* emit,
                             uint8_t* action, hipStream_t stream);
// incl = inclusive sums of emit.  o_act.pos / .sh may alias o_raw's.  noise: [P][2][3] or NULL (Philox keyed by seed, row, child)
void launch_densify_scatter(int64_t P, int sh_floats, const uint8_t* action, const uint32_t* incl, const AdamArrays& raw,
                            const AdamArrays& m, const AdamArrays& v, const AdamArrays& o_raw, const AdamArrays& o_m,
                            const AdamArrays& o_v, const AdamArrays& o_act, float split_drop, const float* noise, uint64_t seed,
                            uint32_t* src_row, hipStream_t stream);
// raw = min(raw, ceiling), m = v = 0, act = sigmoid(raw)
void launch_opacity_reset(int64_t P, float ceiling, float* raw, float* m, float* v, float* act, hipStream_t stream);
// ---- mcmc.hip : 3DGS-MCMC density control (relocation, growth, SGLD noise, the L1 regulariser) ----
constexpr int      kMcmcMaxN        = 51;          // the binomial table's rows: n_max <= 51
constexpr uint32_t kMcmcTagRelocate = 0x4D430001u; // word 2 of the Philox counters (philox.hpp)
constexpr uint32_t kMcmcTagAdd      = 0x4D430002u;
constexpr uint32_t kMcmcTagNoise    = 0x4D430003u;
// w[i] = dead ? 0 : (uint32_t)(sigmoid(raw opacity) * 2^24), dead = !(sigmoid > min_opacity); dead (nullable) = 0 | 1;
// src_row (nullable) = i
void launch_mcmc_weights(int64_t P, float min_opacity, const float* raw_opacity, uint32_t* w, uint32_t* dead, uint32_t* src_row,
                         hipStream_t stream);
// dead_list[dead_incl[i] - 1] = i for every dead row (dead_incl: inclusive sums of dead)
void launch_mcmc_dead_list(int64_t P, const uint32_t* dead, const uint32_t* dead_incl, uint32_t* dead_list, hipStream_t stream);
// draws 0 .. D - 1 (D = *d_n if d_n, else n_host; the launch is sized for n_launch): draw_src[j] = src_in ? src_in[j] : the
// smallest i with cdf[i] > mulhi64(u_j, T), u_j = Philox(seed; j low, j high, tag, 0) words 0 | 1 << 32, T = cdf[P - 1]
// (cdf: the u64 inclusive sums of w, launch_inclusive_sum_u64); count[draw_src[j]] += 1.  status[0] |= 1: an entry of src_in is >= P or has weight 0 (the draw is skipped); |= 2: T == 0
// (no draw is made)
void launch_mcmc_draw(int64_t P, int64_t n_launch, int64_t n_host, const uint32_t* d_n, const uint64_t* cdf, const uint32_t* w,
                      const uint32_t* src_in, uint64_t seed, uint32_t tag, uint32_t* draw_src, uint32_t* count, uint32_t* status,
                      hipStream_t stream);
struct McmcRule {
    float min_opacity;
    int   n_max;
};
// K1: draw j writes row dst = dead_list ? dead_list[j] : dst_first + j from source draw_src[j]; src_row (nullable)
// [dead_list ? dst : j] = the source.  K2: every row with count > 0, in place.  Run K1 first: it reads the sources' ORIGINAL
// scale and opacity.
void launch_mcmc_place(int64_t D, int sh_floats, const uint32_t* dead_list, int64_t dst_first, const uint32_t* draw_src,
                       const uint32_t* count, const McmcRule& rule, const AdamArrays& raw, const AdamArrays& m, const AdamArrays& v,
                       const AdamArrays& act, uint32_t* src_row, hipStream_t stream);
void launch_mcmc_sources(int64_t P, int sh_floats, const uint32_t* count, const McmcRule& rule, const AdamArrays& raw,
                         const AdamArrays& m, const AdamArrays& v, const AdamArrays& act, hipStream_t stream);
// pos += (gain * g(o)) * Sigma eps in place (act_pos too when it is another array); noise: [P][3] or NULL (Philox keyed by seed,
// row, step)
void launch_mcmc_noise(int64_t P, float gain, float k, float x0, const float* raw_opacity, const float* raw_scale,
                       const float* raw_rotq, const float* noise, uint64_t seed, uint32_t step, float* raw_pos, float* act_pos,
                       hipStream_t stream);
// d_opacity[i] += add_opacity, d_scale[i][c] += add_scale
void launch_mcmc_regularize(int64_t P, float add_opacity, float add_scale, float* d_opacity, float* d_scale, hipStream_t stream);
// ---- filter3d.hip : Mip-Splatting's 3-D smoothing filter (sampling rates over the training views, apply, backward) ----
constexpr int kFilter3dViewChunk = 64; // views per launch of the accumulate pass: its table travels in the kernel's arguments
struct Filter3dView {                  // what the pass reads of a view: gs_math.hpp view_transform's rows, cam_clamp's limits
    float right[3], tx, up[3], ty, front[3], tz;
    float limx, limy; // 1.3f * tanfovx, 1.3f * tanfovy
};
struct Filter3dViews {
    Filter3dView v[kFilter3dViewChunk];
};
static_assert(sizeof(Filter3dViews) <= 3840, "the table and the pass's other arguments must fit the 4 KiB of kernel arguments");
// min_z[i] = min(min_z[i], view z of row i) over the first num_views (<= kFilter3dViewChunk) views that see the row
void launch_filter3d_accumulate(int64_t P, const float* pos, int num_views, const Filter3dViews& views, float* min_z,
                                hipStream_t stream);
// word (one u32, zeroed by the caller on the stream): receives the largest finite min_z as an ordered key; then
// filter[i] = ((finite min_z[i] ? min_z[i] : zmax) / max_focal) * sqrt(0.2), all 0 when nothing is finite
void launch_filter3d_finalize(int64_t P, const float* min_z, float max_focal, uint32_t* word, float* filter, hipStream_t stream);
void launch_filter3d_apply(int64_t P, const float* scale, const float* opacity, const float* filter, float* scale_out,
                           float* opacity_out, hipStream_t stream);
// in place on the gradient rows; rows != NULL: gradient row r < *d_count belongs to row rows[r], the launch is sized by P
void launch_filter3d_backward(int64_t P, const float* scale, const float* opacity, const float* filter, const uint32_t* rows,
                              const uint32_t* d_count, float* g_scale, float* g_opacity, hipStream_t stream);
// ---- transform.hip : a similarity transform of a scene's activated arrays, SH bands rotated; the crop box's keep mask ----
// include/lcgs_hip.h's lcgs_similarity_plan, member for member (abi_transform.cpp asserts the sizes): it travels in the kernels' arguments
struct TransformPlan {
    float M[9], t[3], s, q[4], D1[9], D2[25], D3[49];
};
static_assert(sizeof(TransformPlan) == 400, "100 floats");
constexpr int kTransformTileRows = 64; // rows of coefficients a workgroup of the SH pass stages: counts around its multiples are edge cases
// every `out` that is not NULL from its `in` (the same pointer, or disjoint from it); an opacity or a degree-0 coefficient array
// is a plain copy, and none at all in place
void launch_scene_transform(int64_t P, int sh_degree, const TransformPlan& plan, const float* pos, const float* scale,
                            const float* rotq, const float* sh, float* pos_out, float* scale_out, float* rotq_out, float* sh_out,
                            hipStream_t stream);
// keep[i] = every |(M pos_i + t)_k| <= half[k]
void launch_box_keep_mask(int64_t P, const TransformPlan& plan, const float* pos, const float half[3], uint8_t* keep,
                          hipStream_t stream);
// ---- tsdf.hip : TSDF fusion of depth maps into a dense volume, marching tetrahedra on the Kuhn split ----
constexpr int kTsdfViewChunk = 42; // = LCGS_TSDF_VIEW_CHUNK: views per launch of the integrate pass, their table in the kernel's arguments
struct TsdfView {                  // what the pass reads of a view: gs_math.hpp view_transform's rows, the projection, the maps
    float        right[3], tx, up[3], ty, front[3], tz;
    float        inv_tanx, inv_tany;
    int          W, H;
    const float *depth, *alpha, *image; // alpha / image: NULL = the view has none
};
struct TsdfViews {
    TsdfView v[kTsdfViewChunk];
};
static_assert(sizeof(TsdfViews) <= 3840, "the table and the pass's other arguments must fit the 4 KiB of kernel arguments");
struct TsdfGrid { // the lattice of include/lcgs_hip.h's lcgs_tsdf_volume
    float origin[3], voxel;
    int   nx, ny, nz;
};
// every sample through the first num_views (<= kTsdfViewChunk) views of the table, in order; rgb may be NULL
void launch_tsdf_integrate(const TsdfGrid& g, float* tsdf, float* weight, float* rgb, float trunc, float depth_max, float alpha_min,
                           int num_views, const TsdfViews& views, hipStream_t stream);
// The mesh passes.  word[s] (zeroed by the caller): bits 0-6 the crossing edges whose lower sample is s (bit dir - 1), bits 8-11
// the triangle count of the cell whose lowest corner is s.  The cell pass ORs into it (integer OR: order-free).
void launch_tsdf_mesh_cells(const TsdfGrid& g, const float* tsdf, const float* weight, float weight_min, uint32_t* word,
                            hipStream_t stream);
// vcount[s] = popcount of the edge bits, tcount[s] = the triangle count; totals[0] += sum vcount, totals[1] += sum tcount (u64,
// zeroed by the caller; integer adds: order-free)
void launch_tsdf_mesh_counts(int64_t n, const uint32_t* word, uint32_t* vcount, uint32_t* tcount, unsigned long long* totals,
                             hipStream_t stream);
// vincl / tincl: the inclusive sums of vcount / tcount.  vertices 3 floats each (vertex_rgb nullable), triangles 3 indices each
void launch_tsdf_mesh_vertices(const TsdfGrid& g, const float* tsdf, const float* rgb, const uint32_t* word, const uint32_t* vincl,
                               float* vertices, float* vertex_rgb, hipStream_t stream);
void launch_tsdf_mesh_triangles(const TsdfGrid& g, const float* tsdf, const uint32_t* word, const uint32_t* vincl,
                                const uint32_t* tincl, uint32_t* triangles, hipStream_t stream);
// ---- loss.hip : the 3DGS photometric loss, (1 - lambda) L1 + lambda (1 - SSIM), and its gradient ----
// Both passes tile a channel into 32 x 16 outputs, one workgroup each; partial sums are indexed by workgroup.
int64_t photometric_workgroups(int W, int H);
// pass A: per-pixel ssim and |x - y| summed per workgroup into partials[wg] = { sum ssim, sum |x - y| }; abc (nullable:
// evaluation only) = the three planes [3][3 H W] of d ssim / d mu1 (expanded), / d sigma1^2, / d sigma12
void launch_photometric_stats(int W, int H, const float* img, const float* target, float* abc, double* partials,
                              hipStream_t stream);
// pass B: dL[i] = (1 - lambda) sign(x - y) / n - (lambda / n) (G*a + 2 x G*b + y G*c), every element written once
// (lambda == 0: abc is not read)
void launch_photometric_grad(int W, int H, const float* img, const float* target, const float* abc, float lambda, float* dL,
                             hipStream_t stream);
// the partials summed in index order -> loss[0]; terms (nullable) = { L1, SSIM }
void launch_photometric_finish(int W, int H, const double* partials, float lambda, float* loss, float* terms,
                               hipStream_t stream);
// the normal-consistency loss of a W x H frame's maps (include/lcgs_hip.h has the definition): one workgroup per 32 x 16 tile,
// one binary64 partial each (normal_consistency_workgroups of them), summed in index order by the photometric loss's finish
// step -> loss[0] = scale * sum of the interior pixels' terms, scale = weight / ((W - 2)(H - 2)).  The three gradients are all
// NULL (evaluation only: the same loss bits) or all written whole, zeros at the border included.
int64_t normal_consistency_workgroups(int W, int H);
void launch_normal_consistency(int W, int H, double tanx, double tany, double scale, double alpha_min, const float* depth,
                               const float* alpha, const float* normal, float* dL_ddepth, float* dL_dalpha, float* dL_dnormal,
                               double* partials, float* loss, hipStream_t stream);
// ---- depth_prior.hip : the Pearson and aligned-L1 losses of a depth map against a prior, with their gradients ----
// (include/lcgs_hip.h has the definition.)  32 x 16 tiles anchored at the patch grid's anchor, every tile inside one group.
constexpr int kDepthPriorTileW = 32, kDepthPriorTileH = 16;
constexpr int kDepthPriorRec = 8; // doubles of a group's record (means, coefficients, counted flag)
struct DepthPriorGrid {
    int W, H;
    int ox, oy;             // the grid's anchor is pixel (-ox, -oy); 0 for the whole image
    int gtx, gty;           // tiles of a group along x and y
    int groups_x, groups_y; // groups; every tile of every group is launched
};
// patch 0: one group, the image; else 32, 64 or 128 with 0 <= patch_x, patch_y < patch (checked by the caller)
DepthPriorGrid depth_prior_grid(int W, int H, int patch, int patch_x, int patch_y);
inline int64_t depth_prior_groups(const DepthPriorGrid& g) { return (int64_t)g.groups_x * g.groups_y; }
inline int64_t depth_prior_tiles(const DepthPriorGrid& g) { return depth_prior_groups(g) * g.gtx * g.gty; }
struct DepthPriorTerm {
    int    kind;  // LCGS_DEPTH_PRIOR_PEARSON / _L1
    bool   given; // LCGS_DEPTH_ALIGN_GIVEN: (scale, shift) are the caller's, no statistics
    bool   patch; // patch mode, however many groups the grid has on this image: d_stats reports no fit
    double scale, shift, weight, alpha_min;
};
// the call's arrays inside one block of `doubles` binary64 numbers at `base` (base NULL: only the size is wanted)
struct DepthPriorWorkspace {
    double *hdr, *rec, *gsum, *tile1, *tile2, *l1_part;
    size_t  doubles;
};
DepthPriorWorkspace depth_prior_workspace(const DepthPriorGrid& g, double* base);
// mask nullable; dL_ddepth and dL_dalpha both NULL: evaluation only (the same loss bits); stats nullable, 4 floats
void launch_depth_prior(const DepthPriorGrid& g, const DepthPriorTerm& term, const float* depth, const float* alpha, const float* prior,
                        const uint8_t* mask, float* dL_ddepth, float* dL_dalpha, float* loss, float* stats, const DepthPriorWorkspace& w,
                        hipStream_t stream);
// ---- bilagrid.hip : per-view bilateral-grid colour correction -- slice, its two gradients, total variation ----
// A view's grid is [12][gl][gh][gw] floats (include/lcgs_hip.h has the definition); images are CHW.
constexpr int kBilagridTileW = 32, kBilagridTileH = 16; // the pixel tile of a workgroup of the per-pixel passes
struct BilagridDims {
    int gw, gh, gl;
};
// the per-pixel pass, one workgroup per tile: dL_dout == NULL -> out = the sliced image; else out = dL/dimg
void launch_bilagrid_pixels(int W, int H, const float* grid, const BilagridDims& d, const float* img, const float* dL_dout,
                            float* out, hipStream_t stream);
// dL/dgrid as a gather, one workgroup per (vertex column, row slice) for gl <= 8 and per (vertex, row slice) for deeper grids;
// the slice count depends on the dimensions only.  More than one slice: `partials` holds bilagrid_grid_partial_doubles(d)
// doubles, summed in slice order by a second launch.  Every element of dL_dgrid is written.
int    bilagrid_grid_slices(const BilagridDims& d);
size_t bilagrid_grid_partial_doubles(const BilagridDims& d);
void   launch_bilagrid_grid_grad(int W, int H, const BilagridDims& d, const float* img, const float* dL_dout, float* dL_dgrid,
                                 double* partials, hipStream_t stream);
// the TV term of num_grids grids: one binary64 partial per workgroup (bilagrid_tv_workgroups of them), summed in index order
// -> loss[0]; dL_dgrids NULL: evaluation only, the same loss bits
int64_t bilagrid_tv_workgroups(int64_t num_grids, const BilagridDims& d);
void    launch_bilagrid_tv(const float* grids, int64_t num_grids, const BilagridDims& d, double weight, float* dL_dgrids,
                           double* partials, float* loss, hipStream_t stream);
// backward.hip: the per-splat half of the backward with the on-screen-only Adam update applied where the gradients are
// formed (degree 3, frames that kept the colour Jacobian): no gradient rows are written at all
// (r.shjac is not NULL; r.opacity is read for an antialiased frame, before the lane's update of the activated row)
void launch_preprocess_backward_adam(const KeptRows& r, const AdamArrays& raw, const AdamArrays& m, const AdamArrays& v,
                                     const AdamArrays& act, const AdamRates& lr, const AdamStep& a, hipStream_t stream);
// byte offsets, inside one vertex record, of the 59 wanted float columns (pos3 dc3 rest45 opacity scale3 rot4)
struct PlyColumns {
    uint32_t offset[59];
};
// records [first, first + count) of a PLY payload chunk already in device memory -> activated scene arrays
void launch_ply_activate(const unsigned char* raw, int64_t first, int64_t count, uint32_t stride, const PlyColumns& cols,
                         float* pos, float* scale, float* rotq, float* sh, float* opacity, hipStream_t stream);
// spatial (Morton) order of a scene, ingest.hip: position moments (7 doubles per block: sums, sums of squares, count),
// 30-bit Morton keys + identity values, row gather through a permutation
int  pos_moment_blocks();
void launch_pos_moments(int64_t P, const float* pos, double* partial, hipStream_t stream);
void launch_morton_keys(int64_t P, const float* pos, const float lo[3], const float cells_per_unit[3], uint32_t* keys,
                        uint32_t* vals, hipStream_t stream);
// (the same keys, the grid in device memory: d_grid[0..2] = lo, d_grid[3..5] = cells per unit)
void launch_morton_keys(int64_t P, const float* pos, const float* d_grid, uint32_t* keys, uint32_t* vals, hipStream_t stream);
void launch_gather_rows(int64_t rows, int row_floats, const uint32_t* perm, const float* src, float* dst, hipStream_t stream);
// ---- init.hip : a scene from a point cloud -- exact 3-nearest-neighbour mean squared distances, 3DGS's initial rows ----
constexpr int kKnnChunk = 256; // = LCGS_KNN_CHUNK: sorted points per chunk = lanes per query workgroup
// what the box reduction leaves on the device: the Morton grid of the valid points (lo, cells per unit) and their count
struct KnnGrid {
    float    lo[3], cells[3];
    uint32_t num_valid, pad;
};
size_t knn_box_partial_bytes();
// exact min / max and count of the finite points -> *grid (two launches, no atomics)
void launch_knn_grid(int64_t n, const float* pos, void* partial, KnnGrid* grid, hipStream_t stream);
// sorted[r] = (pos[perm[r]], bits(perm[r])); boxes[2 c], boxes[2 c + 1] = lo, hi of chunk c's finite points (+inf, -inf: none)
void launch_knn_gather_boxes(int64_t n, const float* pos, const uint32_t* perm, float4* sorted, float4* boxes, hipStream_t stream);
// dist2[original index] of every point, as include/lcgs_hip.h defines it
void launch_knn_query(int64_t n, const float4* sorted, const float4* boxes, const KnnGrid* grid, float* dist2, hipStream_t stream);
// 3DGS's create_from_pcd rows in the caller's order (act.pos / act.sh may alias raw's)
void launch_init_rows(int64_t n, int sh_floats, const float* pos, const float* rgb, const float* dist2, float min_dist2,
                      float raw_opacity, const AdamArrays& raw, const AdamArrays& act, hipStream_t stream);
// longest-list-first tile schedule for the renderers (order[G], a scheduling hint only)
void launch_tile_order(const uint32_t* ranges, uint32_t G, uint32_t* order, hipStream_t stream, uint32_t grid_x = 0,
                       uint32_t list_shift = 0);
void launch_blend_exp(const float* x, float* out, int64_t n, hipStream_t stream);
void launch_render_forward_rec(const CamParams& cp, const float bg[3], const uint32_t* ranges,
                               const uint32_t* point_list, const SplatRecord* recs, float* img, float* final_T,
                               uint32_t* n_contrib, const uint32_t* d_counts, const FrameParams* d_fp,
                               const uint32_t* tile_order, hipStream_t stream, uint8_t* strip_masks = nullptr,
                               hipEvent_t done = nullptr, uint32_t* work_counter = nullptr, uint32_t persistent_wgs = 0,
                               // frames that keep backward state: the renderer also clears the 2-D gradient rows
                               // (12 floats x d_counts[0]) and the backward's counter block as a side job
                               float* g2d_zero = nullptr, uint32_t* bwd_counters = nullptr);
// work_counter + persistent_wgs: a bounded grid of persistent_wgs workgroups that pull tiles from *work_counter (which
// must be zero when the kernel starts) instead of one workgroup per tile -- caps the wave slots the renderer holds
// strip_masks[list position] = the four per-strip reach bits of that entry (written when final_T / n_contrib are
// kept); the backward takes them instead of repeating the tests

// ---- comm_pack.hip : the opt-in f16 transport of the gradient all-reduce (host/comm.cpp) ----
// |max| of n floats, atomically max-ed into *d_out_bits (float bits; zero it first)
void launch_absmax(const float* x, size_t n, uint32_t* d_out_bits, hipStream_t stream);
// dst[i] = srcs[0][i] + ... + srcs[n - 1][i] (n <= 16; dst may be one of the sources): the loopback transport's reductions
void launch_sum_sources(const float* const* srcs, int n, size_t count, float* dst, hipStream_t stream);
// five power-of-two scales (and their inverses) from the five all-reduced magnitudes: max * scale <= 16384 / world
void launch_transport_scales(const float* d_absmax5, int world, float* d_scale5, float* d_inv5, hipStream_t stream);
void launch_pack_f16(const float* x, size_t n, const float* d_scale, uint16_t* out, hipStream_t stream);
void launch_unpack_f16(const uint16_t* in, size_t n, const float* d_inv, float* x, hipStream_t stream);
// comm_sparse.hip: the sparse gradient exchange (touched-row flags -> ascending row list -> per-owner messages)
size_t   sparse_flag_bytes(int64_t P);
uint32_t sparse_flag_chunks(int64_t P);
void     launch_mark_rows(const KeptRows& r, uint8_t* flags, hipStream_t stream); // flags[r.vis_index[row]] = 1, rows < r.P
void     launch_compact_flags(const uint8_t* flags, int64_t P, uint32_t* chunk_ws, uint32_t* rows, uint32_t* d_total,
                              hipStream_t stream, const uint32_t* copy_src = nullptr, uint32_t* copy_dst = nullptr,
                              const uint32_t* box_word0 = nullptr, uint32_t* host_box = nullptr, uint32_t serial = 0);
void     launch_owner_bounds(const uint32_t* rows, const uint32_t* d_total, int64_t shard, int world, uint32_t* d_bounds,
                             hipStream_t stream);
int64_t  sparse_message_words(int64_t count, int sh_degree);
void     launch_sparse_pack(float* const grads[5], int sh_degree, const uint32_t* rows, int64_t count, float* msg,
                            hipStream_t stream);
void     launch_sparse_accumulate(float* const grads[5], int sh_degree, const float* msg, int64_t count, int64_t row_first,
                                  int64_t row_count, hipStream_t stream);

// ---- backward.hip ----
// floats per on-screen splat in the 2-D gradient buffer: mean(2) conic(3) opacity(1) rgb(3) value(1) pad(2).  Slot 9 is the
// depth maps' dL/dvalue (maps.hip); the colour backward leaves it at the zero it was cleared to
constexpr int kG2D = 12, kG2DValueSlot = 9;
size_t grads2d_bytes(int64_t V_cap);
// (bwd_counter, when given, is zeroed too: the persistent render-backward's tile counter)
void   launch_zero_grads2d(const uint32_t* d_counts, float* grads2d, hipStream_t stream, uint32_t* bwd_counter = nullptr);
// The dense gradient arrays' zero-fill as a side job of the render-backward: the five arrays (pos, scale, rotq, sh, opacity)
// and their lengths in floats; n[3] == 0: no fill.  (Plain pointer members: a dynamically indexed kernel argument would live in
// scratch memory.)
struct DenseFill {
    float *b0 = nullptr, *b1 = nullptr, *b2 = nullptr, *b3 = nullptr, *b4 = nullptr;
    uint32_t n[5] = { 0, 0, 0, 0, 0 };
};
void   launch_render_backward(const KeptFrame& f, const float bg[3], const float* dL_dimg, float* grads2d, hipStream_t stream,
                              uint32_t* work_counter = nullptr, uint32_t persistent_wgs = 0, const DenseFill* fill = nullptr);
// The per-splat pass of the rows r (kept_rows.hpp; r.shjac: the forward's colour Jacobian rows, if kept; r.opacity: read only
// for a row of an antialiased frame, r.cp.raster_mode) into the five gradient arrays, laid out as `out` says:
struct RowsOut {
    // compact: output row k belongs to the frame's k-th on-screen splat (dense id k, splat vis_index[k], ascending) instead of
    // row = splat index: consecutive rows, every one written -- no zero-fill, no 39 %-dense store pattern
    // accumulate: ADD the rows to what the arrays hold (dense rows of a further view)
    bool compact, accumulate;
    // slice_bounds != NULL: only the survivors [slice_bounds[slice], slice_bounds[slice + 1]) (a splat-range slice, see
    // launch_slice_bounds; `slices` sizes the launch).  NULL: all of them (slice 0 of 1)
    const uint32_t* slice_bounds;
    int             slice, slices;
};
void   launch_preprocess_backward(const KeptRows& r, float* dL_dpos, float* dL_dscale, float* dL_drotq, float* dL_dsh,
                                  float* dL_dopacity, const RowsOut& out, hipStream_t stream);
// bounds[0 .. slices]: dense-id boundaries of the splat-index ranges [k P / slices, (k + 1) P / slices), k < slices <= 63
void   launch_slice_bounds(const KeptRows& r, int slices, uint32_t* bounds, hipStream_t stream);

// ---- maps.hip : depth and alpha maps of the last keep-state frame and their backward ----
constexpr int kDepthZ = 0, kDepthInvZ = 1; // = LCGS_DEPTH_Z, LCGS_DEPTH_INV_Z: a splat's value is its view z, or 1 / z
// depth / alpha: H W floats each, either may be NULL; f.strip_masks NULL: every entry of the walk is fetched
void launch_render_maps(const KeptFrame& f, int mode, float* depth, float* alpha, hipStream_t stream);
// the depth-distortion map, H W floats: fl(fl(A M2) - fl(M1 M1)) of the three channels accumulated with u = fl(value - center)
void launch_render_distortion(const KeptFrame& f, int mode, float center, float* dist, hipStream_t stream);
// ADDS the sums of the map channels to grads2d slots 0-5 and kG2DValueSlot (dL_ddepth / dL_dalpha / dL_ddist: any may be NULL).
// dL_ddist != NULL: the distortion channel about `center`, its three per-pixel sums re-derived by a pre-walk inside the kernel;
// NULL: the two-channel kernel
// nrm != NULL: the normal channel as well -- n_i . dL_dnormal[p] joins the per-entry scalar, the three sums w_i dL_dnormal_c[p]
// are ADDED to dL_dn (4 floats per on-screen row, cleared by launch_splat_normals), not to grads2d
struct NormalChannel {
    const float* dL_dnormal; // 3 H W, CHW
    const float4* normals;   // launch_splat_normals' rows
    float*       dL_dn;
};
void launch_render_maps_backward(const KeptFrame& f, int mode, const float* dL_ddepth, const float* dL_dalpha, float* grads2d,
                                 hipStream_t stream, float center = 0.0f, const float* dL_ddist = nullptr,
                                 const NormalChannel* nrm = nullptr);
// one lane per on-screen row: dL_dpos[row] += grads2d slot kG2DValueSlot x dvalue/dz x front (behind the preprocess-backward)
void launch_maps_depth_to_pos(const KeptRows& r, int mode, float* dL_dpos, hipStream_t stream);
// ---- the normal map (maps.hip): the per-splat normal is defined in include/lcgs_hip.h ----
// the two context-owned workspaces, each: 16 bytes per on-screen row (n0, n1, n2, axis | flip << 2; dL/dn0..2, unused)
size_t splat_normals_bytes(int64_t rows);
// one lane per on-screen row: writes the row's normal; dL_dn != NULL: clears the row's dL/dn slot too
void launch_splat_normals(const KeptRows& r, float4* normals, float4* dL_dn, hipStream_t stream);
// k_render_maps' walk with three accumulators: normal_map 3 H W floats, CHW
void launch_render_normals(const KeptFrame& f, const float4* normals, float* normal_map, hipStream_t stream);
// one lane per on-screen row: dL_drotq[row] += (dc/dq)^T dL/dc from dL_dn (behind the preprocess-backward)
void launch_normals_to_rot(const KeptRows& r, const float4* normals, const float4* dL_dn, float* dL_drotq, hipStream_t stream);

// ---- features.hip : caller-supplied per-splat feature channels of the last keep-state frame and their backward ----
// the caller's rows as the walks read them: K floats per scene row, found through the frame's on-screen row -> scene row table
struct FeatureChannel {
    int             K;               // 1 .. LCGS_FEATURES_MAX
    const uint32_t* vis_index;       // on-screen row -> scene row (KeptRows::vis_index)
    const float*    features;        // P x K, row-major
    const float*    dL_dfeature_map; // K H W, CHW (the backward only)
    float*          dL_dfeatures;    // P x K, ADDED to by float atomics (the backward only; NULL: the features are frozen)
};
// the channels a walk takes at a time: the smallest of 4 / 8 / 16 that holds K, 16 beyond; forced (4, 8, 16): that width (measurement)
int features_chunk_width(int K, int forced = 0);
// k_render_maps' walk with `ch` accumulators per chunk of channels (grid.y: the chunks): feature_map K H W floats, CHW
void launch_render_features(const KeptFrame& f, const FeatureChannel& fc, float* feature_map, int ch, hipStream_t stream);
// grads2d != NULL: ADDS the channel's six geometry sums to grads2d slots 0-5 (no value slot); fc.dL_dfeatures != NULL: ADDS
// sum_p w_i dL_dfeature_map[c][p] to it.  grads2d NULL: the frozen-geometry walk, which forms no geometry sums at all
void launch_render_features_backward(const KeptFrame& f, const FeatureChannel& fc, float* grads2d, int ch, hipStream_t stream);

// ---- contrib.hip : per-splat blend-weight statistics of the last keep-state frame, and the keep / drop rule ----
// the context-owned slab: {sum, max bits, count} per on-screen row, indexed by the lists' on-screen indices
size_t contrib_slab_bytes(int64_t rows);
// clears the slots of the frame's on-screen rows
void launch_contrib_zero(const KeptRows& r, uint32_t* slab, hipStream_t stream);
// the walk of launch_render_maps, every entry reduced over the pixels that blend it; ATOMICALLY adds to the slab
void launch_contrib_walk(const KeptFrame& f, uint32_t* slab, hipStream_t stream);
// one lane per on-screen row: slots with a count fold into the caller's arrays at vis_index[row] (any of the four may be NULL)
void launch_contrib_fold(const KeptRows& r, const uint32_t* slab, float* weight_sum, float* weight_max, uint32_t* pixels,
                         uint32_t* views, hipStream_t stream);
struct ContribRule { // a row is kept iff every enabled (non-zero) minimum is met
    float    min_weight_max, min_weight_sum;
    uint64_t min_pixels, min_views;
};
// action[i] = 1 kept / 0 dropped (lcgs_densify's actions); emit (nullable) = the same as a count, for the rewrite's prefix sums
void launch_contrib_classify(int64_t P, const ContribRule& rule, const float* weight_sum, const float* weight_max,
                             const uint32_t* pixels, const uint32_t* views, uint32_t* emit, uint8_t* action, hipStream_t stream);

// ---- absgrad.hip : AbsGS densification statistics of the last keep-state frame ----
// the context-owned workspace: (sum_p |g_x|, sum_p |g_y|) per on-screen row, indexed by the lists' on-screen indices
size_t absgrad_ws_bytes(int64_t rows);
// clears the slots of the frame's on-screen rows
void launch_absgrad_zero(const KeptRows& r, float* ws, hipStream_t stream);
// the walk of launch_render_maps_backward with the frame's colours and background beside the map channels (any of the three
// gradients may be NULL, not all): per (pixel, entry) the mean gradient of all given channels, its absolute value, summed over
// the pixels; ATOMICALLY adds to the workspace.  Reads no 2-D gradient row and writes none
void launch_absgrad_walk(const KeptFrame& f, int mode, const float bg[3], const float* dL_dimg, const float* dL_ddepth,
                         const float* dL_dalpha, float* ws, hipStream_t stream);
// one lane per on-screen row: absgrad[2 i ..] += the slot (NULL: skipped); grad_accum != NULL: grad_accum[i] += its norm in NDC
// units, denom and max_radii as launch_densify_stats
void launch_absgrad_rows(const KeptRows& r, const float* ws, float* absgrad, float* grad_accum, uint32_t* denom, int32_t* max_radii,
                         hipStream_t stream);

// ---- camera_grad.hip : the camera gradient of the last backward, from the 2-D rows it left ----
// the context-owned slab: twelve doubles per block of 256 on-screen rows
size_t camera_grad_slab_bytes(int64_t P);
// dL_dcam: 12 floats (position, front, up, right), overwritten.  r.shjac NULL: the direction part comes from the sh rows;
// depth_mode: the depth mode of the backward that wrote grads2d slot kG2DValueSlot, -1: none.
// Two launches (per-block sums, then one workgroup that adds them in a fixed order); no atomics
void launch_camera_grad(const KeptRows& r, int depth_mode, double* slab, float* dL_dcam, hipStream_t stream);

} // namespace lcgs
