// abi_internal.hpp -- what the translation units behind the C ABI share: the context (context.hpp), the small helpers of
// abi_core.cpp and the frame / sibling plumbing of abi_frame.cpp.  The C ABI itself is split by subject (round 4; one
// 1 700-line file until then), every exported symbol unchanged:
//   abi_core.cpp      errors, context create / destroy, stream, synchronise, profiling, stats, debug hooks
//   device_owned.cpp  the owning types of common.hpp (device buffer, event, stream, pinned block): nothing else frees
//   abi_stages.cpp    the reference's three operators + the two lcpp primitives (stage level), deferred stage mode
//   abi_scene.cpp     scene bind / upload / download / PLY ingest / spatial re-order / f16 SH / LOD
//   abi_frame.cpp     the fused frame: workspace, enqueue, lcgs_render_forward, camera batches, the sibling context
//   abi_backward.cpp  lcgs_render_backward and its variants (compact rows, accumulate, fused Adam, maps, distortion, camera): one
//                     request (BackwardRequest) behind all of them; lcgs_render_maps / _distortion, lcgs_contrib_accumulate
//   abi_train.cpp     lcgs_adam_step, lcgs_fit_views
//   abi_densify.cpp   adaptive density control: lcgs_densify_accumulate, lcgs_densify, lcgs_opacity_reset; lcgs_contrib_keep_mask, lcgs_prune
//   abi_mcmc.cpp      3DGS-MCMC density control: lcgs_mcmc_relocate, lcgs_mcmc_add, lcgs_mcmc_noise, lcgs_mcmc_regularize
//   abi_filter3d.cpp  Mip-Splatting's 3-D smoothing filter: lcgs_filter3d_accumulate / _finalize / _apply / _backward
//   abi_transform.cpp a similarity transform of a scene: lcgs_similarity_plan_make, lcgs_camera_transform, lcgs_scene_transform,
//                     lcgs_scene_box_keep_mask
//   abi_tsdf.cpp      a surface out of the scene: lcgs_tsdf_integrate, lcgs_tsdf_mesh_count / _extract
//   abi_loss.cpp      lcgs_photometric_loss_backward, lcgs_normal_consistency_loss_backward, lcgs_set_fit_loss
//   abi_depth_prior.cpp  depth-prior supervision (Pearson, aligned L1): lcgs_depth_prior_loss_backward
//   abi_bilagrid.cpp  per-view bilateral-grid colour correction: lcgs_bilagrid_slice / _backward / _tv_loss_backward
//   abi_init.cpp      a scene from a point cloud: lcgs_knn_mean_dist2, lcgs_scene_init_from_points, lcgs_scene_extent
//   abi_owner.cpp     the frame in two halves (splat ownership): lcgs_owner_project / _render / _render_backward / _backward
#pragma once

#include <algorithm>
#include <initializer_list>

#include "common.hpp"
#include "context.hpp"
#include "kernels/kept_rows.hpp"
#include "kernels/kept_walk.hpp"
#include "kernels/launch.hpp"
#include "kernels/tie_order.hpp"

#define LCGS_TRY(expr)                    \
    do {                                  \
        lcgs_status _s = (expr);          \
        if (_s != LCGS_OK) return _s;     \
    } while (0)

namespace lcgs
{
namespace abi
{
inline int ceil_log2_u32(uint32_t v)
{
    int b = 0;
    while ((1ull << b) < v) ++b;
    return b;
}

// ---- rows [first, first + count) of the five attribute arrays (pos 3, scale 3, rotq 4, sh (deg + 1)^2 x 3, opacity 1 floats)
inline size_t sh_floats(int deg) { return (size_t)(deg + 1) * (deg + 1) * 3; }
struct RowFloats {
    size_t n[5];
    size_t operator[](int a) const { return n[a]; }
};
inline RowFloats row_floats(int deg) { return { { 3, 3, 4, sh_floats(deg), 1 } }; }
struct SceneRows {
    const float *pos, *scale, *rotq, *sh, *opacity;
};
inline SceneRows scene_rows(const lcgs_context* ctx) { return { ctx->pos, ctx->scale, ctx->rotq, ctx->sh, ctx->opacity }; }
template <class Rows> // lcgs_grads, lcgs_params, SceneRows: five pointers in that order
Rows rows_from(const Rows& r, int deg, size_t first)
{
    auto [pos, scale, rotq, sh, opacity] = r;
    return { pos + 3 * first, scale + 3 * first, rotq + 4 * first, sh + sh_floats(deg) * first, opacity + first };
}
// the render-backward's zero-fill side job for `count` rows of (already offset) gradient arrays; false: an array is too long
// for the kernel's 32-bit lengths
inline bool dense_fill_rows(const lcgs_grads& g, int deg, size_t count, DenseFill* fill)
{
    if (count * sh_floats(deg) >= ((size_t)1 << 32)) return false;
    const RowFloats w = row_floats(deg);
    fill->b0 = g.d_dL_dpos, fill->b1 = g.d_dL_dscale, fill->b2 = g.d_dL_drotq, fill->b3 = g.d_dL_dsh, fill->b4 = g.d_dL_dopacity;
    for (int a = 0; a < 5; ++a) fill->n[a] = (uint32_t)(count * w[a]);
    return true;
}
// ... and the same rows cleared by five memsets on a stream
inline lcgs_status zero_grad_rows(const lcgs_grads& g, int deg, size_t count, hipStream_t stream)
{
    float* const    arr[5] = { g.d_dL_dpos, g.d_dL_dscale, g.d_dL_drotq, g.d_dL_dsh, g.d_dL_dopacity };
    const RowFloats w      = row_floats(deg);
    for (int a = 0; a < 5; ++a) LCGS_HIP_CHECK(hipMemsetAsync(arr[a], 0, count * w[a] * 4, stream));
    return LCGS_OK;
}
// ---- the optimiser's arguments from the C ABI's
inline AdamArrays adam_arrays(const lcgs_params* p) { return { p->pos, p->scale, p->rotq, p->sh, p->opacity }; }
inline AdamRates  adam_rates(const lcgs_adam_config* c)
{
    return { c->lr_pos, c->lr_sh_dc, c->lr_sh_rest, c->lr_opacity, c->lr_scale, c->lr_rot };
}
lcgs_status check_adam_config(const lcgs_adam_config* cfg); // abi_train.cpp
// every member of every pack is a pointer; rotq_aligned: ... and the rotq arrays can be read as float4
inline lcgs_status check_param_packs(std::initializer_list<const lcgs_params*> packs, bool rotq_aligned)
{
    for (const lcgs_params* p : packs)
        LCGS_REQUIRE(p->pos && p->scale && p->rotq && p->sh && p->opacity, "NULL device pointer in a parameter pack");
    if (rotq_aligned)
        for (const lcgs_params* p : packs)
            LCGS_REQUIRE((reinterpret_cast<uintptr_t>(p->rotq) & 15) == 0, "rotq arrays must be 16-byte aligned");
    return LCGS_OK;
}

// abi_core.cpp
lcgs_status mark(lcgs_context* ctx, const char* name);          // per-stage timing mark (+ LCGS_DEBUG_SYNC)
lcgs_status collect_marks(lcgs_context* ctx);
lcgs_status sync_frame(lcgs_context* ctx);                      // the context's stream + the last frame's counter read-back
lcgs_status check_frame_flags(lcgs_context* ctx);               // problems an asynchronous frame reported through its counters
lcgs_status check_camera(const lcgs_camera* cam);
// abi_stages.cpp: deferred stage mode -- run a recorded SHProcessor::process / GSProjector::forward now
lcgs_status run_deferred_sh(lcgs_context* ctx);
lcgs_status run_deferred_proj(lcgs_context* ctx);
// abi_scene.cpp: the cull pass's {position, extent bound} rows of a context-owned scene (context.hpp cull_bound)
lcgs_status refresh_cull_bound(lcgs_context* ctx);
lcgs_status build_cull_bound(lcgs_context* ctx, int P, const float* pos, const float* scale, const float* rotq);
// ... dropped when the library itself writes activated arrays that ARE the context's scene (optimiser steps): the frames
// fall back to reading position + scale + rotation until the arrays are bound again
// (EVERY live context of the process is looked at -- a second context that renders the same arrays keeps rows of its own)
void scene_arrays_written(lcgs_context* ctx, const float* pos, const float* scale, const float* rotq);
// ... and every OTHER thread family's context that has any of ctx's bound arrays bound is told that they changed (its f16
// coefficient copy and the kept state of its last frame are stale); ctx and its siblings are the caller's to handle
void scene_modified_elsewhere(lcgs_context* ctx);
// abi_owner.cpp: lcgs_owner_render, and its variant for the ownership step that reads nothing back (comm.cpp)
struct OwnerAsyncFrame {
    OwnerSegs       segs;            // padded per-owner segments of the received rows / records
    const uint32_t* table = nullptr; // device: the all-gathered counts, [o * N + view] = owner o's rows on `view`'s screen
    uint32_t        view  = 0;
    uint32_t*       overflow = nullptr; // device word: bit 0 a segment was clipped, bit 1 the pair buffers were too small
};
lcgs_status owner_render_frame(lcgs_context* ctx, const lcgs_camera* camera, const float bg_color[3], int num_rows,
                               const uint32_t* d_rows, const float* d_records, float* d_img, int keep_state,
                               const OwnerAsyncFrame* af);
lcgs_status owner_render_backward_into(lcgs_context* ctx, const float* d_dL_dimg, float* d_grads2d, const DenseFill* fill);
lcgs_status owner_backward_rows(lcgs_context* ctx, int slot, const float* d_grads2d, const lcgs_grads* grads, int mode);
void owner_frame_settle(lcgs_context* ctx); // hints / pair capacity from the pinned counters of such a frame
// the process's live contexts (lcgs_create / lcgs_destroy), for scene_arrays_written
void registry_add(lcgs_context* ctx);
void registry_remove(lcgs_context* ctx);
// the owning thread publishes the arrays its derived rows were built from and the arrays it has bound (threading:
// context.hpp foreign_writes)
void registry_publish(lcgs_context* ctx);
// abi_frame.cpp
lcgs_status ensure_fused_workspace(lcgs_context* ctx, const CamParams& cp, bool keep_state);
// a pipelined frame of the context may still be using the workspace through the auxiliary stream: ctx->stream waits for it
lcgs_status join_aux_stream(lcgs_context* ctx);
lcgs_status ensure_head_stream(lcgs_context* ctx); // created on first use; also the stream of the batch sibling
// lcgs_create with the auxiliary stream given (borrowed: synchronised but not destroyed with the context) instead of created
lcgs_status create_context(int device_id, void* stream, hipStream_t borrowed_aux, lcgs_context** out_ctx);
// a frame's zeroed block (tile ranges + the persistent renderers' counters) is copy `zb`; cleared on `st` unless it already is
lcgs_status use_zero_block(lcgs_context* ctx, int zb, bool cleared, hipStream_t st);
// what the depth sort of a re-ordered scene needs to blend equal depths in FILE order (kernels/tie_order.hpp), and the bits
// of a sorted value that are the dense id (on == false: the context holds the scene in file order)
struct FrameTie {
    TieOrder tie;
    uint32_t id_mask = 0xFFFFFFFFu;
    bool     on      = false;
};
FrameTie frame_tie_order(lcgs_context* ctx);
// The second half of a frame, from a depth-sorted order of dense ids to the image: expand -> tile partition -> ranges ->
// tile schedule -> renderer -> the 40-byte counter copy.  What differs between the fused frame and the one drawn from
// received records (abi_owner.cpp, all defaults):
struct FrameTailOptions {
    bool       pipelined = false; // buffers rotate; next schedule, next zero block, counter copy on the auxiliary stream
    bool       marks = false, work_counter = false; // per-stage timing marks; the renderer gets the frame's tile counter
    uint32_t   persist_wgs   = 0;       // > 0: the renderer is a bounded persistent grid of this many workgroups
    bool       g2d_in_render = false;   // the renderer clears the 2-D gradient rows as a side job
    hipEvent_t records_ready = nullptr; // waited for in front of the renderer
    uint32_t*  pair_verdict  = nullptr; // device word, |= 2 in front of the counter copy if the pair buffers were too small
    // a pipelined in-order frame (context.hpp head_stream): expand -> ranges and the counter copy run on this stream, only the
    // renderer on the context's; the frame's parity selects the events later calls wait for
    hipStream_t head   = nullptr;
    int         parity = 0;
};
// rows: the expansion's launch size (hint_V, or a known row count).  Leaves last.list_buf / last_tile_order for the backward.
lcgs_status render_sorted_frame(lcgs_context* ctx, const CamParams& cp, const float bg[3], float* d_img, const SplatRecord* recs,
                                const uint32_t* order, uint32_t id_mask, int64_t rows, int64_t hint_L, bool keep_state,
                                const FrameParams* d_fp, const FrameTailOptions& opt);
// what the walks of the last keep-state frame's kept lists read (kernels/kept_walk.hpp), this context's own records; the
// strip masks the forward kept, unless they are switched off (LCGS_BWD_USE_MASKS=0: every walk fetches every entry)
inline KeptFrame kept_frame(lcgs_context* ctx)
{
    return { ctx->last.cp,
             ctx->ranges,
             ctx->pairv[ctx->last.list_buf].as<uint32_t>(),
             ctx->recs.as<SplatRecord>(),
             ctx->final_T.as<float>(),
             ctx->n_contrib.as<uint32_t>(),
             ctx->bwd_use_masks ? ctx->strip_masks.as<uint8_t>() : nullptr,
             ctx->counts.as<uint32_t>(),
             ctx->last_tile_order };
}
// the launch size of a pass with one lane per on-screen row: the hint the frames keep, never more than the scene's rows
inline int64_t rows_hint(const lcgs_context* ctx) { return ctx->hint_V > 0 ? std::min<int64_t>(ctx->hint_V, ctx->P) : ctx->P; }
// what such a pass over the last keep-state frame reads (kernels/kept_rows.hpp), this context's own records and 2-D rows
inline KeptRows kept_rows(lcgs_context* ctx)
{
    return { ctx->last.cp,
             ctx->last.scale_modifier,
             ctx->sh_deg,
             ctx->pos,
             ctx->scale,
             ctx->rotq,
             ctx->sh,
             ctx->opacity,
             ctx->vis_index.as<uint32_t>(),
             ctx->counts.as<uint32_t>(),
             ctx->grads2d.as<float>(),
             ctx->last_has_jac ? ctx->shjac.as<float4>() : nullptr,
             ctx->recs.as<SplatRecord>(),
             (int64_t)ctx->P,
             rows_hint(ctx) };
}
// ... and a view of an ownership step (abi_owner.cpp): the slot's row range of the scene, its rows and counts, the caller's
// 2-D rows; the launch is sized by the slot's known row count
inline KeptRows owner_slot_rows(lcgs_context* ctx, int slot, const float* d_grads2d)
{
    auto&           s = ctx->owner[slot];
    const SceneRows r = rows_from(scene_rows(ctx), ctx->sh_deg, (size_t)s.row_first);
    return { s.cp,
             s.scale_modifier,
             ctx->sh_deg,
             r.pos,
             r.scale,
             r.rotq,
             r.sh,
             r.opacity, // (s.cp.raster_mode is 0: the classic instantiation runs and reads none of it)
             s.vis.as<uint32_t>(),
             s.counts.as<uint32_t>(),
             d_grads2d,
             s.has_jac ? s.shjac.as<float4>() : nullptr,
             nullptr,
             (int64_t)s.row_count,
             (int64_t)s.num };
}
// The state every pass over a kept frame needs: a keep-state frame of this context's own records, lists per tile.  Both
// overrides are whole messages for callers that have a better one: no_frame, and owner_frame for a frame drawn from
// received records.  (abi_backward.cpp)
lcgs_status check_own_kept_frame(lcgs_context* ctx, const char* who, const char* owner_frame = nullptr,
                                 const char* no_frame = nullptr);
// the kept state of the last frame that every kind of frame records
void keep_frame_state(lcgs_context* ctx, const CamParams& cp, const float bg[3], float scale_modifier, bool has_state);
// launch-size hints follow the live counts once those leave the [hint / 2, hint] band (inside it a captured graph stays valid)
inline void update_hint(int64_t& hint, uint32_t count)
{
    if ((int64_t)count > hint || (int64_t)count * 2 < hint) hint = (int64_t)count + count / 4 + 4096;
}
// clears the counters' overflow record ([3] the last frame's flag; [6] / [7] sticky: frames, largest demand) / ... and grows
// pair_capacity for a demand of `pairs` with a quarter to spare, LCGS_ERR_CAPACITY beyond 2^31 - 1
lcgs_status clear_pair_overflow(lcgs_context* ctx);
lcgs_status grow_pair_capacity(lcgs_context* ctx, uint32_t pairs);
lcgs_status prepare_twin(lcgs_context* ctx); // the sibling context of camera / view batches: created on first use, same scene

// marks a context and its siblings as rendering several frames at once for the duration of a batch call
struct InFlight {
    lcgs_context* c;
    InFlight(lcgs_context* ctx, bool on) : c(on ? ctx : nullptr)
    {
        for (lcgs_context* t = c; t; t = t->twin) t->frames_in_flight = true;
    }
    ~InFlight()
    {
        for (lcgs_context* t = c; t; t = t->twin) t->frames_in_flight = false;
    }
};
} // namespace abi
} // namespace lcgs
