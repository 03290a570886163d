// abi_densify.cpp -- the C ABI, part 7: adaptive density control (csrc/kernels/densify.hip) -- the statistics of a step (and
// their AbsGS form, lcgs_absgrad_accumulate: kernels/absgrad.hip, a walk of the kept frame's lists of its own), the
// out-of-place clone / split / prune rewrite of raw parameters and Adam moments, the opacity reset, and contribution-based
// pruning on the statistics of lcgs_contrib_accumulate (kernels/contrib.hip: the keep mask, and the rewrite restricted to it).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "abi_internal.hpp"

using namespace lcgs;
using namespace lcgs::abi;

namespace
{
// the rule of lcgs_contrib_keep_mask / lcgs_prune: an enabled (non-zero) minimum needs its statistics member
lcgs_status check_prune_rule(const lcgs_prune_config* cfg, const lcgs_contrib_stats* stats)
{
    LCGS_REQUIRE((cfg->min_weight_max == 0.0f || stats->weight_max) && (cfg->min_weight_sum == 0.0f || stats->weight_sum) &&
                     (cfg->min_pixels == 0 || stats->pixels) && (cfg->min_views == 0 || stats->views),
                 "a non-zero minimum whose statistics member is NULL");
    return LCGS_OK;
}
ContribRule prune_rule(const lcgs_prune_config* cfg)
{
    return { cfg->min_weight_max, cfg->min_weight_sum, cfg->min_pixels, cfg->min_views };
}

// The out-of-place rewrite of lcgs_densify and lcgs_prune, behind their argument checks.  classify(emit, action, stream) fills
// the rows each source row emits and what becomes of it; the inclusive sums of `emit` are every row's place, and their last
// the new count: the call's one read-back, known before anything is scattered.  `who`: the call's name; `verb`: needs | keeps.
struct RowRewrite {
    int                sh_degree;
    const lcgs_params *raw, *m, *v, *out_raw, *out_m, *out_v, *out_activated;
    int64_t            capacity;
    float              split_drop; // the scatter's last arguments: lcgs_prune splits no row and has none of them
    const float*       noise;
    uint64_t           seed;
    uint32_t*          src_row;
};
template <class Classify>
lcgs_status rewrite_rows(lcgs_context* ctx, const char* who, const char* verb, int64_t P, const RowRewrite& r, Classify classify,
                         int64_t* new_count)
{
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    LCGS_TRY(ctx->dn_emit.ensure((size_t)P * 4));
    LCGS_TRY(ctx->dn_incl.ensure((size_t)P * 4));
    LCGS_TRY(ctx->dn_action.ensure((size_t)P));
    LCGS_TRY(ctx->st_scan_temp.ensure(scan_temp_bytes(P)));
    classify(ctx->dn_emit.as<uint32_t>(), ctx->dn_action.as<uint8_t>(), st);
    launch_inclusive_sum_u32(ctx->dn_emit.as<uint32_t>(), ctx->dn_incl.as<uint32_t>(), P, ctx->st_scan_temp.ptr, st);
    uint32_t total = 0;
    LCGS_HIP_CHECK(hipMemcpyAsync(&total, ctx->dn_incl.as<uint32_t>() + (P - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    LCGS_HIP_CHECK(hipStreamSynchronize(st));
    *new_count = (int64_t)total;
    if ((int64_t)total > r.capacity) {
        set_last_error(std::string(who) + ": the rewrite " + verb + " " + std::to_string(total) +
                       " rows, the destination arrays hold " + std::to_string((long long)r.capacity));
        return LCGS_ERR_CAPACITY;
    }
    if (total == 0) return LCGS_OK;
    scene_arrays_written(ctx, r.out_activated->pos, r.out_activated->scale, r.out_activated->rotq); // (destinations a context renders)
    launch_densify_scatter(P, (int)sh_floats(r.sh_degree), ctx->dn_action.as<uint8_t>(), ctx->dn_incl.as<uint32_t>(),
                           adam_arrays(r.raw), adam_arrays(r.m), adam_arrays(r.v), adam_arrays(r.out_raw), adam_arrays(r.out_m),
                           adam_arrays(r.out_v), adam_arrays(r.out_activated), r.split_drop, r.noise, r.seed, r.src_row, st);
    return LCGS_OK;
}
} // namespace

extern "C" {

lcgs_status lcgs_densify_accumulate(lcgs_context* ctx, int num_gaussians, const lcgs_densify_stats* stats)
{
    LCGS_REQUIRE(ctx && stats, "NULL argument");
    LCGS_REQUIRE(stats->grad_accum && stats->denom && stats->max_radii, "NULL device pointer in the statistics");
    LCGS_ENTRY(ctx);
    // (an ownership-step frame: its rows are the received records', not this context's scene's)
    LCGS_TRY(check_own_kept_frame(ctx, "lcgs_densify_accumulate",
                                  "the last frame was drawn from received records (lcgs_owner_render): no statistics for it",
                                  "lcgs_densify_accumulate needs a preceding lcgs_render_forward(..., keep_state = 1) of this scene"));
    if (!ctx->g2d_backward_done) {
        set_last_error("lcgs_densify_accumulate needs a backward of the last frame (its 2-D gradient rows are only zeros until then)");
        return LCGS_ERR_STATE;
    }
    LCGS_REQUIRE(num_gaussians == ctx->P, "num_gaussians must be the bound scene's");
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    launch_densify_stats(kept_rows(ctx), stats->grad_accum, stats->denom, stats->max_radii, ctx->stream);
    LCGS_HIP_CHECK(hipGetLastError());
    return LCGS_OK;
}

lcgs_status lcgs_absgrad_accumulate(lcgs_context* ctx, int num_gaussians, const float* d_dL_dimg, int mode,
                                    const float* d_dL_ddepth, const float* d_dL_dalpha, const lcgs_densify_stats* stats,
                                    float* d_absgrad)
{
    LCGS_REQUIRE(ctx, "NULL argument");
    LCGS_REQUIRE(d_dL_dimg || d_dL_ddepth || d_dL_dalpha, "all three gradients are NULL");
    LCGS_REQUIRE(stats || d_absgrad, "both outputs are NULL");
    LCGS_REQUIRE(!stats || (stats->grad_accum && stats->denom && stats->max_radii), "NULL device pointer in the statistics");
    LCGS_REQUIRE(mode == LCGS_DEPTH_Z || mode == LCGS_DEPTH_INV_Z, "mode must be LCGS_DEPTH_Z or LCGS_DEPTH_INV_Z");
    LCGS_ENTRY(ctx);
    LCGS_REQUIRE(num_gaussians == ctx->P, "num_gaussians must be the bound scene's");
    // (no backward is needed, and none is disturbed: the walk reads the kept lists and the caller's gradients, its sums go to a
    //  workspace of their own -- the frame's 2-D gradient rows and the flags behind them stay as they are)
    LCGS_TRY(check_own_kept_frame(ctx, "lcgs_absgrad_accumulate",
                                  "the last frame was drawn from received records (lcgs_owner_render): no statistics for it"));
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    // one slot per on-screen row; sized for the scene's rows like the frame's other per-row buffers (the count stays on the device)
    LCGS_TRY(ctx->absgrad_ws.ensure(absgrad_ws_bytes((int64_t)ctx->P)));
    hipStream_t    st   = ctx->stream;
    const KeptRows rows = kept_rows(ctx);
    float*         ws   = ctx->absgrad_ws.as<float>();
    ctx->n_marks        = 0;
    LCGS_TRY(mark(ctx, "begin"));
    launch_absgrad_zero(rows, ws, st);
    launch_absgrad_walk(kept_frame(ctx), mode, ctx->last.bg, d_dL_dimg, d_dL_ddepth, d_dL_dalpha, ws, st);
    LCGS_TRY(mark(ctx, "absgrad_walk"));
    launch_absgrad_rows(rows, ws, d_absgrad, stats ? stats->grad_accum : nullptr, stats ? stats->denom : nullptr,
                        stats ? stats->max_radii : nullptr, st);
    LCGS_TRY(mark(ctx, "absgrad_rows"));
    LCGS_HIP_CHECK(hipGetLastError());
    if (ctx->profiling) {
        LCGS_HIP_CHECK(hipStreamSynchronize(st));
        LCGS_TRY(collect_marks(ctx));
    }
    return LCGS_OK;
}

lcgs_status lcgs_densify(lcgs_context* ctx, int num_gaussians, int sh_degree, const lcgs_densify_config* cfg,
                         const lcgs_densify_stats* stats, const lcgs_params* raw, const lcgs_params* m, const lcgs_params* v,
                         const lcgs_params* out_raw, const lcgs_params* out_m, const lcgs_params* out_v,
                         const lcgs_params* out_activated, const lcgs_densify_stats* out_stats, int64_t capacity,
                         const float* d_noise, uint32_t* d_src_row, int64_t* new_num_gaussians)
{
    LCGS_REQUIRE(ctx && cfg && stats && raw && m && v && out_raw && out_m && out_v && out_activated && out_stats &&
                     new_num_gaussians,
                 "NULL argument");
    LCGS_REQUIRE(num_gaussians >= 0, "num_gaussians is negative");
    LCGS_REQUIRE(sh_degree >= 0 && sh_degree <= 3, "sh_degree must be in [0,3]");
    LCGS_REQUIRE(capacity >= 0, "capacity is negative");
    *new_num_gaussians = 0;
    if (num_gaussians == 0) return LCGS_OK;
    LCGS_TRY(check_param_packs({ raw, m, v, out_raw, out_m, out_v, out_activated }, true));
    LCGS_REQUIRE(stats->grad_accum && stats->denom && stats->max_radii && out_stats->grad_accum && out_stats->denom &&
                     out_stats->max_radii,
                 "NULL device pointer in the statistics");
    LCGS_REQUIRE(out_raw->pos != raw->pos && out_m->pos != m->pos && out_v->pos != v->pos && out_stats->denom != stats->denom,
                 "the rewrite is out of place: destinations must not alias sources");
    LCGS_ENTRY(ctx);
    DensifyRule rule;
    rule.grad_threshold  = cfg->grad_threshold;
    rule.dense_extent    = cfg->percent_dense * cfg->scene_extent;
    rule.huge_extent     = 0.1f * cfg->scene_extent;
    rule.min_opacity     = cfg->min_opacity;
    rule.max_screen_size = cfg->max_screen_size;
    const int64_t P = num_gaussians;
    // ln 1.6 to binary32 (children are 1.6 x smaller: raw scale - ln 1.6), rounded once from the double value
    const float      split_drop = (float)log((double)1.6f);
    const RowRewrite rw = { sh_degree, raw, m, v, out_raw, out_m, out_v, out_activated, capacity, split_drop, d_noise, cfg->seed,
                            d_src_row };
    LCGS_TRY(rewrite_rows(ctx, "lcgs_densify", "needs", P, rw,
                          [&](uint32_t* emit, uint8_t* action, hipStream_t st) {
                              launch_densify_classify(P, rule, raw->scale, raw->opacity, stats->grad_accum, stats->denom,
                                                      stats->max_radii, emit, action, st);
                          },
                          new_num_gaussians));
    const size_t total = (size_t)*new_num_gaussians;
    if (total == 0) return LCGS_OK;
    LCGS_HIP_CHECK(hipMemsetAsync(out_stats->grad_accum, 0, total * 4, ctx->stream));
    LCGS_HIP_CHECK(hipMemsetAsync(out_stats->denom, 0, total * 4, ctx->stream));
    LCGS_HIP_CHECK(hipMemsetAsync(out_stats->max_radii, 0, total * 4, ctx->stream));
    LCGS_HIP_CHECK(hipGetLastError());
    return LCGS_OK;
}

lcgs_status lcgs_contrib_keep_mask(lcgs_context* ctx, int num_gaussians, const lcgs_prune_config* cfg,
                                   const lcgs_contrib_stats* stats, uint8_t* d_keep)
{
    LCGS_REQUIRE(ctx && cfg && stats && d_keep, "NULL argument");
    LCGS_REQUIRE(num_gaussians >= 0, "num_gaussians is negative");
    LCGS_TRY(check_prune_rule(cfg, stats));
    LCGS_ENTRY(ctx);
    if (num_gaussians == 0) return LCGS_OK;
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    launch_contrib_classify(num_gaussians, prune_rule(cfg), stats->weight_sum, stats->weight_max, stats->pixels, stats->views,
                            nullptr, d_keep, ctx->stream);
    LCGS_HIP_CHECK(hipGetLastError());
    return LCGS_OK;
}

lcgs_status lcgs_prune(lcgs_context* ctx, int num_gaussians, int sh_degree, const lcgs_prune_config* cfg,
                       const lcgs_contrib_stats* stats, const lcgs_params* raw, const lcgs_params* m, const lcgs_params* v,
                       const lcgs_params* out_raw, const lcgs_params* out_m, const lcgs_params* out_v,
                       const lcgs_params* out_activated, int64_t capacity, uint32_t* d_src_row, int64_t* new_num_gaussians)
{
    LCGS_REQUIRE(ctx && cfg && stats && raw && m && v && out_raw && out_m && out_v && out_activated && new_num_gaussians,
                 "NULL argument");
    LCGS_REQUIRE(num_gaussians >= 0, "num_gaussians is negative");
    LCGS_REQUIRE(sh_degree >= 0 && sh_degree <= 3, "sh_degree must be in [0,3]");
    LCGS_REQUIRE(capacity >= 0, "capacity is negative");
    LCGS_TRY(check_prune_rule(cfg, stats));
    *new_num_gaussians = 0;
    if (num_gaussians == 0) return LCGS_OK;
    LCGS_TRY(check_param_packs({ raw, m, v, out_raw, out_m, out_v, out_activated }, true));
    LCGS_REQUIRE(out_raw->pos != raw->pos && out_m->pos != m->pos && out_v->pos != v->pos,
                 "the rewrite is out of place: destinations must not alias sources");
    LCGS_ENTRY(ctx);
    // (actions 0 and 1 only: no row splits, so neither the split's scale drop nor the sampler is reached)
    const RowRewrite rw = { sh_degree, raw, m, v, out_raw, out_m, out_v, out_activated, capacity, 0.0f, nullptr, 0, d_src_row };
    LCGS_TRY(rewrite_rows(ctx, "lcgs_prune", "keeps", num_gaussians, rw,
                          [&](uint32_t* emit, uint8_t* action, hipStream_t st) {
                              launch_contrib_classify(num_gaussians, prune_rule(cfg), stats->weight_sum, stats->weight_max,
                                                      stats->pixels, stats->views, emit, action, st);
                          },
                          new_num_gaussians));
    LCGS_HIP_CHECK(hipGetLastError());
    return LCGS_OK;
}

lcgs_status lcgs_opacity_reset(lcgs_context* ctx, int num_gaussians, float max_opacity, const lcgs_params* raw,
                               const lcgs_params* m, const lcgs_params* v, const lcgs_params* activated)
{
    LCGS_REQUIRE(ctx && raw && m && v && activated, "NULL argument");
    LCGS_REQUIRE(num_gaussians >= 0, "num_gaussians is negative");
    LCGS_REQUIRE(max_opacity > 0.0f && max_opacity < 1.0f, "max_opacity must be in (0,1)");
    LCGS_ENTRY(ctx);
    scene_arrays_written(ctx, activated->pos, activated->scale, activated->rotq);
    if (num_gaussians == 0) return LCGS_OK;
    LCGS_REQUIRE(raw->opacity && m->opacity && v->opacity && activated->opacity, "NULL opacity pointer in a parameter pack");
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    // logit(max_opacity) to binary32, rounded once from the double value
    const float ceiling = (float)log((double)max_opacity / (1.0 - (double)max_opacity));
    launch_opacity_reset(num_gaussians, ceiling, raw->opacity, m->opacity, v->opacity, activated->opacity, ctx->stream);
    LCGS_HIP_CHECK(hipGetLastError());
    return LCGS_OK;
}

} // extern "C"
