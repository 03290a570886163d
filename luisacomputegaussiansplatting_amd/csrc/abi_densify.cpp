// abi_densify.cpp -- the C ABI, part 7: adaptive density control (csrc/kernels/densify.hip) -- the statistics of a step, the
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
    const lcgs_params* packs[7] = { raw, m, v, out_raw, out_m, out_v, out_activated };
    for (const lcgs_params* p : packs)
        LCGS_REQUIRE(p->pos && p->scale && p->rotq && p->sh && p->opacity, "NULL device pointer in a parameter pack");
    for (const lcgs_params* p : packs)
        LCGS_REQUIRE((reinterpret_cast<uintptr_t>(p->rotq) & 15) == 0, "rotq arrays must be 16-byte aligned");
    LCGS_REQUIRE(stats->grad_accum && stats->denom && stats->max_radii && out_stats->grad_accum && out_stats->denom &&
                     out_stats->max_radii,
                 "NULL device pointer in the statistics");
    LCGS_REQUIRE(out_raw->pos != raw->pos && out_m->pos != m->pos && out_v->pos != v->pos && out_stats->denom != stats->denom,
                 "the rewrite is out of place: destinations must not alias sources");
    LCGS_ENTRY(ctx);
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t   st = ctx->stream;
    const int64_t P  = num_gaussians;
    LCGS_TRY(ctx->dn_emit.ensure((size_t)P * 4));
    LCGS_TRY(ctx->dn_incl.ensure((size_t)P * 4));
    LCGS_TRY(ctx->dn_action.ensure((size_t)P));
    LCGS_TRY(ctx->st_scan_temp.ensure(scan_temp_bytes(P)));
    DensifyRule rule;
    rule.grad_threshold  = cfg->grad_threshold;
    rule.dense_extent    = cfg->percent_dense * cfg->scene_extent;
    rule.huge_extent     = 0.1f * cfg->scene_extent;
    rule.min_opacity     = cfg->min_opacity;
    rule.max_screen_size = cfg->max_screen_size;
    launch_densify_classify(P, rule, raw->scale, raw->opacity, stats->grad_accum, stats->denom, stats->max_radii,
                            ctx->dn_emit.as<uint32_t>(), ctx->dn_action.as<uint8_t>(), st);
    launch_inclusive_sum_u32(ctx->dn_emit.as<uint32_t>(), ctx->dn_incl.as<uint32_t>(), P, ctx->st_scan_temp.ptr, st);
    // the call's one read-back: the new count, known before anything is scattered
    uint32_t total = 0;
    LCGS_HIP_CHECK(hipMemcpyAsync(&total, ctx->dn_incl.as<uint32_t>() + (P - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    LCGS_HIP_CHECK(hipStreamSynchronize(st));
    *new_num_gaussians = (int64_t)total;
    if ((int64_t)total > capacity) {
        set_last_error("lcgs_densify: the rewrite needs " + std::to_string(total) + " rows, the destination arrays hold " +
                       std::to_string((long long)capacity));
        return LCGS_ERR_CAPACITY;
    }
    if (total == 0) return LCGS_OK;
    scene_arrays_written(ctx, out_activated->pos, out_activated->scale, out_activated->rotq); // (destinations a context renders)
    // ln 1.6 to binary32 (children are 1.6 x smaller: raw scale - ln 1.6), rounded once from the double value
    const float split_drop = (float)log((double)1.6f);
    launch_densify_scatter(P, (int)sh_floats(sh_degree), ctx->dn_action.as<uint8_t>(), ctx->dn_incl.as<uint32_t>(),
                           adam_arrays(raw), adam_arrays(m), adam_arrays(v), adam_arrays(out_raw), adam_arrays(out_m), adam_arrays(out_v),
                           adam_arrays(out_activated),
                           split_drop, d_noise, cfg->seed, d_src_row, st);
    LCGS_HIP_CHECK(hipMemsetAsync(out_stats->grad_accum, 0, (size_t)total * 4, st));
    LCGS_HIP_CHECK(hipMemsetAsync(out_stats->denom, 0, (size_t)total * 4, st));
    LCGS_HIP_CHECK(hipMemsetAsync(out_stats->max_radii, 0, (size_t)total * 4, st));
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
    const lcgs_params* packs[7] = { raw, m, v, out_raw, out_m, out_v, out_activated };
    for (const lcgs_params* p : packs)
        LCGS_REQUIRE(p->pos && p->scale && p->rotq && p->sh && p->opacity, "NULL device pointer in a parameter pack");
    for (const lcgs_params* p : packs)
        LCGS_REQUIRE((reinterpret_cast<uintptr_t>(p->rotq) & 15) == 0, "rotq arrays must be 16-byte aligned");
    LCGS_REQUIRE(out_raw->pos != raw->pos && out_m->pos != m->pos && out_v->pos != v->pos,
                 "the rewrite is out of place: destinations must not alias sources");
    LCGS_ENTRY(ctx);
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t   st = ctx->stream;
    const int64_t P  = num_gaussians;
    LCGS_TRY(ctx->dn_emit.ensure((size_t)P * 4));
    LCGS_TRY(ctx->dn_incl.ensure((size_t)P * 4));
    LCGS_TRY(ctx->dn_action.ensure((size_t)P));
    LCGS_TRY(ctx->st_scan_temp.ensure(scan_temp_bytes(P)));
    launch_contrib_classify(P, prune_rule(cfg), stats->weight_sum, stats->weight_max, stats->pixels, stats->views,
                            ctx->dn_emit.as<uint32_t>(), ctx->dn_action.as<uint8_t>(), st);
    launch_inclusive_sum_u32(ctx->dn_emit.as<uint32_t>(), ctx->dn_incl.as<uint32_t>(), P, ctx->st_scan_temp.ptr, st);
    // the call's one read-back: the new count, known before anything is scattered
    uint32_t total = 0;
    LCGS_HIP_CHECK(hipMemcpyAsync(&total, ctx->dn_incl.as<uint32_t>() + (P - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    LCGS_HIP_CHECK(hipStreamSynchronize(st));
    *new_num_gaussians = (int64_t)total;
    if ((int64_t)total > capacity) {
        set_last_error("lcgs_prune: the rewrite keeps " + std::to_string(total) + " rows, the destination arrays hold " +
                       std::to_string((long long)capacity));
        return LCGS_ERR_CAPACITY;
    }
    if (total == 0) return LCGS_OK;
    scene_arrays_written(ctx, out_activated->pos, out_activated->scale, out_activated->rotq); // (destinations a context renders)
    // (actions 0 and 1 only: no row splits, so neither the split's scale drop nor the sampler is reached)
    launch_densify_scatter(P, (int)sh_floats(sh_degree), ctx->dn_action.as<uint8_t>(), ctx->dn_incl.as<uint32_t>(),
                           adam_arrays(raw), adam_arrays(m), adam_arrays(v), adam_arrays(out_raw), adam_arrays(out_m), adam_arrays(out_v),
                           adam_arrays(out_activated), 0.0f, nullptr, 0, d_src_row, st);
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
