// abi_mcmc.cpp -- the C ABI, part 8: 3DGS-MCMC density control (csrc/kernels/mcmc.hip) -- relocation of dead splats onto live
// ones, growth towards a cap, SGLD noise on the positions, the L1 regulariser of opacity and scale.  All in place on the
// caller's arrays; the one host read-back of a relocation is its count (of a growth step: one status word).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "abi_internal.hpp"

using namespace lcgs;
using namespace lcgs::abi;

namespace
{
lcgs_status check_mcmc_config(const lcgs_mcmc_config* cfg)
{
    LCGS_REQUIRE(cfg->n_max >= 1 && cfg->n_max <= kMcmcMaxN, "n_max must be in [1,51]");
    LCGS_REQUIRE(cfg->min_opacity >= 0.0f && cfg->min_opacity < 1.0f, "min_opacity must be in [0,1)");
    return LCGS_OK;
}
// weights (+ the dead flags and d_src_row's identity when asked), their u64 sums, cleared counts and status
lcgs_status enqueue_weights(lcgs_context* ctx, int64_t P, float min_opacity, const float* raw_opacity, bool dead, uint32_t* src_row)
{
    LCGS_TRY(ctx->mc_w.ensure((size_t)P * 4));
    LCGS_TRY(ctx->mc_cdf.ensure((size_t)P * 8));
    LCGS_TRY(ctx->mc_count.ensure((size_t)P * 4));
    LCGS_TRY(ctx->st_scan_temp.ensure(scan_temp_bytes(P))); // (also the dead-row scan's, behind this one on the stream)
    LCGS_TRY(ctx->mc_status.ensure(16));
    if (dead) {
        LCGS_TRY(ctx->mc_dead.ensure((size_t)P * 4));
        LCGS_TRY(ctx->mc_dead_incl.ensure((size_t)P * 4));
        LCGS_TRY(ctx->mc_dead_list.ensure((size_t)P * 4));
    }
    hipStream_t st = ctx->stream;
    launch_mcmc_weights(P, min_opacity, raw_opacity, ctx->mc_w.as<uint32_t>(), dead ? ctx->mc_dead.as<uint32_t>() : nullptr, src_row,
                        st);
    launch_inclusive_sum_u64(ctx->mc_w.as<uint32_t>(), ctx->mc_cdf.as<uint64_t>(), P, ctx->st_scan_temp.ptr, st);
    LCGS_HIP_CHECK(hipMemsetAsync(ctx->mc_count.ptr, 0, (size_t)P * 4, st));
    LCGS_HIP_CHECK(hipMemsetAsync(ctx->mc_status.ptr, 0, 16, st));
    return LCGS_OK;
}
} // namespace

extern "C" {

lcgs_status lcgs_mcmc_relocate(lcgs_context* ctx, int num_gaussians, int sh_degree, const lcgs_mcmc_config* cfg,
                               const lcgs_params* raw, const lcgs_params* m, const lcgs_params* v, const lcgs_params* activated,
                               const uint32_t* d_src_in, uint32_t* d_src_row, int64_t* num_relocated)
{
    LCGS_REQUIRE(ctx && cfg && raw && m && v && activated && num_relocated, "NULL argument");
    LCGS_REQUIRE(num_gaussians >= 0, "num_gaussians is negative");
    LCGS_REQUIRE(sh_degree >= 0 && sh_degree <= 3, "sh_degree must be in [0,3]");
    LCGS_TRY(check_mcmc_config(cfg));
    *num_relocated = 0;
    LCGS_ENTRY(ctx);
    if (num_gaussians == 0) return LCGS_OK;
    LCGS_TRY(check_param_packs({ raw, m, v, activated }, true));
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t   st = ctx->stream;
    const int64_t P  = num_gaussians;
    LCGS_TRY(ctx->mc_draw.ensure((size_t)P * 4));
    LCGS_TRY(enqueue_weights(ctx, P, cfg->min_opacity, raw->opacity, true, d_src_row));
    uint32_t* dead_incl = ctx->mc_dead_incl.as<uint32_t>();
    launch_inclusive_sum_u32(ctx->mc_dead.as<uint32_t>(), dead_incl, P, ctx->st_scan_temp.ptr, st);
    launch_mcmc_dead_list(P, ctx->mc_dead.as<uint32_t>(), dead_incl, ctx->mc_dead_list.as<uint32_t>(), st);
    // one draw per dead row (their number stays on the device until the read-back below); only scratch is written
    launch_mcmc_draw(P, P, 0, dead_incl + (P - 1), ctx->mc_cdf.as<uint64_t>(), ctx->mc_w.as<uint32_t>(), d_src_in, cfg->seed,
                     kMcmcTagRelocate, ctx->mc_draw.as<uint32_t>(), ctx->mc_count.as<uint32_t>(), ctx->mc_status.as<uint32_t>(), st);
    // the call's one read-back: the count, with the total weight and the verdict on d_src_in
    uint32_t dead = 0, status = 0;
    uint64_t total = 0;
    LCGS_HIP_CHECK(hipMemcpyAsync(&dead, dead_incl + (P - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    LCGS_HIP_CHECK(hipMemcpyAsync(&total, ctx->mc_cdf.as<uint64_t>() + (P - 1), sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    LCGS_HIP_CHECK(hipMemcpyAsync(&status, ctx->mc_status.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    LCGS_HIP_CHECK(hipStreamSynchronize(st));
    if (dead == 0 || total == 0) return LCGS_OK; // nothing to relocate, or nothing to relocate onto
    if (status & 1u) {
        set_last_error("invalid argument: an entry of d_src_in is not a live row of the scene");
        return LCGS_ERR_INVALID_ARG;
    }
    scene_arrays_written(ctx, activated->pos, activated->scale, activated->rotq);
    const McmcRule rule = { cfg->min_opacity, cfg->n_max };
    launch_mcmc_place(dead, (int)sh_floats(sh_degree), ctx->mc_dead_list.as<uint32_t>(), 0, ctx->mc_draw.as<uint32_t>(),
                      ctx->mc_count.as<uint32_t>(), rule, adam_arrays(raw), adam_arrays(m), adam_arrays(v), adam_arrays(activated),
                      d_src_row, st);
    launch_mcmc_sources(P, (int)sh_floats(sh_degree), ctx->mc_count.as<uint32_t>(), rule, adam_arrays(raw), adam_arrays(m),
                        adam_arrays(v), adam_arrays(activated), st);
    LCGS_HIP_CHECK(hipGetLastError());
    *num_relocated = (int64_t)dead;
    return LCGS_OK;
}

lcgs_status lcgs_mcmc_add(lcgs_context* ctx, int num_gaussians, int sh_degree, const lcgs_mcmc_config* cfg, const lcgs_params* raw,
                          const lcgs_params* m, const lcgs_params* v, const lcgs_params* activated, int64_t num_new, int64_t capacity,
                          const uint32_t* d_src_in, uint32_t* d_src_row)
{
    LCGS_REQUIRE(ctx && cfg && raw && m && v && activated, "NULL argument");
    LCGS_REQUIRE(num_gaussians >= 0, "num_gaussians is negative");
    LCGS_REQUIRE(sh_degree >= 0 && sh_degree <= 3, "sh_degree must be in [0,3]");
    LCGS_REQUIRE(num_new >= 0 && capacity >= 0, "num_new or capacity is negative");
    LCGS_REQUIRE(num_new <= 0x7fffffff && capacity <= 0x7fffffff, "more than 2^31 - 1 rows");
    LCGS_TRY(check_mcmc_config(cfg));
    LCGS_ENTRY(ctx);
    const int64_t P = num_gaussians;
    if (P + num_new > capacity) {
        set_last_error("lcgs_mcmc_add: " + std::to_string((long long)(P + num_new)) + " rows, the arrays hold " +
                       std::to_string((long long)capacity));
        return LCGS_ERR_CAPACITY;
    }
    if (num_new == 0) return LCGS_OK;
    if (P == 0) {
        set_last_error("lcgs_mcmc_add: no live row to grow from");
        return LCGS_ERR_STATE;
    }
    LCGS_TRY(check_param_packs({ raw, m, v, activated }, true));
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    LCGS_TRY(ctx->mc_draw.ensure((size_t)num_new * 4));
    LCGS_TRY(enqueue_weights(ctx, P, cfg->min_opacity, raw->opacity, false, nullptr));
    launch_mcmc_draw(P, num_new, num_new, nullptr, ctx->mc_cdf.as<uint64_t>(), ctx->mc_w.as<uint32_t>(), d_src_in, cfg->seed,
                     kMcmcTagAdd, ctx->mc_draw.as<uint32_t>(), ctx->mc_count.as<uint32_t>(), ctx->mc_status.as<uint32_t>(), st);
    // the call's one read-back: a status word (no live row; a bad entry of d_src_in) -- nothing of the caller's is written before
    uint32_t status = 0;
    LCGS_HIP_CHECK(hipMemcpyAsync(&status, ctx->mc_status.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    LCGS_HIP_CHECK(hipStreamSynchronize(st));
    if (status & 2u) {
        set_last_error("lcgs_mcmc_add: no live row to grow from");
        return LCGS_ERR_STATE;
    }
    if (status & 1u) {
        set_last_error("invalid argument: an entry of d_src_in is not a live row of the scene");
        return LCGS_ERR_INVALID_ARG;
    }
    scene_arrays_written(ctx, activated->pos, activated->scale, activated->rotq);
    const McmcRule rule = { cfg->min_opacity, cfg->n_max };
    launch_mcmc_place(num_new, (int)sh_floats(sh_degree), nullptr, P, ctx->mc_draw.as<uint32_t>(), ctx->mc_count.as<uint32_t>(), rule,
                      adam_arrays(raw), adam_arrays(m), adam_arrays(v), adam_arrays(activated), d_src_row, st);
    launch_mcmc_sources(P, (int)sh_floats(sh_degree), ctx->mc_count.as<uint32_t>(), rule, adam_arrays(raw), adam_arrays(m),
                        adam_arrays(v), adam_arrays(activated), st);
    LCGS_HIP_CHECK(hipGetLastError());
    return LCGS_OK;
}

lcgs_status lcgs_mcmc_noise(lcgs_context* ctx, int num_gaussians, const lcgs_mcmc_noise_config* cfg, const lcgs_params* raw,
                            const lcgs_params* activated, const float* d_noise)
{
    LCGS_REQUIRE(ctx && cfg && raw && activated, "NULL argument");
    LCGS_REQUIRE(num_gaussians >= 0, "num_gaussians is negative");
    LCGS_ENTRY(ctx);
    if (num_gaussians == 0) return LCGS_OK;
    LCGS_REQUIRE(raw->pos && raw->scale && raw->rotq && raw->opacity && activated->pos, "NULL device pointer in a parameter pack");
    LCGS_REQUIRE((reinterpret_cast<uintptr_t>(raw->rotq) & 15) == 0, "rotq arrays must be 16-byte aligned");
    scene_arrays_written(ctx, activated->pos, activated->scale, activated->rotq);
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    launch_mcmc_noise(num_gaussians, cfg->noise_lr * cfg->lr_pos, cfg->k, cfg->x0, raw->opacity, raw->scale, raw->rotq, d_noise,
                      cfg->seed, (uint32_t)cfg->step, raw->pos, activated->pos, ctx->stream);
    LCGS_HIP_CHECK(hipGetLastError());
    return LCGS_OK;
}

lcgs_status lcgs_mcmc_regularize(lcgs_context* ctx, int num_gaussians, float lambda_opacity, float lambda_scale,
                                 const lcgs_grads* grads)
{
    LCGS_REQUIRE(ctx && grads, "NULL argument");
    LCGS_REQUIRE(num_gaussians >= 0, "num_gaussians is negative");
    LCGS_ENTRY(ctx);
    if (num_gaussians == 0) return LCGS_OK;
    LCGS_REQUIRE(grads->d_dL_dopacity && grads->d_dL_dscale, "NULL gradient pointer (opacity and scale are needed)");
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    // the two addends, each rounded once from the double value
    const float add_o = (float)((double)lambda_opacity / (double)num_gaussians);
    const float add_s = (float)((double)lambda_scale / (3.0 * (double)num_gaussians));
    launch_mcmc_regularize(num_gaussians, add_o, add_s, grads->d_dL_dopacity, grads->d_dL_dscale, ctx->stream);
    LCGS_HIP_CHECK(hipGetLastError());
    return LCGS_OK;
}

} // extern "C"
