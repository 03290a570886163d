// abi_depth_prior.cpp -- the C ABI, part 9: depth-prior supervision, the Pearson and aligned-L1 losses of a rendered depth map
// against a depth the caller brings (csrc/kernels/depth_prior.hip).
#include <math.h>

#include "abi_internal.hpp"

using namespace lcgs;
using namespace lcgs::abi;

namespace
{
struct Span {
    const void* p;
    size_t      bytes;
};
bool overlaps(const Span& a, const Span& b)
{
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a.p), pb = reinterpret_cast<uintptr_t>(b.p);
    return pa < pb + b.bytes && pb < pa + a.bytes;
}
} // namespace

extern "C" {

lcgs_status lcgs_depth_prior_loss_backward(lcgs_context* ctx, int width, int height, const float* d_depth, const float* d_alpha,
                                           const float* d_prior, const uint8_t* d_mask, const lcgs_depth_prior_config* cfg,
                                           float* d_dL_ddepth, float* d_dL_dalpha, float* d_loss, float* d_stats)
{
    LCGS_REQUIRE(ctx != nullptr, "ctx is NULL");
    LCGS_REQUIRE(cfg != nullptr, "cfg is NULL");
    LCGS_REQUIRE(d_depth && d_alpha && d_prior && d_loss, "NULL device pointer (depth, alpha, prior or loss)");
    LCGS_REQUIRE(width > 0 && height > 0, "width and height must be positive");
    LCGS_REQUIRE(cfg->kind == LCGS_DEPTH_PRIOR_PEARSON || cfg->kind == LCGS_DEPTH_PRIOR_L1, "unknown kind");
    LCGS_REQUIRE(cfg->align == LCGS_DEPTH_ALIGN_FIT || cfg->align == LCGS_DEPTH_ALIGN_GIVEN, "unknown align");
    const bool given = cfg->align == LCGS_DEPTH_ALIGN_GIVEN;
    LCGS_REQUIRE(!given || cfg->kind == LCGS_DEPTH_PRIOR_L1, "LCGS_DEPTH_ALIGN_GIVEN is for the L1 kind only");
    LCGS_REQUIRE(!given || cfg->patch == 0, "LCGS_DEPTH_ALIGN_GIVEN takes no patch (one scale and shift for the image)");
    LCGS_REQUIRE(!given || (isfinite(cfg->scale) && isfinite(cfg->shift)), "scale and shift must be finite");
    LCGS_REQUIRE(isfinite(cfg->weight) && cfg->weight >= 0.0f, "weight must be finite and not negative");
    LCGS_REQUIRE(isfinite(cfg->alpha_min) && cfg->alpha_min > 0.0f, "alpha_min must be finite and positive");
    LCGS_REQUIRE(cfg->patch == 0 || cfg->patch == 32 || cfg->patch == 64 || cfg->patch == 128, "patch must be 0, 32, 64 or 128");
    if (cfg->patch)
        LCGS_REQUIRE(cfg->patch_x >= 0 && cfg->patch_x < cfg->patch && cfg->patch_y >= 0 && cfg->patch_y < cfg->patch,
                     "patch_x and patch_y must be in [0, patch)");
    LCGS_REQUIRE((d_dL_ddepth != nullptr) == (d_dL_dalpha != nullptr), "the two gradient pointers must be both NULL or both non-NULL");
    {
        const size_t n = (size_t)width * height;
        const Span   in[4]  = { { d_depth, 4 * n }, { d_alpha, 4 * n }, { d_prior, 4 * n }, { d_mask, d_mask ? n : 0 } };
        const Span   out[4] = { { d_dL_ddepth, d_dL_ddepth ? 4 * n : 0 }, { d_dL_dalpha, d_dL_dalpha ? 4 * n : 0 }, { d_loss, 4 },
                                { d_stats, d_stats ? 16 : (size_t)0 } };
        for (int o = 0; o < 4; ++o) {
            for (int k = 0; k < 4; ++k) LCGS_REQUIRE(!overlaps(out[o], in[k]), "an output buffer must not alias an input");
            for (int k = o + 1; k < 4; ++k) LCGS_REQUIRE(!overlaps(out[o], out[k]), "the output buffers must not alias each other");
        }
    }
    LCGS_ENTRY(ctx);
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    const DepthPriorGrid grid = depth_prior_grid(width, height, cfg->patch, cfg->patch_x, cfg->patch_y);
    LCGS_TRY(ctx->loss_ws.ensure(depth_prior_workspace(grid, nullptr).doubles * sizeof(double)));
    const DepthPriorTerm term = { cfg->kind, given, cfg->patch != 0, (double)cfg->scale, (double)cfg->shift, (double)cfg->weight, (double)cfg->alpha_min };
    launch_depth_prior(grid, term, d_depth, d_alpha, d_prior, d_mask, d_dL_ddepth, d_dL_dalpha, d_loss, d_stats,
                       depth_prior_workspace(grid, ctx->loss_ws.as<double>()), ctx->stream);
    LCGS_HIP_CHECK(hipGetLastError());
    return LCGS_OK;
}

} // extern "C"
