// abi_loss.cpp -- the C ABI, part 8: the 3DGS photometric loss (csrc/kernels/loss.hip) and the choice of the loss that
// lcgs_fit_views applies.
#include <math.h>

#include "abi_internal.hpp"

using namespace lcgs;
using namespace lcgs::abi;

namespace
{
bool overlaps(const float* a, const float* b, size_t floats)
{
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b), len = floats * sizeof(float);
    return pa < pb + len && pb < pa + len;
}
} // namespace

extern "C" {

lcgs_status lcgs_photometric_loss_backward(lcgs_context* ctx, int width, int height, const float* d_img_chw,
                                           const float* d_target_chw, float lambda_dssim, float* d_dL_dimg, float* d_loss,
                                           float* d_terms)
{
    LCGS_REQUIRE(ctx != nullptr, "ctx is NULL");
    LCGS_REQUIRE(d_img_chw && d_target_chw && d_loss, "NULL device pointer (image, target or loss)");
    LCGS_REQUIRE(width > 0 && height > 0, "width and height must be positive");
    LCGS_REQUIRE(isfinite(lambda_dssim) && lambda_dssim >= 0.0f && lambda_dssim <= 1.0f, "lambda_dssim must be in [0,1]");
    const size_t n = (size_t)width * height * 3;
    LCGS_REQUIRE(!d_dL_dimg || (!overlaps(d_dL_dimg, d_img_chw, n) && !overlaps(d_dL_dimg, d_target_chw, n)),
                 "d_dL_dimg must not alias the image or the target");
    LCGS_ENTRY(ctx);
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    // workspace: one pair of doubles per workgroup, then (gradient calls with an SSIM term) the planes a, b, c
    const size_t pair_bytes = (size_t)photometric_workgroups(width, height) * 2 * sizeof(double);
    const bool   planes     = d_dL_dimg != nullptr && lambda_dssim != 0.0f;
    LCGS_TRY(ctx->loss_ws.ensure(pair_bytes + (planes ? 3 * n * sizeof(float) : 0)));
    double* partials = ctx->loss_ws.as<double>();
    float*  abc      = planes ? reinterpret_cast<float*>(ctx->loss_ws.as<char>() + pair_bytes) : nullptr;
    launch_photometric_stats(width, height, d_img_chw, d_target_chw, abc, partials, ctx->stream);
    if (d_dL_dimg) launch_photometric_grad(width, height, d_img_chw, d_target_chw, abc, lambda_dssim, d_dL_dimg, ctx->stream);
    launch_photometric_finish(width, height, partials, lambda_dssim, d_loss, d_terms, ctx->stream);
    LCGS_HIP_CHECK(hipGetLastError());
    return LCGS_OK;
}

lcgs_status lcgs_set_fit_loss(lcgs_context* ctx, int kind, float lambda_dssim)
{
    LCGS_REQUIRE(ctx != nullptr, "ctx is NULL");
    LCGS_REQUIRE(kind == LCGS_LOSS_L2 || kind == LCGS_LOSS_PHOTOMETRIC, "unknown loss kind");
    LCGS_REQUIRE(isfinite(lambda_dssim) && lambda_dssim >= 0.0f && lambda_dssim <= 1.0f, "lambda_dssim must be in [0,1]");
    LCGS_ENTRY(ctx);
    ctx->fit_loss   = kind;
    ctx->fit_lambda = lambda_dssim;
    return LCGS_OK;
}

} // extern "C"
