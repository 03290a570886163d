// abi_loss.cpp -- the C ABI, part 8: the 3DGS photometric loss and the normal-consistency loss (csrc/kernels/loss.hip) and the
// choice of the loss that lcgs_fit_views applies.
#include <math.h>

#include "abi_internal.hpp"

using namespace lcgs;
using namespace lcgs::abi;

namespace
{
bool overlaps(const float* a, size_t a_floats, const float* b, size_t b_floats)
{
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + b_floats * sizeof(float) && pb < pa + a_floats * sizeof(float);
}
bool overlaps(const float* a, const float* b, size_t floats) { return overlaps(a, floats, b, floats); }
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

lcgs_status lcgs_normal_consistency_loss_backward(lcgs_context* ctx, const lcgs_camera* camera, const float* d_depth,
                                                  const float* d_alpha, const float* d_normal, float weight, float alpha_min,
                                                  float* d_dL_ddepth, float* d_dL_dalpha, float* d_dL_dnormal, float* d_loss)
{
    LCGS_REQUIRE(ctx != nullptr, "ctx is NULL");
    LCGS_REQUIRE(camera != nullptr, "camera is NULL");
    LCGS_REQUIRE(d_depth && d_alpha && d_normal && d_loss, "NULL device pointer (depth, alpha, normal or loss)");
    LCGS_REQUIRE(camera->width >= 3 && camera->height >= 3, "width and height must be at least 3 (no interior pixel)");
    LCGS_REQUIRE(isfinite(weight) && weight >= 0.0f, "weight must be finite and not negative");
    LCGS_REQUIRE(isfinite(alpha_min) && alpha_min > 0.0f, "alpha_min must be finite and positive");
    const int  num_grads = (d_dL_ddepth != nullptr) + (d_dL_dalpha != nullptr) + (d_dL_dnormal != nullptr);
    LCGS_REQUIRE(num_grads == 0 || num_grads == 3, "the three gradient pointers must be all NULL or all non-NULL");
    const int    W = camera->width, H = camera->height;
    const size_t n = (size_t)W * H;
    if (num_grads) { // the gather reads neighbours: a gradient written over an input or over another gradient corrupts it
        const float* const in[3]     = { d_depth, d_alpha, d_normal };
        float* const       out[3]    = { d_dL_ddepth, d_dL_dalpha, d_dL_dnormal };
        const size_t       floats[3] = { n, n, 3 * n };
        for (int g = 0; g < 3; ++g) {
            for (int k = 0; k < 3; ++k)
                LCGS_REQUIRE(!overlaps(out[g], floats[g], in[k], floats[k]), "a gradient buffer must not alias an input");
            for (int k = g + 1; k < 3; ++k)
                LCGS_REQUIRE(!overlaps(out[g], floats[g], out[k], floats[k]), "the gradient buffers must not alias each other");
        }
    }
    LCGS_ENTRY(ctx);
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    LCGS_TRY(ctx->loss_ws.ensure((size_t)normal_consistency_workgroups(W, H) * sizeof(double))); // one partial per workgroup
    const double tany = tan((double)camera->fov / 180.0 * M_PI * 0.5), tanx = tany * (double)camera->aspect_ratio;
    const double scale = (double)weight / ((double)(W - 2) * (double)(H - 2));
    launch_normal_consistency(W, H, tanx, tany, scale, (double)alpha_min, d_depth, d_alpha, d_normal, d_dL_ddepth, d_dL_dalpha,
                              d_dL_dnormal, ctx->loss_ws.as<double>(), d_loss, ctx->stream);
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
