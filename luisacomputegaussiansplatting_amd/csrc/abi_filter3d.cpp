// abi_filter3d.cpp -- the C ABI, part 9: Mip-Splatting's 3-D smoothing filter (csrc/kernels/filter3d.hip) -- per-splat sampling
// rates over the training views (accumulate, finalize), the filtered scale and opacity (apply) and their backward.  Every array
// is the caller's, in the caller's row order; the bound scene is not read.  All four calls only enqueue.
#include <math.h>

#include "abi_internal.hpp"

using namespace lcgs;
using namespace lcgs::abi;

namespace
{
bool overlaps(const float* a, size_t a_floats, const float* b, size_t b_floats) { return a < b + b_floats && b < a + a_floats; }
} // namespace

extern "C" {

lcgs_status lcgs_filter3d_accumulate(lcgs_context* ctx, int num_gaussians, const float* d_pos, int num_views,
                                     const lcgs_camera* cameras, float* d_min_z, float* max_focal)
{
    LCGS_REQUIRE(ctx && d_pos && d_min_z && max_focal, "NULL argument");
    LCGS_REQUIRE(num_gaussians >= 0, "num_gaussians is negative");
    LCGS_REQUIRE(num_views >= 0, "num_views is negative");
    LCGS_REQUIRE(num_views == 0 || cameras, "NULL cameras");
    LCGS_ENTRY(ctx);
    if (num_views == 0) return LCGS_OK;
    float focal = *max_focal;
    for (int k = 0; k < num_views; ++k) focal = fmax_(focal, make_cam_params(cameras[k]).focalx);
    *max_focal = focal;
    if (num_gaussians == 0) return LCGS_OK;
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    Filter3dViews table;
    for (int first = 0; first < num_views; first += kFilter3dViewChunk) { // one launch per chunk of the table
        const int n = std::min(num_views - first, kFilter3dViewChunk);
        for (int k = 0; k < n; ++k) {
            const CamParams cp = make_cam_params(cameras[first + k]);
            Filter3dView&   v  = table.v[k];
            for (int c = 0; c < 3; ++c) v.right[c] = cp.right[c], v.up[c] = cp.up[c], v.front[c] = cp.front[c];
            v.tx = cp.tx, v.ty = cp.ty, v.tz = cp.tz;
            v.limx = 1.3f * cp.tanfovx, v.limy = 1.3f * cp.tanfovy;
        }
        launch_filter3d_accumulate(num_gaussians, d_pos, n, table, d_min_z, ctx->stream);
    }
    LCGS_HIP_CHECK(hipGetLastError());
    return LCGS_OK;
}

lcgs_status lcgs_filter3d_finalize(lcgs_context* ctx, int num_gaussians, const float* d_min_z, float max_focal, float* d_filter)
{
    LCGS_REQUIRE(ctx && d_min_z && d_filter, "NULL argument");
    LCGS_REQUIRE(num_gaussians >= 0, "num_gaussians is negative");
    LCGS_REQUIRE(isfinite(max_focal) && max_focal > 0.0f, "max_focal must be finite and > 0");
    LCGS_ENTRY(ctx);
    if (num_gaussians == 0) return LCGS_OK;
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    LCGS_TRY(ctx->f3_word.ensure(16));
    LCGS_HIP_CHECK(hipMemsetAsync(ctx->f3_word.ptr, 0, 16, ctx->stream));
    launch_filter3d_finalize(num_gaussians, d_min_z, max_focal, ctx->f3_word.as<uint32_t>(), d_filter, ctx->stream);
    LCGS_HIP_CHECK(hipGetLastError());
    return LCGS_OK;
}

lcgs_status lcgs_filter3d_apply(lcgs_context* ctx, int num_gaussians, const float* d_scale, const float* d_opacity,
                                const float* d_filter, float* d_scale_out, float* d_opacity_out)
{
    LCGS_REQUIRE(ctx && d_scale && d_opacity && d_filter && d_scale_out && d_opacity_out, "NULL argument");
    LCGS_REQUIRE(num_gaussians >= 0, "num_gaussians is negative");
    {
        const size_t P        = (size_t)std::max(num_gaussians, 1); // (equal pointers are refused at any count)
        const float* in[3]    = { d_scale, d_opacity, d_filter };
        const size_t in_n[3]  = { 3 * P, P, P };
        bool         aliased  = overlaps(d_scale_out, 3 * P, d_opacity_out, P);
        for (int a = 0; a < 3; ++a)
            aliased = aliased || overlaps(d_scale_out, 3 * P, in[a], in_n[a]) || overlaps(d_opacity_out, P, in[a], in_n[a]);
        LCGS_REQUIRE(!aliased, "the outputs must not alias the inputs or each other (the filter is applied out of place)");
    }
    LCGS_ENTRY(ctx);
    if (num_gaussians == 0) return LCGS_OK;
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    scene_arrays_written(ctx, nullptr, d_scale_out, nullptr);
    launch_filter3d_apply(num_gaussians, d_scale, d_opacity, d_filter, d_scale_out, d_opacity_out, ctx->stream);
    LCGS_HIP_CHECK(hipGetLastError());
    return LCGS_OK;
}

lcgs_status lcgs_filter3d_backward(lcgs_context* ctx, int num_gaussians, const float* d_scale, const float* d_opacity,
                                   const float* d_filter, const uint32_t* d_rows, const uint32_t* d_count, float* d_dL_dscale,
                                   float* d_dL_dopacity)
{
    LCGS_REQUIRE(ctx && d_scale && d_opacity && d_filter && d_dL_dscale && d_dL_dopacity, "NULL argument");
    LCGS_REQUIRE(num_gaussians >= 0, "num_gaussians is negative");
    LCGS_REQUIRE((d_rows == nullptr) == (d_count == nullptr), "d_rows and d_count go together: both NULL (dense rows) or neither");
    LCGS_ENTRY(ctx);
    if (num_gaussians == 0) return LCGS_OK;
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    launch_filter3d_backward(num_gaussians, d_scale, d_opacity, d_filter, d_rows, d_count, d_dL_dscale, d_dL_dopacity, ctx->stream);
    LCGS_HIP_CHECK(hipGetLastError());
    return LCGS_OK;
}

} // extern "C"
