// abi_bilagrid.cpp -- the C ABI, part 9: per-view bilateral-grid colour correction (csrc/kernels/bilagrid.hip): the slice, its
// backward, and the total-variation term of a set of grids.
#include <limits.h>
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
bool dims_ok(int gw, int gh, int gl) { return gw >= 2 && gw <= 256 && gh >= 2 && gh <= 256 && gl >= 2 && gl <= 16; }
const char* const kDimsMessage = "grid dimensions must satisfy 2 <= gw, gh <= 256 and 2 <= gl <= 16";
} // namespace

extern "C" {

lcgs_status lcgs_bilagrid_slice(lcgs_context* ctx, int width, int height, const float* d_grid, int gw, int gh, int gl,
                                const float* d_img_chw, float* d_out_chw)
{
    LCGS_REQUIRE(ctx != nullptr, "ctx is NULL");
    LCGS_REQUIRE(d_grid && d_img_chw && d_out_chw, "NULL device pointer (grid, image or output)");
    LCGS_REQUIRE(width > 0 && height > 0, "width and height must be positive");
    LCGS_REQUIRE(dims_ok(gw, gh, gl), kDimsMessage);
    const size_t n = (size_t)width * height * 3, cells = (size_t)12 * gl * gh * gw;
    LCGS_REQUIRE(!overlaps(d_out_chw, n, d_img_chw, n) && !overlaps(d_out_chw, n, d_grid, cells),
                 "the output must not alias the image or the grid (in-place slicing is not offered)");
    LCGS_ENTRY(ctx);
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    launch_bilagrid_pixels(width, height, d_grid, { gw, gh, gl }, d_img_chw, nullptr, d_out_chw, ctx->stream);
    LCGS_HIP_CHECK(hipGetLastError());
    return LCGS_OK;
}

lcgs_status lcgs_bilagrid_backward(lcgs_context* ctx, int width, int height, const float* d_grid, int gw, int gh, int gl,
                                   const float* d_img_chw, const float* d_dL_dout_chw, float* d_dL_dimg_chw, float* d_dL_dgrid)
{
    LCGS_REQUIRE(ctx != nullptr, "ctx is NULL");
    LCGS_REQUIRE(d_grid && d_img_chw && d_dL_dout_chw, "NULL device pointer (grid, image or dL_dout)");
    LCGS_REQUIRE(width > 0 && height > 0, "width and height must be positive");
    LCGS_REQUIRE(dims_ok(gw, gh, gl), kDimsMessage);
    LCGS_REQUIRE(d_dL_dimg_chw || d_dL_dgrid, "d_dL_dimg_chw and d_dL_dgrid are both NULL: nothing to compute");
    const size_t       n = (size_t)width * height * 3, cells = (size_t)12 * gl * gh * gw;
    const float* const in[3]        = { d_grid, d_img_chw, d_dL_dout_chw };
    const size_t       in_floats[3] = { cells, n, n };
    for (int k = 0; k < 3; ++k) {
        LCGS_REQUIRE(!d_dL_dimg_chw || !overlaps(d_dL_dimg_chw, n, in[k], in_floats[k]), "a gradient buffer must not alias an input");
        LCGS_REQUIRE(!d_dL_dgrid || !overlaps(d_dL_dgrid, cells, in[k], in_floats[k]), "a gradient buffer must not alias an input");
    }
    LCGS_REQUIRE(!d_dL_dimg_chw || !d_dL_dgrid || !overlaps(d_dL_dimg_chw, n, d_dL_dgrid, cells),
                 "the gradient buffers must not alias each other");
    LCGS_ENTRY(ctx);
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    const BilagridDims d = { gw, gh, gl };
    if (d_dL_dimg_chw) launch_bilagrid_pixels(width, height, d_grid, d, d_img_chw, d_dL_dout_chw, d_dL_dimg_chw, ctx->stream);
    if (d_dL_dgrid) {
        const size_t doubles = bilagrid_grid_partial_doubles(d); // the row slices' partial sums (0: one slice, written directly)
        if (doubles) LCGS_TRY(ctx->loss_ws.ensure(doubles * sizeof(double)));
        launch_bilagrid_grid_grad(width, height, d, d_img_chw, d_dL_dout_chw, d_dL_dgrid, doubles ? ctx->loss_ws.as<double>() : nullptr,
                                  ctx->stream);
    }
    LCGS_HIP_CHECK(hipGetLastError());
    return LCGS_OK;
}

lcgs_status lcgs_bilagrid_tv_loss_backward(lcgs_context* ctx, const float* d_grids, int num_grids, int gw, int gh, int gl,
                                           float weight, float* d_dL_dgrids, float* d_loss)
{
    LCGS_REQUIRE(ctx != nullptr, "ctx is NULL");
    LCGS_REQUIRE(d_grids && d_loss, "NULL device pointer (grids or loss)");
    LCGS_REQUIRE(num_grids > 0, "num_grids must be positive");
    LCGS_REQUIRE(dims_ok(gw, gh, gl), kDimsMessage);
    LCGS_REQUIRE(isfinite(weight) && weight >= 0.0f, "weight must be finite and not negative");
    const BilagridDims d     = { gw, gh, gl };
    const size_t       cells = (size_t)num_grids * 12 * gl * gh * gw;
    LCGS_REQUIRE(bilagrid_tv_workgroups(num_grids, d) <= INT_MAX, "num_grids is too large for one call");
    LCGS_REQUIRE(!overlaps(d_loss, 1, d_grids, cells), "the loss must not alias the grids");
    LCGS_REQUIRE(!d_dL_dgrids || (!overlaps(d_dL_dgrids, cells, d_grids, cells) && !overlaps(d_dL_dgrids, cells, d_loss, 1)),
                 "the gradient buffer must not alias the grids or the loss");
    LCGS_ENTRY(ctx);
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    LCGS_TRY(ctx->loss_ws.ensure((size_t)bilagrid_tv_workgroups(num_grids, d) * sizeof(double))); // one partial per workgroup
    launch_bilagrid_tv(d_grids, num_grids, d, (double)weight, d_dL_dgrids, ctx->loss_ws.as<double>(), d_loss, ctx->stream);
    LCGS_HIP_CHECK(hipGetLastError());
    return LCGS_OK;
}

} // extern "C"
