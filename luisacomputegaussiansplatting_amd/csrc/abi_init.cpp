// abi_init.cpp -- the C ABI, part 9: a scene from a point cloud (csrc/kernels/init.hip) -- the exact 3-nearest-neighbour mean
// squared distance, 3DGS's create_from_pcd rows, and the camera extent (getNerfppNorm) that lcgs_densify_config.scene_extent wants.
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "abi_internal.hpp"

using namespace lcgs;
using namespace lcgs::abi;

static_assert(kKnnChunk == LCGS_KNN_CHUNK, "the header's chunk size is the kernels'");

namespace
{
// box -> Morton sort -> sorted points + chunk boxes -> query; everything on the context's stream, nothing read back
lcgs_status enqueue_knn(lcgs_context* ctx, int64_t n, const float* d_pos, float* d_dist2)
{
    hipStream_t   st     = ctx->stream;
    const int64_t chunks = div_up64(n, kKnnChunk);
    for (int i = 0; i < 2; ++i) {
        LCGS_TRY(ctx->knn_keys[i].ensure((size_t)n * 4));
        LCGS_TRY(ctx->knn_vals[i].ensure((size_t)n * 4));
    }
    LCGS_TRY(ctx->knn_sort_ws.ensure(pair_sort_ws_bytes(n)));
    LCGS_TRY(ctx->knn_sorted.ensure((size_t)n * sizeof(float4)));
    LCGS_TRY(ctx->knn_boxes.ensure((size_t)chunks * 2 * sizeof(float4)));
    LCGS_TRY(ctx->knn_grid.ensure(sizeof(KnnGrid) + knn_box_partial_bytes()));
    KnnGrid* grid    = ctx->knn_grid.as<KnnGrid>();
    void*    partial = ctx->knn_grid.as<char>() + sizeof(KnnGrid);
    ctx->n_marks     = 0;
    LCGS_TRY(mark(ctx, "start"));
    launch_knn_grid(n, d_pos, partial, grid, st);
    LCGS_TRY(mark(ctx, "knn_box"));
    launch_morton_keys(n, d_pos, grid->lo, ctx->knn_keys[0].as<uint32_t>(), ctx->knn_vals[0].as<uint32_t>(), st);
    const int where = launch_pair_sort_u32(ctx->knn_keys[0].as<uint32_t>(), ctx->knn_keys[1].as<uint32_t>(),
                                           ctx->knn_vals[0].as<uint32_t>(), ctx->knn_vals[1].as<uint32_t>(), nullptr, n, n, 0, 30,
                                           ctx->knn_sort_ws.ptr, st);
    LCGS_TRY(mark(ctx, "knn_sort"));
    launch_knn_gather_boxes(n, d_pos, ctx->knn_vals[where].as<uint32_t>(), ctx->knn_sorted.as<float4>(),
                            ctx->knn_boxes.as<float4>(), st);
    LCGS_TRY(mark(ctx, "knn_boxes"));
    launch_knn_query(n, ctx->knn_sorted.as<float4>(), ctx->knn_boxes.as<float4>(), grid, d_dist2, st);
    LCGS_TRY(mark(ctx, "knn_query"));
    LCGS_HIP_CHECK(hipGetLastError());
    return LCGS_OK;
}
} // namespace

extern "C" {

lcgs_status lcgs_knn_mean_dist2(lcgs_context* ctx, int64_t num_points, const float* d_pos, float* d_dist2)
{
    LCGS_REQUIRE(ctx != nullptr, "NULL context");
    LCGS_REQUIRE(num_points >= 0, "num_points is negative");
    LCGS_REQUIRE(num_points <= (int64_t)INT32_MAX, "num_points exceeds 2^31 - 1 (the original index travels in 32 bits)");
    if (num_points == 0) return LCGS_OK;
    LCGS_REQUIRE(d_pos && d_dist2, "NULL device pointer");
    LCGS_ENTRY(ctx);
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    LCGS_TRY(enqueue_knn(ctx, num_points, d_pos, d_dist2));
    if (ctx->profiling) LCGS_TRY(collect_marks(ctx));
    return LCGS_OK;
}

lcgs_status lcgs_scene_init_from_points(lcgs_context* ctx, int num_points, int sh_degree, const float* d_pos, const float* d_rgb,
                                        const lcgs_init_config* cfg, const lcgs_params* out_raw, const lcgs_params* out_activated)
{
    LCGS_REQUIRE(ctx && cfg && out_raw && out_activated, "NULL argument");
    LCGS_REQUIRE(num_points >= 0, "num_points is negative");
    LCGS_REQUIRE(sh_degree >= 0 && sh_degree <= 3, "sh_degree must be in [0,3]");
    LCGS_REQUIRE(cfg->initial_opacity > 0.0f && cfg->initial_opacity < 1.0f, "initial_opacity must be in (0,1)");
    LCGS_REQUIRE(cfg->min_dist2 > 0.0f, "min_dist2 must be > 0");
    if (num_points == 0) return LCGS_OK;
    LCGS_REQUIRE(d_pos && d_rgb, "NULL device pointer");
    LCGS_TRY(check_param_packs({ out_raw, out_activated }, true));
    LCGS_ENTRY(ctx);
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    const int64_t n = num_points;
    LCGS_TRY(ctx->knn_dist2.ensure((size_t)n * 4));
    LCGS_TRY(enqueue_knn(ctx, n, d_pos, ctx->knn_dist2.as<float>()));
    scene_arrays_written(ctx, out_activated->pos, out_activated->scale, out_activated->rotq); // (destinations a context renders)
    // logit(initial_opacity) to binary32, rounded once from the double value
    const double p           = (double)cfg->initial_opacity;
    const float  raw_opacity = (float)log(p / (1.0 - p));
    launch_init_rows(n, (int)sh_floats(sh_degree), d_pos, d_rgb, ctx->knn_dist2.as<float>(), cfg->min_dist2, raw_opacity,
                     adam_arrays(out_raw), adam_arrays(out_activated), ctx->stream);
    LCGS_TRY(mark(ctx, "init_rows"));
    LCGS_HIP_CHECK(hipGetLastError());
    if (ctx->profiling) LCGS_TRY(collect_marks(ctx));
    return LCGS_OK;
}

lcgs_status lcgs_scene_extent(int num_cameras, const lcgs_camera* cameras, float center[3], float* radius)
{
    LCGS_REQUIRE(cameras && center && radius, "NULL argument");
    LCGS_REQUIRE(num_cameras >= 1, "num_cameras must be >= 1");
    double c[3] = { 0.0, 0.0, 0.0 };
    for (int i = 0; i < num_cameras; ++i)
        for (int a = 0; a < 3; ++a) c[a] += (double)cameras[i].position[a];
    for (int a = 0; a < 3; ++a) c[a] /= (double)num_cameras;
    double far = 0.0;
    for (int i = 0; i < num_cameras; ++i) {
        const double dx = (double)cameras[i].position[0] - c[0], dy = (double)cameras[i].position[1] - c[1],
                     dz = (double)cameras[i].position[2] - c[2];
        far = std::max(far, sqrt((dx * dx + dy * dy) + dz * dz));
    }
    for (int a = 0; a < 3; ++a) center[a] = (float)c[a];
    *radius = (float)(far * 1.1);
    return LCGS_OK;
}

} // extern "C"
