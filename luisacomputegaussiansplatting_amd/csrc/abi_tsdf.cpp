// abi_tsdf.cpp -- the C ABI, part 10: a surface out of the trained scene (csrc/kernels/tsdf.hip) -- TSDF fusion of a batch of depth
// maps into a caller-owned dense volume, and the volume's zero level set as a welded triangle mesh by marching tetrahedra.  The
// bound scene is not read and no kept frame is needed.  lcgs_tsdf_integrate only enqueues; the two mesh calls read the counts back.
#include <math.h>

#include "abi_internal.hpp"

using namespace lcgs;
using namespace lcgs::abi;

namespace
{
bool overlaps(const float* a, size_t a_floats, const float* b, size_t b_floats)
{
    return a && b && (uintptr_t)a < (uintptr_t)b + 4 * b_floats && (uintptr_t)b < (uintptr_t)a + 4 * a_floats;
}

lcgs_status check_volume(const lcgs_tsdf_volume* vol)
{
    LCGS_REQUIRE(vol, "NULL volume");
    LCGS_REQUIRE(vol->nx >= 1 && vol->ny >= 1 && vol->nz >= 1, "a lattice dimension is below 1");
    LCGS_REQUIRE((int64_t)vol->nx * vol->ny <= 0x7FFFFFFFll && (int64_t)vol->nx * vol->ny * vol->nz <= 0x7FFFFFFFll,
                 "the volume has more than 2^31 - 1 samples");
    LCGS_REQUIRE(isfinite(vol->voxel_size) && vol->voxel_size > 0.0f, "voxel_size must be finite and > 0");
    LCGS_REQUIRE(isfinite(vol->origin[0]) && isfinite(vol->origin[1]) && isfinite(vol->origin[2]), "the origin must be finite");
    LCGS_REQUIRE(vol->d_tsdf && vol->d_weight, "NULL volume array");
    const size_t n = (size_t)vol->nx * vol->ny * vol->nz;
    LCGS_REQUIRE(!overlaps(vol->d_tsdf, n, vol->d_weight, n) && !overlaps(vol->d_tsdf, n, vol->d_rgb, 3 * n) &&
                     !overlaps(vol->d_weight, n, vol->d_rgb, 3 * n),
                 "the volume's arrays overlap each other");
    return LCGS_OK;
}

TsdfGrid grid_of(const lcgs_tsdf_volume* vol)
{
    return { { vol->origin[0], vol->origin[1], vol->origin[2] }, vol->voxel_size, vol->nx, vol->ny, vol->nz };
}

// the cell pass and the counts of the volume's mesh: leaves ts_word, ts_vcount, ts_tcount (not yet scanned) and reads the totals back
lcgs_status mesh_counts(lcgs_context* ctx, const lcgs_tsdf_volume* vol, float weight_min, uint64_t* nv, uint64_t* nt)
{
    *nv = *nt = 0;
    if (vol->nx == 1 || vol->ny == 1 || vol->nz == 1) return LCGS_OK; // no cells
    const TsdfGrid g = grid_of(vol);
    const int64_t  n = (int64_t)g.nx * g.ny * g.nz;
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    LCGS_TRY(ctx->ts_word.ensure((size_t)n * 4));
    LCGS_TRY(ctx->ts_vcount.ensure((size_t)n * 4));
    LCGS_TRY(ctx->ts_tcount.ensure((size_t)n * 4));
    LCGS_TRY(ctx->ts_scan_temp.ensure(scan_temp_bytes(n)));
    LCGS_TRY(ctx->ts_totals.ensure(16));
    LCGS_HIP_CHECK(hipMemsetAsync(ctx->ts_word.ptr, 0, (size_t)n * 4, ctx->stream));
    LCGS_HIP_CHECK(hipMemsetAsync(ctx->ts_totals.ptr, 0, 16, ctx->stream));
    launch_tsdf_mesh_cells(g, vol->d_tsdf, vol->d_weight, weight_min, ctx->ts_word.as<uint32_t>(), ctx->stream);
    launch_tsdf_mesh_counts(n, ctx->ts_word.as<uint32_t>(), ctx->ts_vcount.as<uint32_t>(), ctx->ts_tcount.as<uint32_t>(),
                            ctx->ts_totals.as<unsigned long long>(), ctx->stream);
    LCGS_HIP_CHECK(hipGetLastError());
    unsigned long long totals[2] = { 0, 0 };
    LCGS_HIP_CHECK(hipMemcpyAsync(totals, ctx->ts_totals.ptr, 16, hipMemcpyDeviceToHost, ctx->stream));
    LCGS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    *nv = totals[0], *nt = totals[1];
    return LCGS_OK;
}
} // namespace

extern "C" {

lcgs_status lcgs_tsdf_integrate(lcgs_context* ctx, const lcgs_tsdf_volume* volume, const lcgs_tsdf_config* cfg, int num_views,
                                const lcgs_camera* cameras, const float* const* d_depths, const float* const* d_alphas,
                                const float* const* d_images)
{
    LCGS_REQUIRE(ctx && cfg, "NULL argument");
    LCGS_TRY(check_volume(volume));
    LCGS_REQUIRE(isfinite(cfg->trunc) && cfg->trunc > 0.0f, "trunc must be finite and > 0");
    LCGS_REQUIRE(isfinite(cfg->depth_max) && cfg->depth_max > 0.0f, "depth_max must be finite and > 0");
    LCGS_REQUIRE(isfinite(cfg->alpha_min) && cfg->alpha_min > 0.0f, "alpha_min must be finite and > 0");
    LCGS_REQUIRE(num_views >= 0, "num_views is negative");
    LCGS_REQUIRE(num_views == 0 || (cameras && d_depths), "NULL cameras or d_depths");
    {
        const size_t n          = (size_t)volume->nx * volume->ny * volume->nz;
        const float* arr[3]     = { volume->d_tsdf, volume->d_weight, volume->d_rgb };
        const size_t arr_n[3]   = { n, n, 3 * n };
        for (int k = 0; k < num_views; ++k) {
            LCGS_REQUIRE(cameras[k].width >= 1 && cameras[k].height >= 1, "a camera's width or height is below 1");
            LCGS_REQUIRE(d_depths[k], "NULL depth map");
            const size_t pixels  = (size_t)cameras[k].width * cameras[k].height;
            const float* map[3]  = { d_depths[k], d_alphas ? d_alphas[k] : nullptr, d_images ? d_images[k] : nullptr };
            const size_t map_n[3] = { pixels, pixels, 3 * pixels };
            bool         aliased = false;
            for (int a = 0; a < 3; ++a)
                for (int m = 0; m < 3; ++m) aliased = aliased || overlaps(arr[a], arr_n[a], map[m], map_n[m]);
            LCGS_REQUIRE(!aliased, "a volume array overlaps an input map");
        }
    }
    LCGS_ENTRY(ctx);
    if (num_views == 0) return LCGS_OK;
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    const TsdfGrid g = grid_of(volume);
    TsdfViews      table;
    for (int first = 0; first < num_views; first += kTsdfViewChunk) { // one launch per chunk of the table
        const int n = std::min(num_views - first, kTsdfViewChunk);
        for (int k = 0; k < n; ++k) {
            const lcgs_camera& cam = cameras[first + k];
            const CamParams    cp  = make_cam_params(cam);
            TsdfView&          v   = table.v[k];
            for (int c = 0; c < 3; ++c) v.right[c] = cp.right[c], v.up[c] = cp.up[c], v.front[c] = cp.front[c];
            v.tx = cp.tx, v.ty = cp.ty, v.tz = cp.tz;
            v.inv_tanx = cp.inv_tanx, v.inv_tany = cp.inv_tany;
            v.W = cam.width, v.H = cam.height;
            v.depth = d_depths[first + k];
            v.alpha = d_alphas ? d_alphas[first + k] : nullptr;
            v.image = d_images ? d_images[first + k] : nullptr;
        }
        launch_tsdf_integrate(g, volume->d_tsdf, volume->d_weight, volume->d_rgb, cfg->trunc, cfg->depth_max, cfg->alpha_min, n, table,
                              ctx->stream);
    }
    LCGS_HIP_CHECK(hipGetLastError());
    return LCGS_OK;
}

lcgs_status lcgs_tsdf_mesh_count(lcgs_context* ctx, const lcgs_tsdf_volume* volume, float weight_min, uint64_t* num_vertices,
                                 uint64_t* num_triangles)
{
    LCGS_REQUIRE(ctx && num_vertices && num_triangles, "NULL argument");
    LCGS_TRY(check_volume(volume));
    LCGS_REQUIRE(isfinite(weight_min) && weight_min > 0.0f, "weight_min must be finite and > 0");
    LCGS_ENTRY(ctx);
    return mesh_counts(ctx, volume, weight_min, num_vertices, num_triangles);
}

lcgs_status lcgs_tsdf_mesh_extract(lcgs_context* ctx, const lcgs_tsdf_volume* volume, float weight_min, uint64_t cap_vertices,
                                   uint64_t cap_triangles, float* d_vertices, float* d_vertex_rgb, uint32_t* d_triangles,
                                   uint64_t* num_vertices, uint64_t* num_triangles)
{
    LCGS_REQUIRE(ctx && num_vertices && num_triangles, "NULL argument");
    LCGS_TRY(check_volume(volume));
    LCGS_REQUIRE(isfinite(weight_min) && weight_min > 0.0f, "weight_min must be finite and > 0");
    LCGS_REQUIRE((cap_vertices == 0 || d_vertices) && (cap_triangles == 0 || d_triangles), "NULL output array of a non-zero capacity");
    LCGS_REQUIRE(!d_vertex_rgb || volume->d_rgb, "vertex colours asked of a volume without colour");
    LCGS_ENTRY(ctx);
    LCGS_TRY(mesh_counts(ctx, volume, weight_min, num_vertices, num_triangles));
    const uint64_t nv = *num_vertices, nt = *num_triangles;
    if (nv > cap_vertices || nt > cap_triangles || nv >= ((uint64_t)1 << 32) || nt >= ((uint64_t)1 << 32)) {
        set_last_error("lcgs_tsdf_mesh_extract: the mesh has " + std::to_string(nv) + " vertices and " + std::to_string(nt) +
                       " triangles: more than the capacities, or than 2^32 - 1");
        return LCGS_ERR_CAPACITY;
    }
    if (nv == 0) return LCGS_OK;
    const TsdfGrid g = grid_of(volume);
    const int64_t  n = (int64_t)g.nx * g.ny * g.nz;
    uint32_t *     word = ctx->ts_word.as<uint32_t>(), *vincl = ctx->ts_vcount.as<uint32_t>(), *tincl = ctx->ts_tcount.as<uint32_t>();
    launch_inclusive_sum_u32(vincl, vincl, n, ctx->ts_scan_temp.ptr, ctx->stream); // in place: a block reads its tile before it writes it
    launch_inclusive_sum_u32(tincl, tincl, n, ctx->ts_scan_temp.ptr, ctx->stream);
    launch_tsdf_mesh_vertices(g, volume->d_tsdf, volume->d_rgb, word, vincl, d_vertices, d_vertex_rgb, ctx->stream);
    launch_tsdf_mesh_triangles(g, volume->d_tsdf, word, vincl, tincl, d_triangles, ctx->stream);
    LCGS_HIP_CHECK(hipGetLastError());
    return LCGS_OK;
}

} // extern "C"
