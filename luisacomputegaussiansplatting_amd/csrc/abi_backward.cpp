// abi_backward.cpp -- the C ABI, part 5: the backward of the fused frame -- dense per-splat rows, compact
// rows, accumulation over views, and the variant with the optimiser folded into the per-splat pass -- and the frame's depth
// alpha, depth-distortion and normal maps with their backward (kernels/maps.hip), the caller's feature channels with theirs (kernels/features.hip), the per-splat blend-weight statistics of the same kept
// lists (kernels/contrib.hip), and the camera gradient (kernels/camera_grad.hip).
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
// What a backward of the last keep-state frame is asked for: the incoming gradients, and where the result goes.
struct BackwardRequest {
    // the incoming gradients of the image, of the depth and alpha maps (about depth mode `mode`) and of the distortion map
    // (about `center`): any may be NULL, not all
    const float *d_dL_dimg = nullptr, *d_dL_ddepth = nullptr, *d_dL_dalpha = nullptr, *d_dL_ddist = nullptr;
    const float *d_dL_dnormal = nullptr; // ... and of the normal map (dense rows only)
    // ... and the caller's feature channel (dense rows only): its rows, the map's incoming gradient, where dL/dfeatures goes
    const lcgs_feature_channel* feat = nullptr;
    int          mode   = kDepthZ;
    float        center = 0.0f;
    // exactly one destination: per-splat rows in `grads` (dense, dense added to what the arrays hold, or compact), the
    // optimiser folded into the per-splat pass (no gradient arrays at all), or the camera's twelve numbers alone
    enum Dest { Dense, DenseAccumulate, Compact, FusedAdam, CameraOnly } dest = Dense;
    const lcgs_grads* grads = nullptr;   // Dense, DenseAccumulate, Compact
    AdamArrays        raw{}, m{}, v{}, act{}; // FusedAdam
    AdamRates         lr{};
    AdamStep          step{};
    float*            d_dL_dcam = nullptr; // CameraOnly

    bool maps() const { return d_dL_ddepth || d_dL_dalpha || d_dL_ddist || d_dL_dnormal; }
    bool value_channel() const { return d_dL_ddepth || d_dL_ddist; } // something arrives in the rows' value slot
    bool rows() const { return dest == Dense || dest == DenseAccumulate || dest == Compact; }
};
lcgs_status render_backward(lcgs_context* ctx, const BackwardRequest& req);
lcgs_status features_only_backward(lcgs_context* ctx, const lcgs_feature_channel& feat, bool accumulate);
// the camera pass over the 2-D rows the context holds (kernels/camera_grad.hip)
lcgs_status camera_pass(lcgs_context* ctx, float* d_dL_dcam)
{
    LCGS_TRY(ctx->cam_slab.ensure(camera_grad_slab_bytes((int64_t)ctx->P)));
    launch_camera_grad(kept_rows(ctx), ctx->g2d_value_mode, ctx->cam_slab.as<double>(), d_dL_dcam, ctx->stream);
    return LCGS_OK;
}
BackwardRequest rows_request(const float* d_dL_dimg, const lcgs_grads* grads, BackwardRequest::Dest dest)
{
    BackwardRequest req;
    req.d_dL_dimg = d_dL_dimg, req.grads = grads, req.dest = dest;
    return req;
}
}

lcgs_status lcgs::abi::check_own_kept_frame(lcgs_context* ctx, const char* who, const char* owner_frame, const char* no_frame)
{
    if (!ctx->frame_state_valid() || !ctx->last.has_state) {
        const std::string plain = std::string(who) + " needs a preceding lcgs_render_forward(..., keep_state = 1)";
        set_last_error(no_frame ? no_frame : plain.c_str());
        return LCGS_ERR_STATE;
    }
    if (ctx->owner_recs) { // the last frame was lcgs_owner_render's: its records are not this context's own
        const std::string plain = std::string(who) + ": the last frame was drawn from received records (lcgs_owner_render)";
        set_last_error(owner_frame ? owner_frame : plain.c_str());
        return LCGS_ERR_STATE;
    }
    // (lcgs_render_forward never puts a frame that keeps state on per-block lists)
    LCGS_REQUIRE(ctx->last.cp.list_shift == 0u, "the kept frame lists its pairs per block: no backward walks those lists");
    return LCGS_OK;
}

extern "C" {

lcgs_status lcgs_render_backward(lcgs_context* ctx, const float* d_dL_dimg, const lcgs_grads* grads)
{
    LCGS_ENTRY(ctx);
    return render_backward(ctx, rows_request(d_dL_dimg, grads, BackwardRequest::Dense));
}

lcgs_status lcgs_render_backward_compact(lcgs_context* ctx, const float* d_dL_dimg, const lcgs_grads* grads)
{
    LCGS_ENTRY(ctx);
    return render_backward(ctx, rows_request(d_dL_dimg, grads, BackwardRequest::Compact));
}

lcgs_status lcgs_render_backward_accumulate(lcgs_context* ctx, const float* d_dL_dimg, const lcgs_grads* grads)
{
    LCGS_ENTRY(ctx);
    return render_backward(ctx, rows_request(d_dL_dimg, grads, BackwardRequest::DenseAccumulate));
}

lcgs_status lcgs_render_backward_adam(lcgs_context* ctx, const float* d_dL_dimg, int num_gaussians, int sh_degree,
                                      const lcgs_adam_config* cfg, const lcgs_params* raw, const lcgs_params* m,
                                      const lcgs_params* v, const lcgs_params* activated)
{
    LCGS_REQUIRE(ctx && d_dL_dimg && cfg && raw && m && v && activated, "NULL argument");
    LCGS_ENTRY(ctx);
    LCGS_REQUIRE(num_gaussians == ctx->P && sh_degree == ctx->sh_deg, "num_gaussians / sh_degree must be the bound scene's");
    LCGS_TRY(check_adam_config(cfg));
    LCGS_TRY(check_param_packs({ raw, m, v, activated }, false));
    auto aligned16 = [](const lcgs_params* p) {
        return ((reinterpret_cast<uintptr_t>(p->rotq) | reinterpret_cast<uintptr_t>(p->sh)) & 15) == 0;
    };
    const bool fusable = ctx->sh_deg == 3 && ctx->frame_state_valid() && ctx->last.has_state && ctx->last_has_jac && aligned16(raw) &&
                         aligned16(m) && aligned16(v) && aligned16(activated);
    if (!fusable) {
        // other SH degrees, frames without the kept colour Jacobian, unaligned rows: the same step as two calls on
        // context-owned compact gradient rows (identical result; the fused kernel exists for the degree-3 training case)
        LCGS_HIP_CHECK(hipSetDevice(ctx->device));
        const size_t feat = sh_floats(ctx->sh_deg);
        const size_t rows = (size_t)ctx->P;
        auto         al   = [](size_t x) { return (x + 3) & ~(size_t)3; }; // every array starts on a 16-byte boundary
        const size_t o_scale = al(rows * 3), o_rotq = al(o_scale + rows * 3), o_sh = al(o_rotq + rows * 4),
                     o_op = al(o_sh + rows * feat);
        LCGS_TRY(ctx->fused_grads.ensure((o_op + rows) * 4));
        float*     g  = ctx->fused_grads.as<float>();
        lcgs_grads gr = { g, g + o_scale, g + o_rotq, g + o_sh, g + o_op };
        LCGS_TRY(render_backward(ctx, rows_request(d_dL_dimg, &gr, BackwardRequest::Compact)));
        lcgs_adam_config c2 = *cfg;
        c2.visible_only     = 2;
        return lcgs_adam_step(ctx, num_gaussians, sh_degree, &c2, &gr, raw, m, v, activated);
    }
    scene_arrays_written(ctx, activated->pos, activated->scale, activated->rotq); // (a context-owned scene trained in place)
    BackwardRequest req;
    req.d_dL_dimg = d_dL_dimg, req.dest = BackwardRequest::FusedAdam;
    req.raw = adam_arrays(raw), req.m = adam_arrays(m), req.v = adam_arrays(v), req.act = adam_arrays(activated);
    req.lr = adam_rates(cfg), req.step = make_adam_step(cfg->beta1, cfg->beta2, cfg->eps, cfg->step);
    return render_backward(ctx, req);
}

lcgs_status lcgs_render_maps(lcgs_context* ctx, int mode, float* d_depth, float* d_alpha)
{
    LCGS_REQUIRE(ctx, "NULL argument");
    LCGS_REQUIRE(mode == LCGS_DEPTH_Z || mode == LCGS_DEPTH_INV_Z, "mode must be LCGS_DEPTH_Z or LCGS_DEPTH_INV_Z");
    LCGS_REQUIRE(d_depth || d_alpha, "both outputs are NULL");
    LCGS_ENTRY(ctx);
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    LCGS_TRY(check_own_kept_frame(ctx, "lcgs_render_maps"));
    launch_render_maps(kept_frame(ctx), mode, d_depth, d_alpha, ctx->stream);
    LCGS_HIP_CHECK(hipGetLastError());
    return LCGS_OK;
}

lcgs_status lcgs_render_distortion(lcgs_context* ctx, int mode, float center, float* d_dist)
{
    LCGS_REQUIRE(ctx && d_dist, "NULL argument");
    LCGS_REQUIRE(mode == LCGS_DEPTH_Z || mode == LCGS_DEPTH_INV_Z, "mode must be LCGS_DEPTH_Z or LCGS_DEPTH_INV_Z");
    LCGS_REQUIRE(isfinite(center), "center must be finite");
    LCGS_ENTRY(ctx);
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    LCGS_TRY(check_own_kept_frame(ctx, "lcgs_render_distortion"));
    launch_render_distortion(kept_frame(ctx), mode, center, d_dist, ctx->stream);
    LCGS_HIP_CHECK(hipGetLastError());
    return LCGS_OK;
}

lcgs_status lcgs_contrib_accumulate(lcgs_context* ctx, int num_gaussians, const lcgs_contrib_stats* stats)
{
    LCGS_REQUIRE(ctx && stats, "NULL argument");
    LCGS_REQUIRE(stats->weight_sum || stats->weight_max || stats->pixels || stats->views, "all four statistics are NULL");
    LCGS_ENTRY(ctx);
    LCGS_REQUIRE(num_gaussians == ctx->P, "num_gaussians must be the bound scene's");
    LCGS_TRY(check_own_kept_frame(ctx, "lcgs_contrib_accumulate"));
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    // one slot per on-screen row; sized for the scene's rows like the frame's other per-row buffers (the count stays on the device)
    LCGS_TRY(ctx->contrib_slab.ensure(contrib_slab_bytes((int64_t)ctx->P)));
    hipStream_t    st   = ctx->stream;
    const KeptRows rows = kept_rows(ctx);
    uint32_t*      slab = ctx->contrib_slab.as<uint32_t>();
    ctx->n_marks        = 0;
    LCGS_TRY(mark(ctx, "begin"));
    launch_contrib_zero(rows, slab, st);
    launch_contrib_walk(kept_frame(ctx), slab, st);
    LCGS_TRY(mark(ctx, "contrib_walk"));
    launch_contrib_fold(rows, slab, stats->weight_sum, stats->weight_max, stats->pixels, stats->views, st);
    LCGS_TRY(mark(ctx, "contrib_fold"));
    LCGS_HIP_CHECK(hipGetLastError());
    if (ctx->profiling) {
        LCGS_HIP_CHECK(hipStreamSynchronize(st));
        LCGS_TRY(collect_marks(ctx));
    }
    return LCGS_OK;
}

lcgs_status lcgs_render_backward_maps(lcgs_context* ctx, const float* d_dL_dimg, int mode, const float* d_dL_ddepth,
                                      const float* d_dL_dalpha, int accumulate, const lcgs_grads* grads)
{
    LCGS_REQUIRE(ctx && grads, "NULL argument");
    LCGS_REQUIRE(mode == LCGS_DEPTH_Z || mode == LCGS_DEPTH_INV_Z, "mode must be LCGS_DEPTH_Z or LCGS_DEPTH_INV_Z");
    LCGS_REQUIRE(d_dL_dimg || d_dL_ddepth || d_dL_dalpha, "all three incoming gradients are NULL");
    LCGS_REQUIRE(grads->d_dL_dpos && grads->d_dL_dscale && grads->d_dL_drotq && grads->d_dL_dsh && grads->d_dL_dopacity,
                 "NULL gradient buffer");
    BackwardRequest req = rows_request(d_dL_dimg, grads, accumulate ? BackwardRequest::DenseAccumulate : BackwardRequest::Dense);
    req.mode = mode, req.d_dL_ddepth = d_dL_ddepth, req.d_dL_dalpha = d_dL_dalpha;
    LCGS_ENTRY(ctx);
    return render_backward(ctx, req);
}

lcgs_status lcgs_render_backward_distortion(lcgs_context* ctx, const float* d_dL_dimg, int mode, float center,
                                            const float* d_dL_ddepth, const float* d_dL_dalpha, const float* d_dL_ddist,
                                            int accumulate, const lcgs_grads* grads)
{
    LCGS_REQUIRE(ctx && grads, "NULL argument");
    LCGS_REQUIRE(mode == LCGS_DEPTH_Z || mode == LCGS_DEPTH_INV_Z, "mode must be LCGS_DEPTH_Z or LCGS_DEPTH_INV_Z");
    LCGS_REQUIRE(isfinite(center), "center must be finite");
    LCGS_REQUIRE(d_dL_dimg || d_dL_ddepth || d_dL_dalpha || d_dL_ddist, "all four incoming gradients are NULL");
    LCGS_REQUIRE(grads->d_dL_dpos && grads->d_dL_dscale && grads->d_dL_drotq && grads->d_dL_dsh && grads->d_dL_dopacity,
                 "NULL gradient buffer");
    BackwardRequest req = rows_request(d_dL_dimg, grads, accumulate ? BackwardRequest::DenseAccumulate : BackwardRequest::Dense);
    req.mode = mode, req.center = center;
    req.d_dL_ddepth = d_dL_ddepth, req.d_dL_dalpha = d_dL_dalpha, req.d_dL_ddist = d_dL_ddist;
    LCGS_ENTRY(ctx);
    return render_backward(ctx, req);
}

lcgs_status lcgs_render_normals(lcgs_context* ctx, float* d_normal)
{
    LCGS_REQUIRE(ctx && d_normal, "NULL argument");
    LCGS_ENTRY(ctx);
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    LCGS_TRY(check_own_kept_frame(ctx, "lcgs_render_normals"));
    LCGS_TRY(ctx->splat_normals.ensure(splat_normals_bytes((int64_t)ctx->P)));
    ctx->n_marks = 0;
    LCGS_TRY(mark(ctx, "begin"));
    launch_splat_normals(kept_rows(ctx), ctx->splat_normals.as<float4>(), nullptr, ctx->stream);
    LCGS_TRY(mark(ctx, "splat_normals"));
    launch_render_normals(kept_frame(ctx), ctx->splat_normals.as<float4>(), d_normal, ctx->stream);
    LCGS_TRY(mark(ctx, "render_normals"));
    LCGS_HIP_CHECK(hipGetLastError());
    if (ctx->profiling) {
        LCGS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        LCGS_TRY(collect_marks(ctx));
    }
    return LCGS_OK;
}

lcgs_status lcgs_render_backward_normals(lcgs_context* ctx, const float* d_dL_dimg, int mode, float center,
                                         const float* d_dL_ddepth, const float* d_dL_dalpha, const float* d_dL_ddist,
                                         const float* d_dL_dnormal, int accumulate, const lcgs_grads* grads)
{
    LCGS_REQUIRE(ctx && grads, "NULL argument");
    LCGS_REQUIRE(mode == LCGS_DEPTH_Z || mode == LCGS_DEPTH_INV_Z, "mode must be LCGS_DEPTH_Z or LCGS_DEPTH_INV_Z");
    LCGS_REQUIRE(isfinite(center), "center must be finite");
    LCGS_REQUIRE(d_dL_dimg || d_dL_ddepth || d_dL_dalpha || d_dL_ddist || d_dL_dnormal, "all five incoming gradients are NULL");
    LCGS_REQUIRE(grads->d_dL_dpos && grads->d_dL_dscale && grads->d_dL_drotq && grads->d_dL_dsh && grads->d_dL_dopacity,
                 "NULL gradient buffer");
    BackwardRequest req = rows_request(d_dL_dimg, grads, accumulate ? BackwardRequest::DenseAccumulate : BackwardRequest::Dense);
    req.mode = mode, req.center = center;
    req.d_dL_ddepth = d_dL_ddepth, req.d_dL_dalpha = d_dL_dalpha, req.d_dL_ddist = d_dL_ddist, req.d_dL_dnormal = d_dL_dnormal;
    LCGS_ENTRY(ctx);
    return render_backward(ctx, req);
}

lcgs_status lcgs_render_features(lcgs_context* ctx, int num_gaussians, int channels, const float* d_features, float* d_feature_map)
{
    LCGS_REQUIRE(ctx && d_features && d_feature_map, "NULL argument");
    LCGS_REQUIRE(channels >= 1 && channels <= LCGS_FEATURES_MAX, "channels must be 1 .. LCGS_FEATURES_MAX");
    LCGS_ENTRY(ctx);
    LCGS_REQUIRE(num_gaussians == ctx->P, "num_gaussians must be the bound scene's");
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    LCGS_TRY(check_own_kept_frame(ctx, "lcgs_render_features"));
    const FeatureChannel fc{ channels, ctx->vis_index.as<uint32_t>(), d_features, nullptr, nullptr };
    ctx->n_marks = 0;
    LCGS_TRY(mark(ctx, "begin"));
    launch_render_features(kept_frame(ctx), fc, d_feature_map, features_chunk_width(channels, ctx->features_ch_forced), ctx->stream);
    LCGS_TRY(mark(ctx, "render_features"));
    LCGS_HIP_CHECK(hipGetLastError());
    if (ctx->profiling) {
        LCGS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        LCGS_TRY(collect_marks(ctx));
    }
    return LCGS_OK;
}

lcgs_status lcgs_render_backward_features(lcgs_context* ctx, const float* d_dL_dimg, int mode, float center,
                                          const float* d_dL_ddepth, const float* d_dL_dalpha, const float* d_dL_ddist,
                                          const float* d_dL_dnormal, const lcgs_feature_channel* feat, int accumulate,
                                          const lcgs_grads* grads)
{
    LCGS_REQUIRE(ctx && (grads || feat), "NULL argument");
    LCGS_REQUIRE(mode == LCGS_DEPTH_Z || mode == LCGS_DEPTH_INV_Z, "mode must be LCGS_DEPTH_Z or LCGS_DEPTH_INV_Z");
    LCGS_REQUIRE(isfinite(center), "center must be finite");
    const bool others = d_dL_dimg || d_dL_ddepth || d_dL_dalpha || d_dL_ddist || d_dL_dnormal;
    LCGS_REQUIRE(others || feat, "all five incoming gradients are NULL and there is no feature channel");
    if (feat) {
        LCGS_REQUIRE(feat->channels >= 1 && feat->channels <= LCGS_FEATURES_MAX, "channels must be 1 .. LCGS_FEATURES_MAX");
        LCGS_REQUIRE(feat->d_features && feat->d_dL_dfeature_map, "NULL feature rows or NULL feature-map gradient");
        LCGS_REQUIRE(grads || feat->d_dL_dfeatures, "grads and d_dL_dfeatures are both NULL: nothing to write");
        LCGS_REQUIRE(grads || !others, "grads may be NULL only when every other incoming gradient is NULL (frozen geometry)");
    }
    LCGS_REQUIRE(!grads || (grads->d_dL_dpos && grads->d_dL_dscale && grads->d_dL_drotq && grads->d_dL_dsh && grads->d_dL_dopacity),
                 "NULL gradient buffer");
    LCGS_ENTRY(ctx);
    if (!grads) return features_only_backward(ctx, *feat, accumulate != 0);
    BackwardRequest req = rows_request(d_dL_dimg, grads, accumulate ? BackwardRequest::DenseAccumulate : BackwardRequest::Dense);
    req.mode = mode, req.center = center, req.feat = feat;
    req.d_dL_ddepth = d_dL_ddepth, req.d_dL_dalpha = d_dL_dalpha, req.d_dL_ddist = d_dL_ddist, req.d_dL_dnormal = d_dL_dnormal;
    return render_backward(ctx, req);
}

lcgs_status lcgs_camera_backward(lcgs_context* ctx, float* d_dL_dcam)
{
    LCGS_REQUIRE(ctx && d_dL_dcam, "NULL argument");
    LCGS_ENTRY(ctx);
    LCGS_TRY(check_own_kept_frame(ctx, "lcgs_camera_backward"));
    if (!ctx->g2d_backward_done) {
        set_last_error("lcgs_camera_backward needs a backward of the last frame (its 2-D gradient rows are only zeros until then)");
        return LCGS_ERR_STATE;
    }
    if (ctx->g2d_normal_channel) { // the view-space normal depends on the camera's rotation directly: that term is not built
        set_last_error("lcgs_camera_backward: the last backward passed a normal gradient (lcgs_render_backward_normals); the camera "
                       "gradient of the normal channel is not offered");
        return LCGS_ERR_STATE;
    }
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    LCGS_TRY(camera_pass(ctx, d_dL_dcam));
    LCGS_HIP_CHECK(hipGetLastError());
    return LCGS_OK;
}

lcgs_status lcgs_render_backward_camera(lcgs_context* ctx, const float* d_dL_dimg, int mode, const float* d_dL_ddepth,
                                        const float* d_dL_dalpha, float* d_dL_dcam)
{
    LCGS_REQUIRE(ctx && d_dL_dcam, "NULL argument");
    LCGS_REQUIRE(mode == LCGS_DEPTH_Z || mode == LCGS_DEPTH_INV_Z, "mode must be LCGS_DEPTH_Z or LCGS_DEPTH_INV_Z");
    LCGS_REQUIRE(d_dL_dimg || d_dL_ddepth || d_dL_dalpha, "all three incoming gradients are NULL");
    BackwardRequest req;
    req.d_dL_dimg = d_dL_dimg, req.mode = mode, req.d_dL_ddepth = d_dL_ddepth, req.d_dL_dalpha = d_dL_dalpha;
    req.dest = BackwardRequest::CameraOnly, req.d_dL_dcam = d_dL_dcam;
    LCGS_ENTRY(ctx);
    return render_backward(ctx, req);
}

lcgs_status lcgs_camera_grad_to_twist(const lcgs_camera* cam, const float dL_dcam[12], float dL_dxi[6])
{
    LCGS_REQUIRE(cam && dL_dcam && dL_dxi, "NULL argument");
    const float* axes[3] = { cam->right, cam->up, cam->front }; // columns of Rc
    const float* g[3]    = { dL_dcam + 9, dL_dcam + 6, dL_dcam + 3 }; // g_right, g_up, g_front
    double       m[3][3]; // m[k] = Rc^T g_k
    for (int k = 0; k < 3; ++k)
        for (int r = 0; r < 3; ++r)
            m[k][r] = (double)axes[r][0] * g[k][0] + (double)axes[r][1] * g[k][1] + (double)axes[r][2] * g[k][2];
    // sum_k e_k x m[k]:  e_0 x a = (0, -a2, a1), e_1 x a = (a2, 0, -a0), e_2 x a = (-a1, a0, 0)
    dL_dxi[0] = (float)(m[1][2] - m[2][1]);
    dL_dxi[1] = (float)(m[2][0] - m[0][2]);
    dL_dxi[2] = (float)(m[0][1] - m[1][0]);
    for (int r = 0; r < 3; ++r)
        dL_dxi[3 + r] = (float)((double)axes[r][0] * dL_dcam[0] + (double)axes[r][1] * dL_dcam[1] + (double)axes[r][2] * dL_dcam[2]);
    return LCGS_OK;
}

lcgs_status lcgs_visible_rows(lcgs_context* ctx, const uint32_t** d_rows, const uint32_t** d_count)
{
    LCGS_REQUIRE(ctx && d_rows && d_count, "NULL argument");
    LCGS_ENTRY(ctx);
    LCGS_REQUIRE(ctx->frame_state_valid(), "no frame rendered yet");
    *d_rows  = ctx->vis_index.as<uint32_t>();
    *d_count = ctx->counts.as<uint32_t>(); // [0] = on-screen splats of the last frame
    return LCGS_OK;
}

} // extern "C"

namespace
{
lcgs_status render_backward(lcgs_context* ctx, const BackwardRequest& req)
{
    using Dest = BackwardRequest::Dest;
    const float* const      d_dL_dimg = req.d_dL_dimg;
    const lcgs_grads* const grads     = req.grads; // (non-NULL behind the first check when the request has rows)
    const bool maps = req.maps(), rows_out = req.rows(); // (rows_out: gradient arrays are written; else the optimiser's or the camera's)
    const bool camera_only = req.dest == Dest::CameraOnly; // (lcgs_render_backward_camera: the walks and the camera pass, no per-splat pass)
    const bool accumulate = req.dest == Dest::DenseAccumulate, compact = !accumulate && req.dest != Dest::Dense;
    const lcgs_feature_channel* const feat = req.feat;
    LCGS_REQUIRE(ctx && (d_dL_dimg || maps || feat) && (grads || !rows_out), "NULL argument");
    LCGS_HIP_CHECK(hipSetDevice(ctx->device)); // multi-GPU processes: every entry point selects its device
    LCGS_REQUIRE(!rows_out || (grads->d_dL_dpos && grads->d_dL_dscale && grads->d_dL_drotq && grads->d_dL_dsh &&
                               grads->d_dL_dopacity),
                 "NULL gradient buffer");
    LCGS_TRY(check_own_kept_frame(ctx, "lcgs_render_backward",
                              "the last frame was drawn from received records (lcgs_owner_render): use lcgs_owner_render_backward"));
    LCGS_REQUIRE(!rows_out || (reinterpret_cast<uintptr_t>(grads->d_dL_drotq) & 15) == 0, "dL_drotq must be 16-byte aligned");
    if (camera_only) LCGS_TRY(ctx->cam_slab.ensure(camera_grad_slab_bytes((int64_t)ctx->P))); // (before any device work)
    const bool normals = req.d_dL_dnormal != nullptr;
    LCGS_REQUIRE(!normals || (rows_out && !compact), "the normal channel writes dense rows only");
    LCGS_REQUIRE(!feat || (rows_out && !compact), "the feature channel writes dense rows only");
    if (normals) {
        LCGS_TRY(ctx->splat_normals.ensure(splat_normals_bytes((int64_t)ctx->P)));
        LCGS_TRY(ctx->splat_normal_grads.ensure(splat_normals_bytes((int64_t)ctx->P)));
    }
    hipStream_t  st   = ctx->stream;
    const size_t P    = (size_t)ctx->P;
    ctx->n_marks      = 0;
    LCGS_TRY(mark(ctx, "begin"));
    // dense per-splat gradients: splats that did not reach the screen get exact zeros.  The 236 B/splat zero-fill
    // is pure HBM writes and independent of the render-backward: it runs on the auxiliary stream beside it.
    // (Compact rows: every row that exists is written by the preprocess-backward, nothing to clear.)
    // accumulate: the arrays hold the sum of earlier views of the batch -- no fill, the rows are added to
    // Round 4: the fill is a SIDE JOB of the render-backward kernel (backward.hip, DenseFill) -- its workgroups clear their
    // share of the five arrays with fire-and-forget stores before they turn to their tile -- instead of 0.33 ms of memset
    // kernels on the auxiliary stream, a fork and a join: 1.741 -> 1.724 ms per step (most of what the fill costs the
    // VALU-bound kernel is the memory system's either way).
    // (Per-stage profiling keeps the memsets, in order, as "zero_grads"; so do arrays too long for the kernel's 32-bit lengths.)
    const bool  dense_fill = !compact && !accumulate;
    DenseFill   fill;
    // (a maps backward without an image gradient launches no render-backward: the memsets clear the rows)
    const bool  fill_in_kernel = dense_fill && d_dL_dimg && !ctx->profiling && dense_fill_rows(*grads, ctx->sh_deg, P, &fill); // (u32 lengths)
    const bool  overlap = !ctx->profiling && dense_fill && !fill_in_kernel;
    hipStream_t zs      = overlap ? ctx->aux_stream : st;
    if (overlap) {
        LCGS_HIP_CHECK(hipEventRecord(ctx->ev_fork, st));
        LCGS_HIP_CHECK(hipStreamWaitEvent(ctx->aux_stream, ctx->ev_fork, 0));
    }
    // dense rows with a communicator attached: the preprocess pass runs as splat-range slices so that the gradient
    // all-reduce (lcgs_grads_allreduce) can start on the first rows while the later ones are still being computed
    // (the maps backward adds to dL_dpos behind the preprocess pass: unsliced, so that no all-reduce starts on rows it has yet to finish)
    const bool sliced = !compact && !maps && !feat && ctx->grad_slices > 1 && P >= 4096;
    if (sliced) {
        LCGS_TRY(ctx->slice_bounds.ensure((lcgs::kMaxGradSlices + 1) * sizeof(uint32_t)));
        for (int k = 0; k < ctx->grad_slices; ++k)
            LCGS_TRY(ctx->ev_slice[k].ensure());
        launch_slice_bounds(kept_rows(ctx), ctx->grad_slices, ctx->slice_bounds.as<uint32_t>(), zs); // (before the fill: ev_join / stream order covers it)
    }
    if (dense_fill && !fill_in_kernel) LCGS_TRY(zero_grad_rows(*grads, ctx->sh_deg, P, zs));
    if (overlap) LCGS_HIP_CHECK(hipEventRecord(ctx->ev_join, ctx->aux_stream));
    if (ctx->g2d_zeroed && !ctx->profiling) { // cleared by the forward's renderer (first backward of this frame only)
        ctx->g2d_zeroed = false;
    } else {
        LCGS_TRY(ctx->grads2d.ensure(grads2d_bytes((int64_t)P)));
        launch_zero_grads2d(ctx->counts.as<uint32_t>(), ctx->grads2d.as<float>(), st, ctx->bwd_counter.as<uint32_t>());
        ctx->g2d_zeroed = false;
    }
    LCGS_TRY(mark(ctx, "zero_grads"));
    // another view's forward in flight (lcgs_fit_views): a bounded persistent grid leaves its sort chain room on every CU
    const int      k_bwd = ctx->persist_bwd_forced >= 0 ? ctx->persist_bwd_forced
                                                        : (ctx->frames_in_flight ? ctx->persist_bwd_in_flight : 0);
    const uint32_t bwd_wgs = (!ctx->profiling && k_bwd > 0) ? (uint32_t)(k_bwd * std::max(ctx->num_cus, 1)) : 0u;
    const KeptFrame kept   = kept_frame(ctx);
    const KeptRows  rows   = kept_rows(ctx); // (behind the 2-D rows' ensure above)
    if (d_dL_dimg) {
        launch_render_backward(kept, ctx->last.bg, d_dL_dimg, ctx->grads2d.as<float>(), st, ctx->bwd_counter.as<uint32_t>(), bwd_wgs,
                               fill_in_kernel ? &fill : nullptr);
        LCGS_TRY(mark(ctx, "render_backward"));
    }
    NormalChannel nrm{ req.d_dL_dnormal, ctx->splat_normals.as<float4>(), ctx->splat_normal_grads.as<float>() };
    if (normals) { // the rows' normals, as the forward's own pass forms them, and their cleared dL/dn slots
        launch_splat_normals(rows, ctx->splat_normals.as<float4>(), ctx->splat_normal_grads.as<float4>(), st);
        LCGS_TRY(mark(ctx, "splat_normals"));
    }
    if (maps) { // the map channels add to the rows the colour walk (or the zeroing alone) left: one walk for all of them
        launch_render_maps_backward(kept, req.mode, req.d_dL_ddepth, req.d_dL_dalpha, ctx->grads2d.as<float>(), st, req.center,
                                    req.d_dL_ddist, normals ? &nrm : nullptr);
        LCGS_TRY(mark(ctx, "render_maps_backward"));
    }
    if (feat) { // the caller's channels: one walk per chunk of them, adding to the same 2-D rows; their own sums go to the caller
        if (feat->d_dL_dfeatures && !accumulate) { // rows nothing blends: exact zeros (P K floats: a stage of its own under profiling)
            LCGS_HIP_CHECK(hipMemsetAsync(feat->d_dL_dfeatures, 0, P * (size_t)feat->channels * sizeof(float), st));
            LCGS_TRY(mark(ctx, "zero_features"));
        }
        const FeatureChannel fc{ feat->channels, rows.vis_index, feat->d_features, feat->d_dL_dfeature_map, feat->d_dL_dfeatures };
        launch_render_features_backward(kept, fc, ctx->grads2d.as<float>(), features_chunk_width(feat->channels, ctx->features_ch_forced), st);
        LCGS_TRY(mark(ctx, "render_features_backward"));
    }
    if (overlap) LCGS_HIP_CHECK(hipStreamWaitEvent(st, ctx->ev_join, 0));
    const int slices = rows_out ? (sliced ? ctx->grad_slices : 1) : 0;
    if (req.dest == Dest::FusedAdam) // (compact, unsliced: the update is applied where the gradients are formed; nothing is written out)
        launch_preprocess_backward_adam(rows, req.raw, req.m, req.v, req.act, req.lr, req.step, st);
    for (int k = 0; k < slices; ++k) {
        launch_preprocess_backward(rows, grads->d_dL_dpos, grads->d_dL_dscale, grads->d_dL_drotq, grads->d_dL_dsh,
                                   grads->d_dL_dopacity,
                                   RowsOut{ compact, accumulate, sliced ? ctx->slice_bounds.as<uint32_t>() : nullptr, k, slices }, st);
        if (sliced) LCGS_HIP_CHECK(hipEventRecord(ctx->ev_slice[k], st));
    }
    if (rows_out && req.value_channel()) // view z = front . pos + tz: the depth and distortion channels' dL/dvalue reaches the position rows directly
        launch_maps_depth_to_pos(rows, req.mode, grads->d_dL_dpos, st);
    ctx->slices_recorded = sliced ? slices : 0;
    ctx->slices_of       = sliced ? grads->d_dL_dpos : nullptr;
    // sparse exchange (opt-in, lcgs_comm_track_touched_rows): the rows this frame wrote join the step's touched set
    if (rows_out && !compact && ctx->comm)
        LCGS_TRY(lcgs::comm_mark_touched(ctx->comm, rows, accumulate, st));
    ctx->g2d_backward_done = true; // the frame's 2-D gradient rows now hold a backward's sums (lcgs_densify_accumulate)
    ctx->g2d_value_mode    = req.value_channel() ? req.mode : -1; // (every backward starts from zeroed rows)
    ctx->g2d_normal_channel = normals;
    if (camera_only) LCGS_TRY(camera_pass(ctx, req.d_dL_dcam));
    LCGS_TRY(mark(ctx, "preprocess_backward"));
    if (normals) { // dL/dn reaches the rotation rows through the closed form of the axis' column
        launch_normals_to_rot(rows, ctx->splat_normals.as<float4>(), ctx->splat_normal_grads.as<float4>(), grads->d_dL_drotq, st);
        LCGS_TRY(mark(ctx, "normals_to_rot"));
    }
    LCGS_HIP_CHECK(hipGetLastError());
    if (ctx->profiling) {
        LCGS_HIP_CHECK(hipStreamSynchronize(st));
        LCGS_TRY(collect_marks(ctx));
    }
    return LCGS_OK;
}

// lcgs_render_backward_features without gradient arrays: the geometry is frozen, dL/dfeatures alone.  A short path of its own:
// the walk forms no geometry sums, and the frame's 2-D gradient rows and the flags behind them are left as they were
lcgs_status features_only_backward(lcgs_context* ctx, const lcgs_feature_channel& feat, bool accumulate)
{
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    LCGS_TRY(check_own_kept_frame(ctx, "lcgs_render_backward_features"));
    hipStream_t st = ctx->stream;
    ctx->n_marks   = 0;
    LCGS_TRY(mark(ctx, "begin"));
    if (!accumulate) {
        LCGS_HIP_CHECK(hipMemsetAsync(feat.d_dL_dfeatures, 0, (size_t)ctx->P * (size_t)feat.channels * sizeof(float), st));
        LCGS_TRY(mark(ctx, "zero_features"));
    }
    const FeatureChannel fc{ feat.channels, ctx->vis_index.as<uint32_t>(), feat.d_features, feat.d_dL_dfeature_map, feat.d_dL_dfeatures };
    launch_render_features_backward(kept_frame(ctx), fc, nullptr, features_chunk_width(feat.channels, ctx->features_ch_forced), st);
    LCGS_TRY(mark(ctx, "render_features_backward"));
    LCGS_HIP_CHECK(hipGetLastError());
    if (ctx->profiling) {
        LCGS_HIP_CHECK(hipStreamSynchronize(st));
        LCGS_TRY(collect_marks(ctx));
    }
    return LCGS_OK;
}
} // namespace
