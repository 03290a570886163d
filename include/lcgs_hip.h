/*
 * lcgs_hip.h -- C ABI of liblcgs_hip.so: the MI355X-native (gfx950) implementation of the LuisaComputeGaussianSplatting hot
 * path (SH colour -> 3D->2D projection -> tile keys -> sort -> per-tile alpha compositing) plus the matching backward.
 * Every entry point names the reference interface it replaces (paths relative to the reference repository).
 *
 * Contract, for every function unless it says otherwise:
 *   - `d_` pointers are DEVICE pointers owned by the caller, laid out as the reference's flat float buffers
 *     (lcgs/include/lcgs/proxy.h:21-73: pos xyz.., rotq rxyz.., SH [P][16][3]); `h_` pointers are host memory;
 *   - structs are POD, passed by pointer, copied before the call returns;
 *   - the return value is an lcgs_status (no exception crosses the boundary); lcgs_last_error() has the message;
 *   - work is ENQUEUED on the context's stream; "synchronises" is said where a call waits for the device;
 *   - one lcgs_context per (GPU, stream), used by one host thread at a time (like the reference's operator objects,
 *     gs_tile_splatter.h:23,50-55); different contexts may be driven from different threads.
 * Long-form notes (why, measured effects, history) per declaration: docs/API_NOTES.md.
 */
#ifndef LCGS_HIP_H
#define LCGS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(_WIN32)
#define LCGS_API __declspec(dllexport)
#else
#define LCGS_API __attribute__((visibility("default")))
#endif

typedef enum lcgs_status {
    LCGS_OK                = 0,
    LCGS_ERR_INVALID_ARG   = 1,
    LCGS_ERR_HIP           = 2, /* a HIP / RCCL call failed; see lcgs_last_error() */
    LCGS_ERR_NO_DEVICE     = 3, /* no gfx950 device (there is no CPU fallback), or RCCL absent for lcgs_comm_* */
    LCGS_ERR_OUT_OF_MEMORY = 4,
    LCGS_ERR_CAPACITY      = 5, /* pair buffers too small (the reference does not check, app/main.cpp:245) */
    LCGS_ERR_IO            = 6,
    LCGS_ERR_FORMAT        = 7,
    LCGS_ERR_STATE         = 8  /* e.g. backward without a preceding keep_state forward */
} lcgs_status;

typedef struct lcgs_context lcgs_context;

/* struct Camera, lcgs/include/lcgs/util/camera.h:15-25 */
typedef struct lcgs_camera {
    float position[3], front[3], up[3], right[3];
    float fov;          /* vertical, degrees (default 60) */
    float aspect_ratio; /* width / height */
    int   width, height;
} lcgs_camera;

/* ---- library / context ------------------------------------------------------------------------------------------ */
LCGS_API const char* lcgs_version(void);
LCGS_API const char* lcgs_last_error(void); /* thread-local message of the last failing call */
/* Context::create_device + Device::create_stream (app/main.cpp:162-163) and the three create(Device&) calls.
 * stream: a hipStream_t (NULL = the null stream).  Kernels are precompiled for gfx950. */
LCGS_API lcgs_status lcgs_create(int device_id, void* stream, lcgs_context** out_ctx);
LCGS_API lcgs_status lcgs_destroy(lcgs_context* ctx);
LCGS_API lcgs_status lcgs_set_stream(lcgs_context* ctx, void* stream);
LCGS_API lcgs_status lcgs_synchronize(lcgs_context* ctx); /* Stream::synchronize (app/main.cpp:223,315) */

/* ---- host camera helpers: get_lookat_cam, local_to_world, world_to_local, projection matrix (util/camera.h:74-82,
 * 27-36, 38-51, 54-72); matrices column-major float[16], m[c*4+r] ------------------------------------------------ */
LCGS_API void lcgs_get_lookat_cam(const float pos[3], const float target[3], const float world_up[3], lcgs_camera* out_cam);
LCGS_API void lcgs_local_to_world_matrix(const lcgs_camera* cam, float m[16]);
LCGS_API void lcgs_world_to_local_matrix(const lcgs_camera* cam, float m[16]);
LCGS_API void lcgs_projection_matrix(float tanfovx, float tanfovy, float znear, float zfar, float m[16]);

/* ---- stage-level operators: one call per reference class method, the reference's buffers bit for bit ----------- */
/* SHProcessor::process (sh_preprocessor.h:30-37, sh_preprocessor.cpp:169-188): d_color[3P] = clamp(SH(dir) + 0.5, 0, 1) */
LCGS_API lcgs_status lcgs_sh_process(lcgs_context* ctx, int num_points, const float* d_pos, const lcgs_camera* camera,
                                     const float* d_sh, float* d_color, int level, int channel);
/* GSProjector::forward (gs_projector.h:37-43, gs_projector/impl.cpp:26-93): means_2d[2P] NDC, covs_2d[3P], depth[P];
 * splats with view z < 0.2 are left unwritten (gs_projector/shader.cpp:121). */
LCGS_API lcgs_status lcgs_project_forward(lcgs_context* ctx, int num_gaussians, const float* d_pos, const float* d_scale,
                                          const float* d_rotq, float scale_modifier, float* d_means_2d, float* d_covs_2d,
                                          float* d_depth, const lcgs_camera* camera, int use_focal);
/* GSTileSplatterAccelProxy (proxy.h:56-64) + the pair capacity the app fixes at 20 M (app/main.cpp:245) */
typedef struct lcgs_tile_accel {
    uint32_t* tiles_touched;            /* P */
    uint32_t* point_offsets;            /* P */
    uint64_t* point_list_keys_unsorted; /* capacity */
    uint32_t* point_list_unsorted;      /* capacity */
    uint64_t* point_list_keys;          /* capacity */
    uint32_t* point_list;               /* capacity */
    uint32_t* ranges;                   /* 2 * ceil(W/16) * ceil(H/16) */
    int64_t   capacity;                 /* (tile, splat) pairs the four pair buffers hold */
} lcgs_tile_accel;
/* GSTileSplatterInputProxy (proxy.h:43-54); means_2d / conic are overwritten in place (NDC -> pixel, cov -> conic) */
typedef struct lcgs_tile_input {
    int          num_gaussians;
    float        bg_color[3];
    float*       means_2d;         /* 2P */
    const float* depth_features;   /* P  */
    float*       conic;            /* 3P */
    const float* color_features;   /* 3P */
    const float* opacity_features; /* P  */
} lcgs_tile_input;
/* GSSplatForwardOutputProxy (proxy.h:66-71); target_img planar CHW; final_T / n_contrib optional (NULL to skip) */
typedef struct lcgs_tile_output {
    int       height, width;
    float*    target_img; /* 3*H*W */
    int32_t*  radii;      /* P */
    float*    final_T;    /* H*W */
    uint32_t* n_contrib;  /* H*W */
} lcgs_tile_output;
/* GSTileSplatter::forward (gs_tile_splatter.h:28-35, impl.cpp:63-180).  *num_rendered = the reference's return value
 * (0: nothing drawn, image untouched, impl.cpp:109).  Synchronises once, like impl.cpp:106-107. */
LCGS_API lcgs_status lcgs_tile_splat_forward(lcgs_context* ctx, const lcgs_tile_accel* accel, const lcgs_tile_input* input,
                                             const lcgs_tile_output* output, int use_focal, int* num_rendered);
/* LCGS_STAGES_EXACT (default): each call runs at once.  LCGS_STAGES_DEFERRED: lcgs_sh_process / lcgs_project_forward only
 * record; a splat call on exactly their outputs renders the fused frame into target_img / radii (same bits, intermediates
 * not written); anything else (a non-matching call, lcgs_stage_flush, lcgs_synchronize, a mode switch) runs what was recorded. */
typedef enum lcgs_stage_mode { LCGS_STAGES_EXACT = 0, LCGS_STAGES_DEFERRED = 1 } lcgs_stage_mode;
LCGS_API lcgs_status lcgs_set_stage_mode(lcgs_context* ctx, int mode);
LCGS_API lcgs_status lcgs_stage_flush(lcgs_context* ctx);
/* lcpp DeviceScan::InclusiveSum (call site impl.cpp:104) and DeviceRadixSort::SortPairs<ulong,uint> (impl.cpp:135-143):
 * u32 wrap-around sum; stable ascending sort on bits [begin_bit, end_bit).  Temp storage is the context's. */
LCGS_API lcgs_status lcgs_inclusive_sum_u32(lcgs_context* ctx, const uint32_t* d_in, uint32_t* d_out, int64_t n);
LCGS_API lcgs_status lcgs_sort_pairs_u64_u32(lcgs_context* ctx, const uint64_t* d_keys_in, uint64_t* d_keys_out,
                                             const uint32_t* d_vals_in, uint32_t* d_vals_out, int64_t n, int begin_bit, int end_bit);

/* ---- the scene a context renders ------------------------------------------------------------------------------- */
/* Caller-owned activated arrays (the five buffers of app/main.cpp:180-186 after :216-223); rotq 16-byte aligned. */
LCGS_API lcgs_status lcgs_scene_bind(lcgs_context* ctx, int num_gaussians, int sh_degree, const float* d_pos, const float* d_scale,
                                     const float* d_rotq, const float* d_sh, const float* d_opacity);
/* Host arrays -> device copies OWNED by the context.  Synchronises. */
LCGS_API lcgs_status lcgs_scene_upload(lcgs_context* ctx, int num_gaussians, int sh_degree, const float* h_pos, const float* h_scale,
                                       const float* h_rotq, const float* h_sh, const float* h_opacity);
/* read_gs_ply (app/gaussians.cpp:75-171) + upload, de-interleave and activations on the device (exp within 2 ulp of the
 * host reader's; ascii / non-float files take the host path).  Context-owned.  Synchronises. */
LCGS_API lcgs_status lcgs_scene_load_ply(lcgs_context* ctx, const char* path, int* num_gaussians);
/* Order of a context-owned scene: LCGS_ORDER_SPATIAL (default; upload / load_ply finish with lcgs_scene_reorder_spatial,
 * per-splat outputs follow the new order) or LCGS_ORDER_FILE.  Bound arrays always keep the caller's order. */
typedef enum lcgs_splat_order { LCGS_ORDER_FILE = 0, LCGS_ORDER_SPATIAL = 1 } lcgs_splat_order;
LCGS_API lcgs_status lcgs_set_ingest_order(lcgs_context* ctx, int order);
/* Morton re-order of the context's scene (a bound scene is copied first).  d_perm[P] (device, nullable): new row r = old
 * row d_perm[r].  Same images bit for bit (equal depths still blend in file order).  Synchronises. */
LCGS_API lcgs_status lcgs_scene_reorder_spatial(lcgs_context* ctx, uint32_t* d_perm);
/* *d_perm: context-owned, (*d_perm)[r] = file index of row r; NULL in file / caller order.  Valid until the next bind / load. */
LCGS_API lcgs_status lcgs_scene_permutation(lcgs_context* ctx, const uint32_t** d_perm);
/* Device pointers of the bound scene (outputs nullable).  A context-owned scene is READ-ONLY through them: the context keeps
 * rows derived from it; after writing it any other way than through this library, call lcgs_scene_modified. */
LCGS_API lcgs_status lcgs_scene_pointers(lcgs_context* ctx, int* num_gaussians, int* sh_degree, const float** d_pos,
                                         const float** d_scale, const float** d_rotq, const float** d_sh, const float** d_opacity);
/* "The bound arrays were written behind the library's back": derived rows, the f16 coefficient copy and kept frame state
 * are dropped (rows rebuilt at once for a context-owned scene); other contexts on the same arrays are told and act at their
 * next frame.  Order it behind the writes. */
LCGS_API lcgs_status lcgs_scene_modified(lcgs_context* ctx);
/* Diagnostics: derived rows in use that no longer match the bound arrays (0 = consistent).  Synchronises. */
LCGS_API lcgs_status lcgs_debug_verify_derived(lcgs_context* ctx, int64_t* stale_rows);
/* Caller-owned arrays that do not change between frames may have the derived 16-byte cull rows too: declared for exactly
 * these three pointers, until repeated ("contents changed"), withdrawn (num_gaussians 0 / d_pos NULL) or written by the library. */
LCGS_API lcgs_status lcgs_scene_declare_static(lcgs_context* ctx, int num_gaussians, const float* d_pos, const float* d_scale,
                                               const float* d_rotq);
/* Opt-in f16 copy of the degree-3 SH coefficients for the fused forward's colour pass: image moves by ~1e-3, outside the
 * 1e-4 bar by construction.  Call again after the coefficients change / after lcgs_scene_bind.  0 = back to f32. */
LCGS_API lcgs_status lcgs_scene_use_half_sh(lcgs_context* ctx, int enable);
/* Opt-in footprint cull: splats whose reference radius (pixels, gs_tile_splatter/shader.cpp:145-148) is below
 * min_radius_px touch no tile.  Changes the image; never the default; 0 = off.  Stage-level operators ignore it. */
LCGS_API lcgs_status lcgs_set_lod(lcgs_context* ctx, int min_radius_px);
/* Opt-in antialiased frame (the 2-D filter of Mip-Splatting, Yu et al. CVPR 2024; gsplat's rasterize_mode="antialiased"): the
 * 0.3 px^2 dilation of the projected covariance stays, and the frame blends with opacity * rho,
 * rho = sqrt(max(0, det cov2d / det(cov2d + 0.3 I))), so the dilated splat carries the energy of the undilated one.  radii,
 * num_rendered, depths and the order of the lists are the classic frame's; the image changes; never the default.  A kept frame
 * remembers the mode it was rendered in: every backward, lcgs_render_maps, lcgs_contrib_accumulate and the camera gradient work
 * on that frame, whatever the context's mode is by then; dL/dopacity is with respect to the splat's own opacity, and the
 * position / scale / rotation / camera gradients carry d rho.  lcgs_fit_views and batches follow the context's mode.
 * NOT offered: the stage-level operators (lcgs_sh_process / lcgs_project_forward / lcgs_tile_splat_forward, deferred mode
 * included) and the ownership step (lcgs_owner_*, lcgs_owner_step_*) ignore the mode and render and differentiate the classic
 * frame consistently; a per-call mode argument.  (The other half of that paper, the 3-D smoothing filter, is a set of calls of
 * its own that work on the caller's arrays in front of the frame: lcgs_filter3d_accumulate / _finalize / _apply / _backward.)
 * Any other value: LCGS_ERR_INVALID_ARG. */
#define LCGS_RASTER_CLASSIC     0   /* default: the reference's frame, unchanged */
#define LCGS_RASTER_ANTIALIASED 1
LCGS_API lcgs_status lcgs_set_raster_mode(lcgs_context* ctx, int mode);
/* Bound scene -> host arrays sized like lcgs_scene_upload's inputs (NULL outputs skipped).  Synchronises. */
LCGS_API lcgs_status lcgs_scene_download(lcgs_context* ctx, float* h_pos, float* h_scale, float* h_rotq, float* h_sh, float* h_opacity);

/* ---- the fused frame: app/main.cpp:266-308 (process + forward + forward) as one stream submission -------------- */
/* d_img: 3*H*W floats CHW; d_radii: P ints or NULL.  num_rendered non-NULL: synchronises and stores the reference's
 * num_rendered; NULL: only enqueues.  keep_state != 0 keeps what lcgs_render_backward needs. */
LCGS_API lcgs_status lcgs_render_forward(lcgs_context* ctx, const lcgs_camera* camera, const float bg_color[3], float scale_modifier,
                                         float* d_img, int32_t* d_radii, int keep_state, int* num_rendered);
/* A batch of views (two frames in flight on sibling workspaces); d_imgs[i]: 3*H_i*W_i floats for cameras[i].  Enqueues;
 * the context's stream waits for the whole batch. */
LCGS_API lcgs_status lcgs_render_forward_batch(lcgs_context* ctx, int num_views, const lcgs_camera* cameras, const float bg_color[3],
                                               float scale_modifier, float* const* d_imgs);
/* Per-stage device time (ms, hipEvent pairs) of the last forward / backward, while profiling is on (frames then run in order). */
#define LCGS_MAX_STAGES 16
typedef struct lcgs_stage_times {
    int         count;
    const char* name[LCGS_MAX_STAGES];
    float       ms[LCGS_MAX_STAGES];
} lcgs_stage_times;
LCGS_API lcgs_status lcgs_set_profiling(lcgs_context* ctx, int enabled);
LCGS_API lcgs_status lcgs_get_stage_times(lcgs_context* ctx, lcgs_stage_times* out);
/* Counters of the last synchronised frame. */
typedef struct lcgs_frame_stats {
    int64_t num_gaussians;
    int64_t num_visible;            /* radius > 0 and >= 1 tile */
    int64_t num_rendered;           /* the reference's: sum of tiles of the unpruned rects */
    int64_t num_pairs;              /* pairs actually sorted (pruned; at list_shift's granularity) */
    int64_t num_tiles;
    int64_t equal_depth_unresolved; /* always 0 (kept for layout stability) */
    int64_t list_shift;             /* 0: lists per 16 x 16 tile; 1: per block of 2 x 2 tiles */
} lcgs_frame_stats;
LCGS_API lcgs_status lcgs_get_frame_stats(lcgs_context* ctx, lcgs_frame_stats* out);
/* Granularity of the fused frame's sorted pair lists: per tile like the reference (impl.cpp:135-149), per block of 2 x 2
 * tiles (same image bit for bit; fewer pairs through duplication / partition), or AUTO (default): per block for frames
 * without backward state while the last synchronised frame had >= 3 M per-tile pairs and >= 2.2 tiles per on-screen splat. */
#define LCGS_LISTS_PER_TILE 0
#define LCGS_LISTS_PER_BLOCK 1
#define LCGS_LISTS_AUTO 2
LCGS_API lcgs_status lcgs_set_list_policy(lcgs_context* ctx, int policy);
/* Diagnostics (all synchronise).  last_lists: the sorted lists in ORIGINAL splat indices (accel.point_list, proxy.h:62) and
 * ranges (proxy.h:63) at the last frame's granularity (per block: the first ceil(gx/2)*ceil(gy/2) ranges, rest zero).
 * last_state: per pixel final T and 1-based list position of the last contributor of the last keep_state frame
 * (shader.cpp:219-220,252,273).  blend_exp: the compositing loop's defined exp (<= 2.73 ulp on [-6, 0]) for n values in [-86, 0]. */
LCGS_API lcgs_status lcgs_debug_last_lists(lcgs_context* ctx, uint32_t* d_list, uint32_t* d_ranges);
LCGS_API lcgs_status lcgs_debug_last_state(lcgs_context* ctx, float* d_final_T, uint32_t* d_n_contrib);
LCGS_API lcgs_status lcgs_debug_blend_exp(lcgs_context* ctx, const float* d_x, float* d_out, int64_t n);
/* Debug/test hook: forward frames of this context whose cull and sort chain ran on the head stream (enqueue-only frames of a
 * context-owned scene), those of them that chained behind the frame before, and those that rendered with the bounded grid. */
LCGS_API lcgs_status lcgs_debug_pipeline_counts(lcgs_context* ctx, uint64_t* piped, uint64_t* chained, uint64_t* bounded);
/* Debug/test hook: chained frames of this context whose cull pass ran one slot ahead, on the cull stream beside the previous
 * frame's sort chain: the frames that chained while the GPU was behind the host (none if LCGS_EARLY_CULL=0 was set when the
 * context was created). */
LCGS_API lcgs_status lcgs_debug_early_cull_count(lcgs_context* ctx, uint64_t* early);

/* ---- backward of the last lcgs_render_forward(keep_state = 1) (no reference counterpart, README.md:70) ---- */
/* Outputs w.r.t. the ACTIVATED inputs: dL/dpos[3P], dL/dscale[3P], dL/drotq[4P] (as stored; 16-byte aligned),
 * dL/dsh[P*(deg+1)^2*3], dL/dopacity[P]. */
typedef struct lcgs_grads {
    float *d_dL_dpos, *d_dL_dscale, *d_dL_drotq, *d_dL_dsh, *d_dL_dopacity;
} lcgs_grads;
/* dense rows, overwritten (exact zeros off screen) / ADDED to what the arrays hold (further views of a batch) */
LCGS_API lcgs_status lcgs_render_backward(lcgs_context* ctx, const float* d_dL_dimg, const lcgs_grads* grads);
LCGS_API lcgs_status lcgs_render_backward_accumulate(lcgs_context* ctx, const float* d_dL_dimg, const lcgs_grads* grads);
/* Compact rows: row r = the frame's r-th on-screen splat (ascending index; lcgs_visible_rows); only those rows are written. */
LCGS_API lcgs_status lcgs_render_backward_compact(lcgs_context* ctx, const float* d_dL_dimg, const lcgs_grads* grads);
/* (*d_rows)[r] = splat of compact row r, *d_count = device address of the row count.  Valid until the next forward. */
LCGS_API lcgs_status lcgs_visible_rows(lcgs_context* ctx, const uint32_t** d_rows, const uint32_t** d_count);

/* ---- depth and alpha maps of the last lcgs_render_forward(keep_state = 1), and their backward ---- */
/* For pixel p let i run over the entries p blended: the list positions 1..n_contrib[p] that pass the frame's own per-pixel
 * tests (binary32 expressions, exp, thresholds and order of the renderer).  With T_1 = 1, w_i = T_i alpha_i,
 * T_{i+1} = T_i (1 - alpha_i):
 *     alpha[p] = sum_i w_i          depth[p] = sum_i fl(w_i v_i)
 * both summed in list order in binary32, starting from 0.  v_i is the splat's view-space z (LCGS_DEPTH_Z) or 1.0f / z, one
 * IEEE division per splat (LCGS_DEPTH_INV_Z).  Neither map is normalised and no background is blended in: depth is the
 * ACCUMULATED depth, divide by alpha for the expected depth.  A pixel outside every list, and every pixel of a frame that drew
 * nothing, is 0 in both maps (such a frame leaves the colour image untouched; the maps are written).
 * The backward treats thresholds as lcgs_render_backward does: constants; the 0.99 alpha cap passes nothing; a saturated pixel
 * stops. */
#define LCGS_DEPTH_Z 0
#define LCGS_DEPTH_INV_Z 1
/* d_depth, d_alpha: H*W floats each, either (not both) may be NULL.  Enqueues on the context's stream, reads nothing back. */
LCGS_API lcgs_status lcgs_render_maps(lcgs_context* ctx, int mode, float* d_depth, float* d_alpha);
/* The gradient of <dL_dimg, img> + <dL_ddepth, depth> + <dL_dalpha, alpha>: dense rows like lcgs_render_backward's, overwritten
 * (accumulate = 0) or added to (accumulate != 0, like lcgs_render_backward_accumulate).  Any of the three incoming gradients
 * may be NULL, not all three.  The per-splat pass is not sliced for the chunked all-reduce.  lcgs_densify_accumulate behind this
 * call sees the COMBINED 2-D mean gradient (colour + depth + alpha), as 3DGS's viewspace gradient does under a depth loss.
 * Both calls: LCGS_ERR_STATE without a keep_state frame, or after a frame drawn from received records (lcgs_owner_render). */
LCGS_API lcgs_status lcgs_render_backward_maps(lcgs_context* ctx, const float* d_dL_dimg, int mode, const float* d_dL_ddepth,
                                               const float* d_dL_dalpha, int accumulate, const lcgs_grads* grads);

/* ---- depth-distortion map of the last lcgs_render_forward(keep_state = 1), and its backward ---- */
/* The Mip-NeRF 360 distortion loss in the squared form that 2DGS, GOF and RaDe-GS rasterise: it pulls the blend weights of a
 * ray together in depth.  With the entries i, the weights w_i, the value v_i of `mode` and the list order of the maps above,
 * u_i = fl(v_i - center), s_i = fl(u_i u_i):
 *     A = sum_i w_i      M1 = sum_i fl(w_i u_i)      M2 = sum_i fl(w_i s_i)          (binary32, list order, from 0)
 *     dist[p] = fl( fl(A M2) - fl(M1 M1) )       ( = sum_{i<j} w_i w_j (v_i - v_j)^2 in exact arithmetic )
 * The closed form, not 2DGS's running form: three accumulated channels, which a CPU restatement of the frame composites bit
 * for bit as the per-splat colour (u, 1, u u).  `center` is any finite float, 0 included: in exact arithmetic the term does not
 * depend on it; it is there to cut the cancellation between A M2 and M1 M1, which grows with the square of the distance
 * between the values and the centre.  Pass a typical depth of the scene (in inverse-depth mode its reciprocal), e.g. the
 * distance from the camera to the scene's centre.
 * The map is NOT normalised (divide by alpha^2 for the normalised term), NO background is blended in and it is NOT clamped:
 * rounding may leave a pixel with one blended entry a few ulps from 0, on either side.  A pixel outside every list, and every
 * pixel of a frame that drew nothing, is 0.
 * The backward treats thresholds, the 0.99 cap and saturation as lcgs_render_backward does.  With g = dL/ddist[p] and the
 * pixel's own A, M1, M2:
 *     d dist / d w_i = M2 + u_i (A u_i - 2 M1)          d dist / d u_i = 2 w_i (A u_i - M1)
 * the first taken through the blend like a per-pixel value of entry i, the second reaching the position through dv/dz.  The
 * backward re-derives A, M1, M2 itself, with the forward's bits: it needs no preceding lcgs_render_distortion and no map as input.
 * Not offered: a distortion channel in lcgs_render_backward_camera, in lcgs_fit_views, in the ownership step, or as an lcgs-app flag. */
/* d_dist: H*W floats.  Enqueues on the context's stream, reads nothing back. */
LCGS_API lcgs_status lcgs_render_distortion(lcgs_context* ctx, int mode, float center, float* d_dist);
/* lcgs_render_backward_maps with one more channel: the gradient of <dL_dimg, img> + <dL_ddepth, depth> + <dL_dalpha, alpha> +
 * <dL_ddist, dist>, dense rows overwritten (accumulate = 0) or added to.  Any of the four incoming gradients may be NULL, not
 * all four; `mode` holds for the depth and the distortion channel, `center` as above; the three map channels share one walk of
 * the lists.  With d_dL_ddist NULL the call is lcgs_render_backward_maps.  lcgs_densify_accumulate and lcgs_camera_backward work
 * behind it and see the combined gradient.
 * Both calls: LCGS_ERR_STATE without a keep_state frame, or after a frame of lcgs_owner_render.  LCGS_ERR_INVALID_ARG (before
 * any device work): a mode that is neither constant, a non-finite center, a NULL output, all four gradients NULL, a NULL
 * gradient buffer. */
LCGS_API lcgs_status lcgs_render_backward_distortion(lcgs_context* ctx, const float* d_dL_dimg, int mode, float center,
                                                     const float* d_dL_ddepth, const float* d_dL_dalpha, const float* d_dL_ddist,
                                                     int accumulate, const lcgs_grads* grads);

/* ---- normal map of the last lcgs_render_forward(keep_state = 1), and its backward ---- */
/* The blended per-splat normal of every ray, in VIEW space: the other half of the regulariser pair 2DGS, GOF, RaDe-GS and PGSR
 * train with (normal consistency against the normal of the rendered depth surface; the stencil and the loss stay with the
 * caller, who has depth, alpha and normal differentiable).
 * The per-splat normal, per on-screen row, from the BOUND arrays (activated scale s, rotq as stored, pos) and the frame's
 * camera, every operation binary32 and uncontracted; scale_modifier plays no part:
 *     axis         k = 0; if (s[1] < s[k]) k = 1; if (s[2] < s[k]) k = 2;          (the shortest axis, ties to the lower index)
 *     world normal c = column k of the rotation matrix of rotq, (w, x, y, z) as stored, NOT renormalised:
 *                      k = 0: (1 - 2yy - 2zz, 2xy + 2zw, 2xz - 2yw)     every term as ((2 a) b), a difference or sum of two
 *                      k = 1: (2xy - 2zw, 1 - 2xx - 2zz, 2yz + 2xw)     terms as such, the diagonal as ((1 - 2aa) - 2bb);
 *                      k = 2: (2xz + 2yw, 2yz - 2xw, 1 - 2xx - 2yy)     a unit vector for a unit quaternion
 *     facing       d = pos - camera position (componentwise), t = (c0 d0 + c1 d1) + c2 d2;  if (t > 0) c = -c
 *                  (t == 0 and NaN leave c as it is)
 *     view space   n = (right . c, up . c, front . c), each dot product as (a0 b0 + a1 b1) + a2 b2
 * The map, with the entries i, the weights w_i and the list order of the maps above:
 *     normal[c][p] = sum_i fl(w_i n_i,c)          (binary32, list order, from 0;  c = 0, 1, 2;  3*H*W floats, CHW)
 * which a CPU restatement of the frame composites bit for bit as the per-splat colour n.  The map is NOT normalised (divide by
 * alpha, or normalise the vector), NO background is blended in and it is NOT clamped.  A pixel outside every list, and every
 * pixel of a frame that drew nothing, is 0 in all three channels (such a frame leaves the colour image untouched).
 * The backward treats thresholds, the 0.99 cap and saturation as lcgs_render_backward does; the axis k and the flip are
 * constants too.  n_i . dL/dnormal[p] is taken through the blend like a per-pixel value of entry i (to pos, scale, rotq and
 * opacity through the weights, as in every other channel), and dL/dn_i = sum_p w_i dL/dnormal[.][p] reaches rotq alone, through
 * dL/dc = +-(right gn0 + up gn1 + front gn2) and the closed-form derivative of column k: nothing goes to scale or pos from the
 * normal's own value.
 * Like lcgs_camera_backward both calls re-read the BOUND arrays: call them before anything rewrites those.  Both compute the
 * rows' normals themselves: the backward needs no preceding lcgs_render_normals and no map as input.
 * Not offered: world-space output; a normal channel in lcgs_render_backward_camera, lcgs_render_backward_compact, lcgs_fit_views
 * or the ownership step; a fused normal-consistency loss; an lcgs-app flag.  (That loss has since been added as a call of
 * its own on the three maps, outside these two: lcgs_normal_consistency_loss_backward, below.) */
/* d_normal: 3*H*W floats, CHW.  Enqueues on the context's stream, reads nothing back.  Stages under lcgs_set_profiling:
 * splat_normals, render_normals. */
LCGS_API lcgs_status lcgs_render_normals(lcgs_context* ctx, float* d_normal);
/* lcgs_render_backward_distortion with a fifth channel: the gradient of <dL_dimg, img> + <dL_ddepth, depth> + <dL_dalpha, alpha>
 * + <dL_ddist, dist> + <dL_dnormal, normal>, dense rows overwritten (accumulate = 0) or added to.  d_dL_dnormal: 3*H*W floats,
 * CHW.  Any of the five incoming gradients may be NULL, not all five; all map channels share one walk of the lists.  With
 * d_dL_dnormal NULL the call is lcgs_render_backward_distortion.  lcgs_densify_accumulate works behind it and sees the combined
 * 2-D gradient.  lcgs_camera_backward behind a call that passed a non-NULL d_dL_dnormal returns LCGS_ERR_STATE: the view-space
 * normal depends on the camera's rotation directly, that term is not built, and a silently incomplete gradient is worse than a
 * refusal; behind any later backward of the frame it works as before.
 * Both calls: LCGS_ERR_STATE without a keep_state frame, or after a frame of lcgs_owner_render.  LCGS_ERR_INVALID_ARG (before
 * any device work): NULL ctx, output or grads, a NULL gradient buffer, a mode that is neither constant, a non-finite center,
 * all five gradients NULL.  Stages under lcgs_set_profiling: splat_normals, render_maps_backward, normals_to_rot. */
LCGS_API lcgs_status lcgs_render_backward_normals(lcgs_context* ctx, const float* d_dL_dimg, int mode, float center,
                                                  const float* d_dL_ddepth, const float* d_dL_dalpha, const float* d_dL_ddist,
                                                  const float* d_dL_dnormal, int accumulate, const lcgs_grads* grads);

/* ---- caller-supplied per-splat feature channels of the last lcgs_render_forward(keep_state = 1), and their backward ---- */
/* Per-splat vectors the CALLER brings, blended like colour: semantic logits, distilled CLIP / DINO / SAM features (Feature-3DGS,
 * LangSplat, LEGaussians), instance ids as one-hot rows, per-splat uncertainty.  The general case of the normal channel: the
 * vector f_i has K components, comes from the caller and its gradient goes back to the caller.
 * d_features: P x K floats, row-major, row r the features of row r of the context's scene arrays -- the context's row order,
 * as lcgs_grads' arrays: after lcgs_scene_upload that is the spatial (Morton) order of lcgs_scene_permutation.  num_gaussians
 * must be the bound scene's P.  A row of odd K need not be 16-byte aligned.
 * The map, with the entries i, the weights w_i and the list order of lcgs_render_maps:
 *     feature_map[c][p] = sum_i fl(w_i f_i,c)          (binary32, list order, from 0;  c = 0 .. K-1;  K*H*W floats, CHW)
 * the multiply and the add separate operations (the build does not contract, and no matrix instruction is used: an f32 MFMA
 * is an fmaf chain), which a CPU restatement of the frame composites bit for bit, three columns at a time, as the per-splat
 * colour.  The map is NOT normalised (divide by alpha), NO background is blended in and it is NOT clamped.  A pixel outside
 * every list, and every pixel of a frame that drew nothing, is 0 in all K channels (such a frame leaves the colour image
 * untouched).  The call reads the kept state, so it works on antialiased and LOD frames unchanged.
 * The backward treats thresholds, the 0.99 cap and saturation as lcgs_render_backward does.  f_i . dL/dfeature_map[.][p] is
 * taken through the blend like a per-pixel value of entry i (to pos, scale, rotq and opacity through the weights, as in every
 * other channel), and dL/df_i,c = sum_p w_i dL/dfeature_map[c][p] goes to d_dL_dfeatures.  Nothing reaches sh, and nothing
 * reaches pos, scale or rotq from the feature's own value.  d_dL_dfeatures is summed by float atomics in unspecified order: the
 * last bits of a row that several tiles blend vary from run to run, as weight_sum's do.
 * Not offered: compact rows; a feature channel in lcgs_render_backward_camera, lcgs_fit_views or the ownership step; an
 * lcgs-app flag; f16 features. */
#define LCGS_FEATURES_MAX 256
typedef struct lcgs_feature_channel {
    int          channels;           /* K, 1 .. LCGS_FEATURES_MAX */
    const float* d_features;         /* P x K, row-major, the context's row order (as lcgs_grads' arrays) */
    const float* d_dL_dfeature_map;  /* K x H x W (CHW); backward only */
    float*       d_dL_dfeatures;     /* P x K; backward only; may be NULL (features frozen) */
} lcgs_feature_channel;
/* d_feature_map: K*H*W floats, CHW.  Enqueues on the context's stream, reads nothing back.  K channels are walked in chunks of
 * 4, 8 or 16 (the smallest that holds K, 16 beyond): ceil(K / 16) walks of the lists for a large K.  Stage under
 * lcgs_set_profiling: render_features. */
LCGS_API lcgs_status lcgs_render_features(lcgs_context* ctx, int num_gaussians, int channels, const float* d_features,
                                          float* d_feature_map);
/* lcgs_render_backward_normals with one more channel group: the gradient of <dL_dimg, img> + <dL_ddepth, depth> +
 * <dL_dalpha, alpha> + <dL_ddist, dist> + <dL_dnormal, normal> + <dL_dfeature_map, feature_map>, dense rows overwritten
 * (accumulate = 0) or added to; `accumulate` holds for the rows of `grads` and for d_dL_dfeatures alike, and with
 * accumulate = 0 the rows that nothing blends are exact zeros in both.  With feat NULL the call is
 * lcgs_render_backward_normals.  feat->d_dL_dfeatures NULL with grads given: the features are frozen, only the geometry rows
 * are written.  grads NULL is allowed when every other incoming gradient is NULL and feat->d_dL_dfeatures is not: the
 * frozen-geometry mode (LangSplat's) -- the walk then forms no geometry sums, and the frame's 2-D gradient rows are left as they
 * were, so lcgs_camera_backward and lcgs_densify_accumulate behind it give what they gave before the call.  Both NULL is an
 * argument error.  Otherwise lcgs_densify_accumulate and lcgs_camera_backward work behind the call and see the combined 2-D
 * gradient: a caller-supplied feature has no direct camera term, so nothing is refused on its account (the refusal behind a
 * non-NULL d_dL_dnormal stays).
 * Both calls: LCGS_ERR_STATE without a keep_state frame, or after a frame of lcgs_owner_render.  LCGS_ERR_INVALID_ARG (before
 * any device work): NULL ctx, rows, map or map gradient, channels outside 1 .. LCGS_FEATURES_MAX, a num_gaussians that is not
 * the bound scene's, every gradient NULL, a NULL gradient buffer, a mode that is neither constant, a non-finite center.
 * Stages under lcgs_set_profiling: those of lcgs_render_backward_normals, zero_features (accumulate = 0), render_features_backward. */
LCGS_API lcgs_status lcgs_render_backward_features(lcgs_context* ctx, const float* d_dL_dimg, int mode, float center,
                                                   const float* d_dL_ddepth, const float* d_dL_dalpha, const float* d_dL_ddist,
                                                   const float* d_dL_dnormal, const lcgs_feature_channel* feat, int accumulate,
                                                   const lcgs_grads* grads);

/* ---- per-splat blend-weight statistics of the last lcgs_render_forward(keep_state = 1) ---- */
/* Which splats a set of views actually uses.  w is the w_i = T_i alpha_i above: the weight pixel p gives entry i of its list, for
 * the entries p blended (positions up to n_contrib[p] that pass the renderer's power and 1/255 tests, the 0.99 cap and the
 * renderer's exp applied).  For every row with at least one such (pixel, entry) in the kept frame:
 *     weight_sum += sum of w     weight_max = max(., max w)     pixels += number of such pairs     views += 1
 * Every other row is untouched -- rows that sit on a list but that no pixel blends included.  Pixels outside the image (partial
 * tiles) contribute nothing; a frame that drew nothing touches nothing.  Rows follow the context's row order, like
 * lcgs_densify_accumulate.  No backward is needed.
 * Precision: weight_max, pixels and views are exact (a max of non-negative floats and integer sums do not depend on order) and
 * equal a binary32 CPU restatement of the frame bit for bit.  weight_sum is a binary32 sum of those bit-exact terms in an
 * UNSPECIFIED order (float atomics across tiles): its bits may differ from run to run, within
 *     |weight_sum - exact sum| <= gamma_n x exact sum,   gamma_n = n u / (1 - n u),  u = 2^-24,  n = the row's pixel count.
 * Not offered: frames of the ownership step (lcgs_owner_render), a fused "score while rendering" mode, gradient-weighted scores,
 * an lcgs-app flag. */
typedef struct lcgs_contrib_stats { /* caller-owned, P entries each, zeroed by the caller; any member may be NULL, not all */
    float*    weight_sum; /* sum over views and pixels of w                         */
    float*    weight_max; /* largest w of any pixel of any view                     */
    uint32_t* pixels;     /* number of (view, pixel) pairs that blended the row     */
    uint32_t* views;      /* number of views in which at least one pixel blended it */
} lcgs_contrib_stats;
/* Enqueues on the context's stream, reads nothing back.  LCGS_ERR_STATE without a keep_state frame, or after a frame of
 * lcgs_owner_render.  LCGS_ERR_INVALID_ARG (before any device work): NULL ctx / stats, all four members NULL, num_gaussians not
 * the bound scene's.  Stages under lcgs_set_profiling: contrib_walk, contrib_fold. */
LCGS_API lcgs_status lcgs_contrib_accumulate(lcgs_context* ctx, int num_gaussians, const lcgs_contrib_stats* stats);

/* ---- camera gradient: the frame differentiated with respect to its camera pose ---- */
/* Twelve floats in the order of lcgs_camera's members: position[3], front[3], up[3], right[3].  They are the gradient of the
 * scalar the LAST backward differentiated, <dL_dimg, img> + <dL_ddepth, depth> + <dL_dalpha, alpha>, the frame taken as a
 * function of those twelve reals as INDEPENDENT variables with fov, aspect_ratio, width and height fixed.  The kernels' camera
 * constants derive from them as the host derives them: campos = position, view rows right / up / front,
 * t = -(right.position, up.position, front.position).  No orthonormality constraint is imposed: whoever parameterises the
 * pose chains onto the twelve numbers (lcgs_camera_grad_to_twist does it for a twist in the camera's own frame).
 * Thresholds, cull decisions, tile rectangles and list membership are constants, as in lcgs_render_backward.
 * Per on-screen splat i, with d = pos_i - position, dv / dT0 / dT1 the gradients w.r.t. its view-space position (the depth
 * channel's dL/dz included) and its two projected covariance axes, j00, j11, j02, j12 the projection Jacobian's entries and
 * gdir the view-direction part of dL/dpos_i from the colour step:
 *     g_position = - sum_i (right dv0 + up dv1 + front dv2 + gdir)        ( = - sum_i dL/dpos_i )
 *     g_right    =   sum_i (dv0 d + j00 dT0)
 *     g_up       =   sum_i (dv1 d + j11 dT1)
 *     g_front    =   sum_i (dv2 d + j02 dT0 + j12 dT1)
 * Per-splat terms are formed in the precision of the parameter pass (binary32; binary64 for screen-filling footprints), the
 * twelve sums are accumulated in binary64 in a tree that depends on the number of on-screen rows only (no atomics: the same
 * 2-D rows give the same bits) and rounded once.  A frame that drew nothing gives twelve zeros.
 * Like lcgs_densify_accumulate the pass re-evaluates geometry from the BOUND arrays: call it before anything rewrites them
 * (behind lcgs_render_backward_adam it sees the updated scene).
 * Not offered: gradients w.r.t. fov / aspect_ratio, frames of the ownership step, pose gradients inside lcgs_fit_views. */
/* The camera gradient of the last backward of the kept frame (any of lcgs_render_backward, _accumulate, _compact,
 * lcgs_render_backward_maps, lcgs_render_backward_distortion, lcgs_render_backward_adam, lcgs_render_backward_camera), from
 * the 2-D rows the context still holds (behind lcgs_render_backward_distortion the distortion channel's dL/dz is part of dv).  d_dL_dcam: 12 floats, device, overwritten.  Enqueues on the context's stream, reads nothing back.
 * LCGS_ERR_STATE: no keep_state frame, a frame of lcgs_owner_render, or no backward of the frame yet. */
LCGS_API lcgs_status lcgs_camera_backward(lcgs_context* ctx, float* d_dL_dcam);
/* Walks + camera pass, NO parameter gradients: the 2-D rows zeroed, the colour walk (d_dL_dimg), the maps walk (d_dL_ddepth /
 * d_dL_dalpha, mode as in lcgs_render_backward_maps), lcgs_camera_backward.  Any of the three may be NULL, not all.  Counts as
 * a backward of the frame: lcgs_densify_accumulate and lcgs_camera_backward work behind it. */
LCGS_API lcgs_status lcgs_render_backward_camera(lcgs_context* ctx, const float* d_dL_dimg, int mode, const float* d_dL_ddepth,
                                                 const float* d_dL_dalpha, float* d_dL_dcam);
/* Host only: the 12 numbers -> the gradient w.r.t. a twist xi = (omega, tau) applied in the camera's own frame,
 * [right up front]' = [right up front] exp([omega]x), position' = position + [right up front] tau, at xi = 0:
 *     dL/dtau   = (right.g_position, up.g_position, front.g_position)
 *     dL/domega = sum_k e_k x (Rc^T g_k),  e_0..2 = unit vectors, g_0..2 = g_right, g_up, g_front, Rc = [right up front]
 * evaluated in binary64, each output rounded once.  dL_dxi: omega[3], tau[3]. */
LCGS_API lcgs_status lcgs_camera_grad_to_twist(const lcgs_camera* cam, const float dL_dcam[12], float dL_dxi[6]);

/* ---- optimiser step (doc/roadmap.md:4 names training; 3DGS parameterisation: scale = exp, opacity = sigmoid, rotq normalised) ---- */
typedef struct lcgs_params {
    float *pos, *scale, *rotq, *sh, *opacity; /* device arrays laid out like the scene */
} lcgs_params;
typedef struct lcgs_adam_config {
    float lr_pos, lr_sh_dc, lr_sh_rest, lr_opacity, lr_scale, lr_rot;
    float beta1, beta2, eps;
    int   step;         /* 1, 2, ... (bias correction) */
    int   visible_only; /* 0 every splat; 1 on-screen splats, per-splat gradient rows; 2 on-screen, compact rows */
} lcgs_adam_config;
/* Gradients w.r.t. activated values -> Adam (torch.optim.Adam semantics) on raw / m / v in place -> `activated` rewritten
 * (pos / sh may alias raw).  visible_only refers to the context's last forward frame. */
LCGS_API lcgs_status lcgs_adam_step(lcgs_context* ctx, int num_gaussians, int sh_degree, const lcgs_adam_config* cfg, const lcgs_grads* grads,
                                    const lcgs_params* raw, const lcgs_params* m, const lcgs_params* v, const lcgs_params* activated);
/* lcgs_render_backward_compact + lcgs_adam_step(visible_only = 2) in one pass, no gradient arrays (same bits). */
LCGS_API lcgs_status lcgs_render_backward_adam(lcgs_context* ctx, const float* d_dL_dimg, int num_gaussians, int sh_degree,
                                               const lcgs_adam_config* cfg, const lcgs_params* raw, const lcgs_params* m,
                                               const lcgs_params* v, const lcgs_params* activated);
/* *d_loss = mean((img - target)^2), d_dL_dimg = its gradient (what lcgs_render_backward takes).  Device pointers. */
LCGS_API lcgs_status lcgs_l2_loss_backward(lcgs_context* ctx, int width, int height, const float* d_img_chw, const float* d_target_chw,
                                           float* d_dL_dimg, float* d_loss);
/* The 3DGS training loss of two CHW float32 images [3][H][W] (the layout lcgs_render_forward writes):
 *   window      w[k] = exp(-(k - 5)^2 / (2 1.5^2)) / sum, k = 0..10, as binary32 constants rounded from the binary64 values; the
 *               2-D window G = w w^T, applied per channel with ZERO padding of 5 (conv2d(padding = 5, groups = 3))
 *   statistics  mu1 = G*x, mu2 = G*y, s1 = G*x^2 - mu1^2, s2 = G*y^2 - mu2^2, s12 = G*xy - mu1 mu2; C1 = 0.01^2, C2 = 0.03^2
 *   ssim        ((2 mu1 mu2 + C1)(2 s12 + C2)) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)) per element; SSIM = its mean over 3 H W
 *   loss        (1 - lambda) L1 + lambda (1 - SSIM), L1 = mean|x - y|
 *   gradient    dL/dx = (1 - lambda) sign(x - y) / n - (lambda / n) [ G*a + 2 x (G*b) + y (G*c) ], n = 3 H W, sign(0) = 0,
 *               a = d ssim / d mu1 with s1 and s12 expanded (it includes the -2 mu1 and -mu2 terms), b = d ssim / d s1,
 *               c = d ssim / d s12; G is symmetric, so the adjoint of the zero-padded convolution is that convolution
 * *d_loss = (1 - lambda_dssim) * mean|img - target| + lambda_dssim * (1 - SSIM(img, target)), the 3DGS training loss;
 * d_dL_dimg (nullable: evaluation only) = its gradient w.r.t. img, what lcgs_render_backward takes;
 * d_terms (nullable) = { L1, SSIM }.  Device pointers; only enqueues; same inputs -> same bits. */
LCGS_API lcgs_status lcgs_photometric_loss_backward(lcgs_context* ctx, int width, int height, const float* d_img_chw,
                                                    const float* d_target_chw, float lambda_dssim, float* d_dL_dimg,
                                                    float* d_loss, float* d_terms);
/* The normal-consistency loss of a frame's maps, the other half of the regulariser pair 2DGS, GOF, RaDe-GS and PGSR train with
 * (the distortion term is a map, its loss a mean): the rendered normal against the normal of the rendered depth surface.
 * Inputs of a W x H frame, binary32 device arrays as the library writes them: depth[H*W], the accumulated view z of
 * LCGS_DEPTH_Z mode (lcgs_render_maps); alpha[H*W]; normal[3*H*W], CHW, view space (lcgs_render_normals).  `camera` supplies
 * width, height, fov and aspect_ratio ONLY: the pose plays no part.  All per-pixel algebra is binary64, uncontracted, the
 * inputs widened exactly, each output rounded to binary32 once (the edge vectors are differences of neighbouring points whose
 * z agree to three or four digits on a smooth surface, and the result is divided by the length of their cross product):
 *     tany = tan((double)fov / 180 * pi * 0.5)      tanx = tany * (double)aspect_ratio
 *     rx(x) = ((x + 0.5) / W * 2 - 1) * tanx        ry(y) = ((y + 0.5) / H * 2 - 1) * tany       (pixel centres)
 *     z_q   = depth_q / max(alpha_q, alpha_min)      P_q = (rx z_q, ry z_q, z_q)                 (view space)
 *     for every INTERIOR pixel p = (x, y), 1 <= x <= W-2, 1 <= y <= H-2:
 *       ex = P(x+1,y) - P(x-1,y)     ey = P(x,y+1) - P(x,y-1)
 *       m  = ey x ex                 (faces the camera: a fronto-parallel plane gives (0, 0, -1), the sign convention of the
 *                                     rendered normals' facing rule)
 *       s  = sqrt(m.m + 1e-20)       nt = m / s
 *       term_p = alpha_p - normal_p . nt
 *     loss = weight / ((W-2)(H-2)) * sum_p term_p     (binary64 sum in a fixed order; same inputs -> same bits)
 * Gradients, with c = weight / ((W-2)(H-2)); zero where nothing below reaches, the border included:
 *     dL/dnormal_p = -c nt                                   (interior p)
 *     g_m  = -c (normal_p / s - m (m . normal_p) / s^3)      g_ey = ex x g_m       g_ex = g_m x ey      (interior p, else 0)
 *     G_q  = g_ex(q - x^) - g_ex(q + x^) + g_ey(q - y^) - g_ey(q + y^)           (a GATHER over q's four neighbours)
 *     g_z  = G_q . (rx, ry, 1)
 *     dL/ddepth_q = g_z / max(alpha_q, alpha_min)
 *     dL/dalpha_q = [q interior] c  +  (alpha_q >= alpha_min ? -g_z depth_q / alpha_q^2 : 0)
 * alpha_q is differentiated both in the leading alpha_p and through z: nothing is detached.  The clamp passes its gradient at
 * equality, as torch.clamp_min does.
 * The three gradients (d_dL_ddepth[H*W], d_dL_dalpha[H*W], d_dL_dnormal[3*H*W]: what lcgs_render_backward_normals takes) are
 * either all non-NULL or all NULL.  All NULL is evaluation only: the call writes the loss, and its bits equal the gradient
 * call's loss.  Gradients are overwritten, never accumulated, and the whole array is written, zeros at the border included.
 * The call needs no kept frame: it is a function of its arguments, like the photometric loss.  It enqueues on the context's
 * stream, reads nothing back and uses no atomics.
 * LCGS_ERR_INVALID_ARG (before any device work): a NULL ctx, camera, input or loss pointer; width or height below 3; a weight
 * that is not finite or is negative; an alpha_min that is not finite or is <= 0; gradient pointers of which some but not all
 * are NULL; a gradient buffer that overlaps any input or another gradient buffer (the gather reads neighbours).
 * Not offered: the term inside lcgs_fit_views; LCGS_DEPTH_INV_Z input; world-space normals; a median-depth surface; an
 * lcgs-app flag for it; a camera gradient. */
LCGS_API lcgs_status lcgs_normal_consistency_loss_backward(lcgs_context* ctx, const lcgs_camera* camera, const float* d_depth,
                                                           const float* d_alpha, const float* d_normal, float weight,
                                                           float alpha_min, float* d_dL_ddepth, float* d_dL_dalpha,
                                                           float* d_dL_dnormal, float* d_loss);
/* Depth-prior supervision: the rendered depth of a frame against a depth the caller brings (a monocular estimate, a sensor, a
 * COLMAP-scaled map), the term sparse-view and indoor recipes add first.  Two kinds: the Pearson-correlation loss of FSGS,
 * SparseGS and DNGaussian (per patch in the last two: a monocular prior is only locally affine-correct), and 3DGS's "depth
 * regularisation", an L1 against the prior aligned by a scale and a shift.
 * Inputs of a W x H frame, binary32 device arrays: depth[H*W] and alpha[H*W] as lcgs_render_maps writes them, prior[H*W], and
 * mask[H*W] bytes (nullable).  The call does not care which map mode produced depth: render LCGS_DEPTH_INV_Z for a disparity
 * prior and LCGS_DEPTH_Z for a metric one.
 * Arithmetic: all per-pixel and per-group algebra is binary64, uncontracted, the inputs widened exactly; every output is
 * rounded to binary32 once; all sums run in a fixed order with no float atomics: same inputs -> same bits, across calls and
 * contexts.
 *     value    v_p = depth_p / max(alpha_p, alpha_min)           m_p = prior_p
 *     valid    (d_mask == NULL or mask_p != 0) and isfinite(prior_p)
 *     group    patch == 0: the whole image.  Otherwise the patch x patch blocks of the grid anchored at pixel
 *              (-patch_x, -patch_y), cut at the image border (the offsets let a trainer jitter the grid per step)
 *     counted  a group that holds at least 2 valid pixels; under LCGS_DEPTH_ALIGN_GIVEN there is one group and 1 valid pixel
 *              suffices.  G = the number of counted groups, N_c = the number of valid pixels in counted groups
 * Per-group statistics over the n valid pixels of a counted group, the means first, then centred sums (two passes, not raw
 * moments); eps = 1e-12:
 *     mu_v = sum v / n      mu_m = sum m / n
 *     var_v = sum (v - mu_v)^2 / n      var_m = sum (m - mu_m)^2 / n      cov = sum (v - mu_v)(m - mu_m) / n
 *     r = cov / sqrt((var_v + eps)(var_m + eps))      s = cov / (var_m + eps)      t = mu_v - s mu_m
 * (a constant prior gives m - mu_m = 0 exactly, so r = 0 and s = 0).
 * LCGS_DEPTH_PRIOR_PEARSON:
 *     loss = weight / G * sum_g (1 - r_g)             (0 if G == 0)
 *     g_v(p) = -weight / (G n) * [ (m_p - mu_m) - cov (v_p - mu_v) / (var_v + eps) ] / sqrt((var_v + eps)(var_m + eps))
 * LCGS_DEPTH_PRIOR_L1:
 *     res_p = v_p - (s_g m_p + t_g)      loss = weight / N_c * sum |res_p|      (0 if N_c == 0)
 *     g_v(p) = weight / N_c * sign(res_p), sign(0) = 0
 *   s and t are constants of the gradient: they are detached, as in a fit done under no_grad or taken from COLMAP.
 *   LCGS_DEPTH_ALIGN_GIVEN uses cfg->scale and cfg->shift for s and t and computes no statistics.
 * The chain to the maps, for the valid pixels of counted groups; every other pixel gets an exact zero:
 *     dL/ddepth_p = g_v / max(alpha_p, alpha_min)
 *     dL/dalpha_p = (alpha_p >= alpha_min ? -g_v depth_p / alpha_p^2 : 0)          (the clamp passes its gradient at equality)
 * d_dL_ddepth[H*W] and d_dL_dalpha[H*W] (what lcgs_render_backward_maps takes) are both non-NULL or both NULL.  Both NULL is
 * evaluation only: the call writes the loss, and its bits equal the gradient call's loss.  Both arrays are written whole,
 * overwritten, never accumulated.
 * d_stats (nullable, 4 floats) = { N_c, G, s, t }: the group's fit when patch == 0, the given pair under
 * LCGS_DEPTH_ALIGN_GIVEN, zeros for s and t in patch mode.
 * The call needs no kept frame: it is a function of its arguments.  It enqueues on the context's stream and reads nothing back.
 * LCGS_ERR_INVALID_ARG (before any device work): a NULL ctx, cfg, input or loss pointer; a width or height that is not
 * positive; an unknown kind or align; LCGS_DEPTH_ALIGN_GIVEN with the Pearson kind or with patch != 0; a scale or shift that
 * is not finite under LCGS_DEPTH_ALIGN_GIVEN; a weight that is not finite or is negative; an alpha_min that is not finite or
 * is <= 0; a patch that is not 0, 32, 64 or 128, or an offset outside [0, patch); exactly one gradient pointer NULL; any
 * output (gradients, loss, stats) that overlaps any input or another output.
 * Not offered: FSGS's min over two depth transforms; random or overlapping patches; a non-detached alignment; the term inside
 * lcgs_fit_views; an lcgs-app flag for it; a camera gradient. */
#define LCGS_DEPTH_PRIOR_PEARSON 0
#define LCGS_DEPTH_PRIOR_L1      1
#define LCGS_DEPTH_ALIGN_FIT     0   /* per-group least-squares scale and shift of the prior, detached */
#define LCGS_DEPTH_ALIGN_GIVEN   1   /* L1 only: the caller's scale and shift (3DGS: from COLMAP) */
typedef struct lcgs_depth_prior_config {
    int   kind, align;
    float scale, shift;               /* ALIGN_GIVEN */
    float weight, alpha_min;
    int   patch, patch_x, patch_y;    /* 0 = one group (the image); else 32, 64 or 128 with 0 <= patch_x, patch_y < patch */
} lcgs_depth_prior_config;
LCGS_API lcgs_status lcgs_depth_prior_loss_backward(lcgs_context* ctx, int width, int height, const float* d_depth,
                                                    const float* d_alpha, const float* d_prior, const uint8_t* d_mask,
                                                    const lcgs_depth_prior_config* cfg, float* d_dL_ddepth, float* d_dL_dalpha,
                                                    float* d_loss, float* d_stats);
/* Per-view bilateral-grid colour correction ("Bilateral Guided Radiance Field Processing"; gsplat's use_bilateral_grid): what
 * absorbs the exposure, white balance and tone curve that change from photograph to photograph, so that the scene does not.
 * Each training view owns a small 3-D grid of 3 x 4 affine colour transforms; the grid is sliced at (pixel x, pixel y,
 * luminance of the rendered pixel), the transform is applied to the rendered colour in front of the photometric loss, and a
 * total-variation term keeps each grid smooth.
 * One view's grid is float32 [12][L][GH][GW], contiguous: the layout of a torch (12, L, GH, GW) tensor.  Channel c = 4 r + k is
 * entry (row r, column k) of the 3 x 4 matrix: columns 0..2 multiply r, g, b, column 3 is the offset.  A training set's grids
 * are [N][12][L][GH][GW]; a slice or backward call takes one view's slab.  (gw, gh, gl) = (GW, GH, L); the usual choice is
 * (16, 16, 8); accepted: 2 <= gw, gh <= 256 and 2 <= gl <= 16.  Images are float32 [3][H][W] as everywhere else, W, H >= 1.
 * For pixel (px, py) with input colour c = (r, g, b), in binary32, uncontracted:
 *     x = ((float)px + 0.5f) / W * (GW-1)      x0 = min(floor(x), GW-2)      fx = x - x0      (the same for y with H and GH;
 *                                                                                              x and y never reach the border)
 *     gray = 0.299f*r + 0.587f*g + 0.114f*b     (the three products summed in that order)
 *     zr = gray*(L-1)      z = clamp(zr, 0, L-1)      z0 = min((int)z, L-2)      fz = z - z0
 *     A[c] = the trilinear sample of channel c at (x, y, z), written as nested lerps a + t*(b - a): along x, then y, then z
 *     out_r = A[4r]*r + A[4r+1]*g + A[4r+2]*b + A[4r+3]
 * With the nested-lerp form an identity grid returns a finite image bit for bit (every lerp is a + t*0), the sign of a zero
 * aside: a channel that is -0 comes back as +0 when the sum of the other products is +0.
 * This is torch.nn.functional.grid_sample(grid[None], coords, mode="bilinear", padding_mode="border", align_corners=True) with
 * coords = 2 (x/(GW-1), y/(GH-1), gray) - 1, followed by the affine apply (tests/bilagrid_ref.py).
 * Backward, given g = dL/dout, with hat(t) = max(0, 1 - |t|):
 *     dL/dgrid[c=4r+k][l][j][i] = sum over pixels of hat(x-i) hat(y-j) hat(z-l) g_r (k<3 ? c_k : 1)
 *     dL/dc_k = sum_r A[4r+k] g_r + w_k (L-1) inside sum_r g_r (dA[4r..4r+3]/dz . (r,g,b,1))
 *     dA/dz = the xy-bilinear sample at level z0+1 minus the one at z0         w = (0.299f, 0.587f, 0.114f)
 *     inside = (zr > 0 && zr < L-1)
 * The guidance passes no gradient where it is clamped, exactly 0 included: black background pixels pass none.  At an interior
 * integer z the cell is the one above (floor).  Both rules are grid_sample's.
 * dL/dgrid is a gather, not a scatter: every vertex sums the pixels in its reach in a fixed order (a lane's run of pixels in
 * binary32 for gl <= 8, everything across lanes and row slices in binary64, rounded to binary32 once); no float atomics.
 * Vertices that no pixel reaches are written as exact zeros (more vertices than pixels is a legal call).
 * lcgs_bilagrid_backward: d_dL_dimg_chw (3*H*W floats) and d_dL_dgrid (12*L*GH*GW floats) are each optional (NULL: not wanted,
 * nothing is computed for it and the other's bits do not change), not both NULL.
 * The TV term over N grids:
 *     loss = weight/N * sum over axis in {x,y,z} of sum (grid[v+e_axis] - grid[v])^2 / count_axis
 * count_axis = the number of differences along that axis in ONE grid, times 12: for x, 12 L GH (GW-1).  The per-element algebra
 * is binary64, the sum is binary64 in a fixed order, the loss and each gradient element are rounded to binary32 once.
 * d_dL_dgrids NULL is evaluation only: *d_loss has the gradient call's bits.  weight = 0 gives exact zeros.
 * All outputs are overwritten, never accumulated.  The same inputs give the same bits, across calls and across contexts.  No
 * call needs a kept frame or reads anything back; each enqueues on the context's stream.  Workspace: the buffer the photometric
 * loss uses, grown on demand.  The grids are ordinary caller-owned arrays: the caller's optimiser steps them.
 * LCGS_ERR_INVALID_ARG (before any device work): a NULL ctx or required pointer; a non-positive width or height; grid
 * dimensions outside the accepted ranges; a weight that is not finite or is negative; num_grids <= 0; both gradient pointers
 * NULL in lcgs_bilagrid_backward; any output that overlaps any input or another output (in-place slicing is not offered);
 * in lcgs_bilagrid_tv_loss_backward, more than 2^31 - 1 workgroups of 256 grid elements (num_grids is too large for one call).
 * Not offered: the grid inside lcgs_fit_views or lcgs-app; a library optimiser for grids; interpolation between views' grids;
 * slicing fused into the photometric loss; guidance other than the input's luminance. */
LCGS_API lcgs_status lcgs_bilagrid_slice(lcgs_context* ctx, int width, int height, const float* d_grid, int gw, int gh, int gl,
                                         const float* d_img_chw, float* d_out_chw);
LCGS_API lcgs_status lcgs_bilagrid_backward(lcgs_context* ctx, int width, int height, const float* d_grid, int gw, int gh, int gl,
                                            const float* d_img_chw, const float* d_dL_dout_chw, float* d_dL_dimg_chw,
                                            float* d_dL_dgrid);
LCGS_API lcgs_status lcgs_bilagrid_tv_loss_backward(lcgs_context* ctx, const float* d_grids, int num_grids, int gw, int gh, int gl,
                                                    float weight, float* d_dL_dgrids, float* d_loss);
#define LCGS_LOSS_L2 0
#define LCGS_LOSS_PHOTOMETRIC 1
/* The loss lcgs_fit_views applies (default LCGS_LOSS_L2: unchanged behaviour). */
LCGS_API lcgs_status lcgs_set_fit_loss(lcgs_context* ctx, int kind, float lambda_dssim);
/* The views of ONE optimiser step: forward(keep_state) -> the selected loss (lcgs_set_fit_loss; L2 unless told otherwise) vs
 * d_targets[j] -> backward per view, dense gradients
 * summed into `grads`, d_losses[j] (device); views alternate between the context and its sibling.  The context's stream
 * waits for the batch; the context holds the last view's frame state. */
LCGS_API lcgs_status lcgs_fit_views(lcgs_context* ctx, int num_views, const lcgs_camera* cameras, const float bg_color[3],
                                    float scale_modifier, const float* const* d_targets, const lcgs_grads* grads, float* d_losses);

/* ---- adaptive density control (no reference counterpart: doc/roadmap.md:4 only names training) -------------- */
/* Per-splat statistics of the steps since the last rewrite, caller-owned, zeroed by the caller (lcgs_densify zeroes its outputs). */
typedef struct lcgs_densify_stats {
    float*    grad_accum; /* P: sum over frames of |dL/d(mean in NDC)| */
    uint32_t* denom;      /* P: frames in which the row was on screen   */
    int32_t*  max_radii;  /* P: largest screen radius seen (pixels)     */
} lcgs_densify_stats;
/* The context's last keep_state lcgs_render_forward and the backward that followed it (any variant): for every on-screen row,
 * grad_accum += |(gx W/2, gy H/2)| of its pixel-space mean gradient, denom += 1, max_radii = max(., reference radius,
 * gs_tile_splatter/shader.cpp:145-148).  Other rows untouched; the context's row order.  LCGS_ERR_STATE: no such frame, no
 * backward on it yet, or a frame of lcgs_owner_render.  Only enqueues.  Behind lcgs_render_backward_maps or
 * lcgs_render_backward_distortion the mean gradient is the combined one of every channel that call was given. */
LCGS_API lcgs_status lcgs_densify_accumulate(lcgs_context* ctx, int num_gaussians, const lcgs_densify_stats* stats);
/* AbsGS densification statistics (Ye et al. 2024; GOF's criterion, gsplat's absgrad): the sum over PIXELS of the absolute per-pixel
 * gradient of the pixel-space mean, where lcgs_densify_accumulate takes the norm of the summed one -- a large splat that is wrong
 * in opposite directions on its two sides sums to almost nothing there and is never split.
 * The frame is the context's last lcgs_render_forward(keep_state = 1), classic or antialiased (the frame remembers its mode), and
 *     L = <dL_dimg, img> + <dL_ddepth, depth> + <dL_dalpha, alpha>
 * with depth and alpha as lcgs_render_maps(mode) defines them; any of the three gradients may be NULL, not all three.  For pixel p
 * and on-screen row i, g(p, i) is the gradient of the part of L that belongs to pixel p with respect to the pixel-space mean of i,
 * by the conventions of lcgs_render_backward and lcgs_render_backward_maps: thresholds are constants, the 0.99 cap passes nothing,
 * a saturated pixel stops, the kept frame's background colour is the last layer behind the colour channels and nothing lies behind
 * the map channels.  The channels are summed per pixel FIRST, then the absolute value is taken, then the pixels are summed:
 *     a_i = ( sum_p |g_x(p, i)| , sum_p |g_y(p, i)| ).
 * Two outputs, each nullable, at least one given:
 *   d_absgrad[2 P]: (a_x, a_y) of row i is ADDED at [2 i, 2 i + 1], in pixel units, the context's row order (gsplat's
 *                   means2d.absgrad); rows not on screen are untouched.
 *   stats:          grad_accum[i] += sqrt((a_x W/2)^2 + (a_y H/2)^2), denom[i] += 1, max_radii[i] = max(., reference radius) --
 *                   the last two exactly what lcgs_densify_accumulate does for the same frame (the same code), bit for bit.
 * A caller calls ONE of the two accumulate calls per step and then lcgs_densify unchanged; the threshold is the caller's (AbsGS
 * uses about twice the 3DGS value).
 * State: this context's own kept frame (LCGS_ERR_STATE otherwise; a frame of lcgs_owner_render is refused).  NO preceding backward
 * is needed.  Reads nothing back, only enqueues on the context's stream.  It leaves the frame's 2-D gradient rows and everything
 * else a later backward, lcgs_densify_accumulate or lcgs_camera_backward reads as it was.  A frame that drew nothing returns
 * LCGS_OK and writes nothing.  The sums are binary32 sums of non-negative terms in an UNSPECIFIED order (float atomics across tiles).
 * LCGS_ERR_INVALID_ARG (before any device work): NULL ctx, all three gradients NULL, both outputs NULL, a stats with a NULL member,
 * a mode that is neither constant, num_gaussians not the bound scene's.
 * Not offered: the distortion, normal and feature channels, compact rows, frames of the ownership step, the statistic inside
 * lcgs_fit_views, an lcgs-app flag, the sums fused into the render-backward (a second walk of the lists is what the call costs,
 * on the steps that collect statistics).  Stages under lcgs_set_profiling: absgrad_walk, absgrad_rows. */
LCGS_API lcgs_status lcgs_absgrad_accumulate(lcgs_context* ctx, int num_gaussians, const float* d_dL_dimg, int mode,
                                             const float* d_dL_ddepth, const float* d_dL_dalpha,
                                             const lcgs_densify_stats* stats, float* d_absgrad);
typedef struct lcgs_densify_config {
    float    grad_threshold;  /* 3DGS: 2e-4 */
    float    percent_dense;   /* 3DGS: 0.01 */
    float    scene_extent;
    float    min_opacity;     /* 3DGS: 0.005 */
    int      max_screen_size; /* pixels; 0 = no size pruning */
    uint64_t seed;            /* built-in sampler, used when d_noise is NULL */
} lcgs_densify_config;
/* Out-of-place rewrite of raw / m / v (destinations must not alias sources; out_activated pos / sh may alias out_raw's).  Per
 * source row, binary32: avg = denom ? grad_accum / denom : 0, smax = max exp(raw scale), op = sigmoid(raw opacity);
 * prune = op < min_opacity || (max_screen_size > 0 && (max_radii > max_screen_size || smax > 0.1 scene_extent)) -> no row;
 * else avg < grad_threshold -> the row, bit for bit; else smax <= percent_dense scene_extent -> the row + a copy of raw with
 * zero moments (clone); else two children instead of the row (split): pos + R(q/|q|) (s * n_k), raw scale - ln 1.6, the rest
 * copied, zero moments; n_k = d_noise[i][k][0..2], or (NULL) standard normals of a counter-based generator keyed by
 * (seed, i, k).  Output rows in source order at the prefix sums of the emit counts; out_activated written for all of them;
 * out_stats rows zero; d_src_row[r] (nullable) = source row of output row r.  Synchronises once (the new count).
 * LCGS_ERR_CAPACITY: *new_num_gaussians = rows needed > capacity, no destination touched.  The scene binding is not changed. */
LCGS_API lcgs_status lcgs_densify(lcgs_context* ctx, int num_gaussians, int sh_degree, const lcgs_densify_config* cfg,
                                  const lcgs_densify_stats* stats, const lcgs_params* raw, const lcgs_params* m, const lcgs_params* v,
                                  const lcgs_params* out_raw, const lcgs_params* out_m, const lcgs_params* out_v,
                                  const lcgs_params* out_activated, const lcgs_densify_stats* out_stats, int64_t capacity,
                                  const float* d_noise /* [P][2][3] or NULL */, uint32_t* d_src_row /* [capacity] or NULL */,
                                  int64_t* new_num_gaussians);
/* Contribution-based pruning on the statistics of lcgs_contrib_accumulate.  A row is KEPT iff every enabled test passes:
 * value >= minimum in binary32 (the two weights), unsigned compares (the two counts); a minimum of 0 disables its test, a
 * non-zero minimum whose statistics member is NULL is LCGS_ERR_INVALID_ARG.  (The counts' minimums are 64-bit so that every
 * value of a 32-bit counter can be asked for.) */
typedef struct lcgs_prune_config {
    float    min_weight_max; /* RadSplat: 0.01 */
    float    min_weight_sum;
    uint64_t min_pixels;
    uint64_t min_views;
} lcgs_prune_config;
/* d_keep[i] = 1 kept, 0 dropped; P bytes on the device.  Only enqueues. */
LCGS_API lcgs_status lcgs_contrib_keep_mask(lcgs_context* ctx, int num_gaussians, const lcgs_prune_config* cfg,
                                            const lcgs_contrib_stats* stats, uint8_t* d_keep);
/* lcgs_densify's rewrite with only its prune and keep actions: out of place, in source order; raw / m / v of the kept rows copied
 * bit for bit, out_activated written with the optimiser step's activation expressions; d_src_row[r] (nullable) = source row of
 * output row r -- any other per-row array of the caller is gathered through it.  Synchronises once (the new count).
 * LCGS_ERR_CAPACITY: *new_num_gaussians = rows kept > capacity, no destination touched.  No row kept: LCGS_OK and 0.  The scene
 * binding is not changed. */
LCGS_API lcgs_status lcgs_prune(lcgs_context* ctx, int num_gaussians, int sh_degree, const lcgs_prune_config* cfg,
                                const lcgs_contrib_stats* stats, const lcgs_params* raw, const lcgs_params* m, const lcgs_params* v,
                                const lcgs_params* out_raw, const lcgs_params* out_m, const lcgs_params* out_v,
                                const lcgs_params* out_activated, int64_t capacity, uint32_t* d_src_row, int64_t* new_num_gaussians);
/* raw opacity = min(raw opacity, logit(max_opacity)), its moments zeroed, activated opacity rewritten; only the opacity
 * members of the packs are read.  Only enqueues. */
LCGS_API lcgs_status lcgs_opacity_reset(lcgs_context* ctx, int num_gaussians, float max_opacity /* 3DGS: 0.01 */, const lcgs_params* raw,
                                        const lcgs_params* m, const lcgs_params* v, const lcgs_params* activated);

/* ---- 3DGS-MCMC density control (Kheradmand et al., NeurIPS 2024; no reference counterpart) ------------------- */
/* The other density control in general use: a fixed splat budget and no clone / split thresholds.  Everything is IN PLACE on the
 * caller's raw / m / v / activated arrays (activated pos / sh may alias raw's); none of the calls changes the scene binding --
 * rebind, or call lcgs_scene_modified, before the next frame.
 *   dead        o = 1 / (1 + exp(-raw opacity)) in binary32 (the optimiser step's expression); a row is dead iff !(o > min_opacity):
 *               a NaN opacity is dead, o == min_opacity is dead
 *   weight      w_i = dead ? 0 : (uint32_t)(o * 2^24) -- exact in binary32, a pure function of the row; sums of w in u64 are
 *               exact and order free, so the sampler is reproducible bit for bit anywhere
 *   cdf         cdf_i = w_0 + ... + w_i (u64), T = cdf_{P-1}; the scan works in blocks of 512 rows
 *   draw j      c = Philox4x32-10(key = seed, counter = (j low, j high, tag, 0)); u = c[0] | (uint64_t)c[1] << 32;
 *               t = the high 64 bits of u * T; src_j = the smallest i with cdf_i > t.  tag = 0x4D430001 (relocate), 0x4D430002 (add);
 *               the SGLD normals below use 0x4D430003 -- all unlike lcgs_densify's counters (row low, row high, child 0 | 1, 0)
 *   count       count_i = draws with src_j == i
 *   values      for a source with original raw opacity x and n = min(count + 1, n_max), in BINARY64 from the binary32 inputs,
 *               each result rounded once to binary32:
 *                 o = 1 / (1 + exp(-x)), q = 1 / (1 + exp(x)) (= 1 - o without its rounding), o' = 1 - q^(1/n)
 *                 D = sum_{i=1..n} sum_{k=0..i-1} C(i-1, k) (-1)^k o'^(k+1) / sqrt(k+1)   (i outer, k inner, summed in that order)
 *                 new raw scale = old raw scale + log(o / D) per component (no exp / log round trip)
 *                 o^ = min(max(o', min_opacity), 1 - 2^-23), new raw opacity = log(o^) - log1p(-o^)
 *               liveness: where that binary32 raw opacity is dead by the rule above (o' <= min_opacity was clamped TO min_opacity,
 *               and the rounding fell at or below it), it is replaced by the next binary32 values up until it is live (at most
 *               64 steps; one step at min_opacity = 0.005) -- no row is dead right after a relocation.  gsplat leaves such a row
 *               at min_opacity, to be relocated again the next time.
 *   destination (a dead row, or an appended one) raw pos / rotq / sh of the source bit for bit, the source's new scale and opacity
 *               (computed from its ORIGINAL values), ZERO Adam moments in every group, activated values by the optimiser step's
 *               expressions
 *   source      (count > 0) the same new scale and opacity -- the same bits as its copies --, its Adam moments zeroed in every
 *               group, activated scale and opacity rewritten
 * Zeroing the DESTINATION's moments too departs from gsplat's MCMCStrategy, which leaves a relocated row the moments of the dead
 * splat that used to live there. */
typedef struct lcgs_mcmc_config {
    float    min_opacity; /* 0.005 */
    int      n_max;       /* 1..51; 51 */
    uint64_t seed;        /* built-in sampler, used when d_src_in is NULL */
} lcgs_mcmc_config;
/* Every dead row, in ascending row order (draw j fills the j-th dead row), becomes a copy of a live row.  d_src_in (nullable):
 * [#dead] sources to use instead of the built-in sampler; an entry >= num_gaussians or naming a dead row is
 * LCGS_ERR_INVALID_ARG, found on the device and reported with the count's read-back, nothing of the scene written.  d_src_row
 * (nullable, [P], written whenever the call gets past its argument checks): the source of a relocated row, its own index for
 * every other row.  *num_relocated = rows relocated; no dead row, or no live row (T == 0): 0 and nothing written.
 * Synchronises once (the count). */
LCGS_API lcgs_status lcgs_mcmc_relocate(lcgs_context* ctx, int num_gaussians, int sh_degree, const lcgs_mcmc_config* cfg,
                                        const lcgs_params* raw, const lcgs_params* m, const lcgs_params* v,
                                        const lcgs_params* activated, const uint32_t* d_src_in, uint32_t* d_src_row,
                                        int64_t* num_relocated);
/* Rows [num_gaussians, num_gaussians + num_new) of the caller's arrays (which hold `capacity` rows) become copies of live rows:
 * the same weights, dead rule, draws (tag 0x4D430002) and values as lcgs_mcmc_relocate.  d_src_in (nullable): [num_new] sources;
 * d_src_row (nullable): [num_new], the source of row num_gaussians + j.  num_gaussians + num_new > capacity: LCGS_ERR_CAPACITY,
 * before any device work; num_new == 0: nothing happens; no live row: LCGS_ERR_STATE; a bad entry of d_src_in:
 * LCGS_ERR_INVALID_ARG -- the last two are found on the device: the call reads one status word back (one synchronisation) and
 * has written nothing of the scene when it reports them. */
LCGS_API lcgs_status lcgs_mcmc_add(lcgs_context* ctx, int num_gaussians, int sh_degree, const lcgs_mcmc_config* cfg,
                                   const lcgs_params* raw, const lcgs_params* m, const lcgs_params* v, const lcgs_params* activated,
                                   int64_t num_new, int64_t capacity, const uint32_t* d_src_in, uint32_t* d_src_row);
typedef struct lcgs_mcmc_noise_config {
    float    noise_lr /* 5e5 */, lr_pos /* the step's position learning rate */, k /* 100 */, x0 /* 0.995 */;
    uint64_t seed;
    int      step; /* word 3 of the built-in sampler's counter */
} lcgs_mcmc_noise_config;
/* SGLD noise, binary32, in place on raw pos (and on activated pos when that is another array); moments untouched:
 *   o = 1 / (1 + exp(-raw opacity)), g = 1 / (1 + exp(-k ((1 - o) - x0))), a = (noise_lr * lr_pos) * g
 *   s = exp(raw scale), R = the rotation of rotq / |rotq|, t_j = (sum_r R_rj eps_r) * (s_j * s_j), d_c = sum_j R_cj t_j  (= R S^2 R^T eps)
 *   pos_c += a * d_c
 * eps = d_noise[i][0..2], or (NULL) three standard normals: Box-Muller on Philox4x32-10(seed; row low, row high, 0x4D430003, step)
 * with lcgs_densify's (0, 1) mapping ((x >> 8) + 0.5) / 2^24: (r0 cos t0, r0 sin t0, r1 cos t1), r = sqrt(-2 ln u), t = 2 pi u'.
 * Only enqueues. */
LCGS_API lcgs_status lcgs_mcmc_noise(lcgs_context* ctx, int num_gaussians, const lcgs_mcmc_noise_config* cfg, const lcgs_params* raw,
                                     const lcgs_params* activated, const float* d_noise);
/* grads.d_dL_dopacity[i] += (float)(lambda_opacity / P), grads.d_dL_dscale[i][c] += (float)(lambda_scale / (3 P)), the quotients
 * formed in binary64: the gradients of lambda_opacity mean(o) + lambda_scale mean(s) with respect to the ACTIVATED values, what
 * lcgs_adam_step consumes (3DGS-MCMC: 0.01 each).  Call it between the backward and the optimiser step.  The on-screen-only
 * modes of lcgs_adam_step (visible_only 1 with per-splat rows) apply it to on-screen rows only; compact rows (visible_only 2)
 * are not indexed by splat and must not be passed.  Only the opacity and scale members are read.  Only enqueues. */
LCGS_API lcgs_status lcgs_mcmc_regularize(lcgs_context* ctx, int num_gaussians, float lambda_opacity, float lambda_scale,
                                          const lcgs_grads* grads);

/* ---- Mip-Splatting's 3-D smoothing filter (Yu et al., CVPR 2024; no reference counterpart) -------------------- */
/* The 2-D filter (lcgs_set_raster_mode) fixes zoom-out aliasing; this one stops zoom-in erosion: every splat's size is bounded
 * from below by the highest rate at which any training view sampled it.  Four calls on CALLER-OWNED arrays in the caller's row
 * order (device pointers; the bound scene is not read), all of which only enqueue on the context's stream.  Arithmetic: binary32,
 * round to nearest, nothing contracted, IEEE division and square root; u = 2^-24 below.
 *
 * Training recipe.  (1) Start d_min_z at +inf and max_focal at 0, lcgs_filter3d_accumulate over ALL training views (any number of
 * calls), lcgs_filter3d_finalize -> d_filter; repeat after every density-control rewrite (Mip-Splatting: every 100 iterations).
 * Between recomputations a rewritten scene gathers d_filter through the rewrite's d_src_row.  (2) After every optimiser step,
 * lcgs_filter3d_apply from the optimiser's activated scale / opacity into the arrays bound with lcgs_scene_bind: the frames render
 * the filtered scene.  (3) Between the render backward and lcgs_adam_step, lcgs_filter3d_backward turns the gradients with respect
 * to the filtered values into gradients with respect to the activated ones.  (4) A baked export writes log(scale_out) and
 * logit(opacity_out) through lcgs_ply_write_raw.
 * NOT offered: the filter inside lcgs_render_backward_adam (the fused step goes straight to the raw values); the filter inside
 * lcgs_fit_views or the ownership step (lcgs_owner_step_*); a filter_3D PLY property; an lcgs-app flag.
 *
 * lcgs_filter3d_accumulate.  d_min_z [P] in/out: the caller starts it at +inf, which means "no view has seen the row";
 * *max_focal (host) in/out: the caller starts it at 0.  For every view, cp = the frame's camera constants and
 * v = (right . p + tx, up . p + ty, front . p + tz), each ((a0 p0 + a1 p1) + a2 p2) + t -- the frame's view transform.  The row is
 * SEEN by the view iff  v.z > 0.2f  and  |v.x| <= (1.3f * tanfovx) * v.z  and  |v.y| <= (1.3f * tanfovy) * v.z  (Mip-Splatting's
 * compute_3D_filter: depth beyond 0.2 and inside the screen with a 15 % margin, -0.15 W <= x_pix <= 1.15 W, stated in the tangent
 * plane with the limit the projector clamps to); for a seen row min_z = min(min_z, v.z).  A NaN fails every comparison: such a row
 * is never seen.  *max_focal = max(*max_focal, W / (2 tanfovx)) over the views, on the host (also when num_gaussians is 0).
 * cameras: host array.  Reads nothing back.  Two calls with the views split between them leave what one call with all leaves. */
LCGS_API lcgs_status lcgs_filter3d_accumulate(lcgs_context* ctx, int num_gaussians, const float* d_pos, int num_views,
                                              const lcgs_camera* cameras, float* d_min_z, float* max_focal);
/* d_filter[i] = ((isfinite(d_min_z[i]) ? d_min_z[i] : zmax) / max_focal) * c, zmax = the largest finite entry of d_min_z (a row
 * no view saw gets the coarsest rate of the scene), c = the binary32 nearest to sqrt(0.2) -- Mip-Splatting's filter_3D.  No finite
 * entry: every d_filter[i] = 0, the identity filter.  zmax is found on the device (no read-back); bit-exact whatever the order. */
LCGS_API lcgs_status lcgs_filter3d_finalize(lcgs_context* ctx, int num_gaussians, const float* d_min_z, float max_focal, float* d_filter);
/* Mip-Splatting's get_scaling_with_3D_filter / get_opacity_with_3D_filter from ACTIVATED d_scale [P][3] / d_opacity [P].  Per row,
 * f = d_filter[i]: f == 0 copies the row bit for bit; otherwise f2 = f f, a_k = s_k s_k, b_k = a_k + f2,
 *   scale_out_k = sqrt(b_k),  r_k = a_k / b_k,  coef = sqrt((r_0 r_1) r_2),  opacity_out = opacity * coef.
 * The determinant ratio det(S^2) / det(S^2 + f2 I) is taken as a product of three ratios in [0, 1]: it cannot underflow where
 * prod(s^2) does (scales of 1e-8).  Against exact arithmetic: scale_out within 3 u, opacity_out within 8 u, relative.
 * Out of place: an output that overlaps an input or the other output is LCGS_ERR_INVALID_ARG.  A context whose bound scene is
 * d_scale_out rebuilds its derived rows, as after the library's other writers. */
LCGS_API lcgs_status lcgs_filter3d_apply(lcgs_context* ctx, int num_gaussians, const float* d_scale, const float* d_opacity,
                                         const float* d_filter, float* d_scale_out, float* d_opacity_out);
/* In place: d_dL_dscale / d_dL_dopacity arrive as the gradients with respect to scale_out / opacity_out and leave as those with
 * respect to d_scale / d_opacity (what lcgs_adam_step takes).  f == 0: the row is untouched.  Otherwise, with the forward's coef,
 * b_k and sf_k = scale_out_k re-derived from d_scale / d_filter:
 *   g_op'  = g_op * coef
 *   g_s_k' = g_s_k * (s_k / sf_k) + (((g_op * opacity) * coef) * f2) / (s_k * b_k)
 * within 8 u relative and 16 u (|first term| + |second term|) of exact arithmetic.  d_rows NULL (with d_count): dense rows.
 * Otherwise gradient row r < *d_count (device) belongs to row d_rows[r] of d_scale / d_opacity / d_filter -- the layout of
 * lcgs_render_backward_compact with lcgs_visible_rows; rows beyond the count are untouched, the launch is sized by num_gaussians.
 *
 * All four: LCGS_ERR_INVALID_ARG before any device work for a NULL context or array, a negative count, num_views > 0 with NULL
 * cameras, exactly one of d_rows / d_count NULL, max_focal not finite or <= 0.  num_gaussians == 0 or num_views == 0: LCGS_OK,
 * no array touched (*max_focal untouched for 0 views). */
LCGS_API lcgs_status lcgs_filter3d_backward(lcgs_context* ctx, int num_gaussians, const float* d_scale, const float* d_opacity,
                                            const float* d_filter, const uint32_t* d_rows, const uint32_t* d_count,
                                            float* d_dL_dscale, float* d_dL_dopacity);

/* ---- scene similarity transforms: rotate the SH bands, move, scale, crop (no reference counterpart) ------------ */
/* new = scale * rot * old + trans moves a whole scene: a COLMAP frame onto the axis-aligned volume lcgs_tsdf_integrate fuses into,
 * a second capture into the first one's frame, a scene normalised before training, a region of interest cropped out.  The
 * view-dependent colour rotates with the scene: band l = 1, 2, 3 of the coefficients is multiplied by the rotation's matrix D_l
 * ((2l+1) x (2l+1), orthogonal) in THIS library's basis -- gs_math.hpp's LCGS_SH_TERMS with its signs and constants -- for which
 * B_l(R d) = D_l B_l(d) for every unit direction d, so that sum_k c'_k B_k(R d) = sum_k c_k B_k(d) with c'_l = D_l c_l per
 * colour channel.  A transform that skips this renders highlights that stay nailed to the old axes.
 * Not offered: non-uniform scale (it needs an eigendecomposition per splat) and reflections (they have no quaternion); raw
 * (pre-activation) arrays and optimiser moments -- the second moment has no exact image under a rotation, so a caller who
 * transforms mid-training transforms the activated arrays, recovers the raw ones (log, logit) and resets the moments; an
 * lcgs-app flag (tools/transform_ply.py is the tool); gradients with respect to the transform; the ownership step's sharded
 * scenes (each rank transforms its own rows with the same lcgs_similarity). */
typedef struct lcgs_similarity {
    float rot[9];   /* row-major: new = scale * rot * old + trans */
    float scale;
    float trans[3];
} lcgs_similarity;
typedef struct lcgs_similarity_plan {
    float M[9];     /* row-major, fl32(scale * Rhat) */
    float t[3];
    float s;
    float q[4];     /* (w, x, y, z), the stored order */
    float D1[9], D2[25], D3[49];   /* row-major, D_l[k][j] */
} lcgs_similarity_plan;
/* The plan, host only, no context, entirely in binary64: q = the unit quaternion of rot by Shepperd's method (the largest of the
 * trace and the three diagonal entries picks the component taken by a square root), normalised, w >= 0; Rhat = the matrix rebuilt
 * from q with rot_from_quat's expressions -- EVERYTHING downstream uses Rhat, so positions, orientations and colours see exactly
 * the same rotation; M = scale * Rhat; D_1, D_2, D_3 for Rhat (the basis functions as symmetric tensors, rotated index by index
 * and contracted with the unrotated ones: no solve, nothing sampled; the constants are gs_math.hpp's literals read as binary64).
 * M, q and every D_l entry are rounded to binary32 once (t and s are the caller's values); D64 (nullable, [83]) receives the
 * unrounded D1 then D2 then D3.  LCGS_ERR_INVALID_ARG for a NULL xf or out, a non-finite value, scale <= 0,
 * max |rot rot^T - I| > 1e-4 (an input check, not a measurement: a binary32 rotation composed a few times stays far inside it),
 * det rot <= 0. */
LCGS_API lcgs_status lcgs_similarity_plan_make(const lcgs_similarity* xf, lcgs_similarity_plan* out, double* D64 /* nullable [83] */);
/* The camera that sees the transformed scene as `in` saw the original: position' = scale Rhat position + trans, front' = Rhat
 * front, up' = Rhat up, right' = Rhat right, in binary64 from the plan's Rhat with one rounding; fov, aspect_ratio, width, height
 * copied.  (The frame is the original's up to rounding for scale 1; for another scale up to the projector's 1 / (v.z + 1e-6),
 * which is not scale-invariant: a few 1e-6.)  out may be in.  The plan's refusals, and NULL in / out. */
LCGS_API lcgs_status lcgs_camera_transform(const lcgs_camera* in, const lcgs_similarity* xf, lcgs_camera* out);
/* The ACTIVATED arrays of a scene, in the layouts of lcgs_params (pos [P][3], scale [P][3], rotq [P][4] stored (w, x, y, z),
 * sh [P][(deg+1)^2][3], opacity [P]; device pointers), from `in` to `out`.  Binary32, round to nearest, nothing contracted: every
 * product and every sum is rounded, sums run left to right as written -- one defined bit pattern, the same bits for the same
 * inputs, equal bit for bit to tests/transform_ref.py's restatement.  With the plan of xf:
 *   pos'_i   = ((M[i][0]*x + M[i][1]*y) + M[i][2]*z) + t[i]
 *   scale'_i = s * scale_i
 *   with (W, X, Y, Z) = plan q and (w, x, y, z) = the row's stored quaternion:
 *     w' = ((W*w - X*x) - Y*y) - Z*z      x' = ((W*x + X*w) + Y*z) - Z*y
 *     y' = ((W*y - X*z) + Y*w) + Z*x      z' = ((W*z + X*y) - Y*x) + Z*w
 *   sh'[0][c]    = sh[0][c]                                    (bit copy)
 *   sh'[lo+k][c] = sum over j = 0..2l of D_l[k][j] * sh[lo+j][c], j ascending, the sum started from its first product,
 *                  lo = l*l, for every l <= sh_degree
 *   opacity'     = opacity                                     (bit copy)
 * The quaternion is not renormalised: the product of two unit quaternions is a unit quaternion to rounding, and a caller's
 * non-unit input keeps its norm.  Non-finite values propagate as IEEE arithmetic says (0 * inf = NaN inside a band).
 * Every member pair (in->X, out->X) is the same pointer (in place) or disjoint; partial overlap, and overlap of an output with a
 * different input or another output, is refused (alias).  Each out member may be NULL to skip that array, its in member is then
 * not read: out->pos NULL with out->sh given rotates the colours only.  Only enqueues on the context's stream, reads nothing
 * back, no atomics.  If a written array is one of the context's bound scene arrays, what lcgs_scene_modified does happens:
 * derived rows, the f16 coefficient copy and the kept state of the last frame are dropped (a context-owned scene gets its rows
 * rebuilt behind the transform).  LCGS_ERR_INVALID_ARG before any device work: NULL ctx, xf, in or out; a negative count;
 * sh_degree outside 0..3; an output whose input is NULL; the plan's refusals; alias.  num_gaussians == 0: LCGS_OK, no launch. */
LCGS_API lcgs_status lcgs_scene_transform(lcgs_context* ctx, int num_gaussians, int sh_degree, const lcgs_similarity* xf,
                                          const lcgs_params* in, const lcgs_params* out);
/* The crop: b = pos' by the expression above with the plan of world_to_box; d_keep[i] = 1 iff |b_k| <= half_extent[k] for
 * k = 0, 1, 2, compared in binary32 (a row exactly on a face is kept), else 0; a NaN position is dropped.  The bytes are what
 * lcgs_ply_filter_rows takes after a copy to the host.  Only enqueues.  LCGS_ERR_INVALID_ARG: a NULL pointer, a negative count, a
 * half extent that is negative or NaN (+inf is legal: unbounded on this axis), the plan's refusals. */
LCGS_API lcgs_status lcgs_scene_box_keep_mask(lcgs_context* ctx, int num_gaussians, const float* d_pos,
                                              const lcgs_similarity* world_to_box, const float half_extent[3], uint8_t* d_keep);

/* ---- a scene from a point cloud (no reference counterpart: app/gaussians.cpp only loads trained PLYs) -------- */
/* The mean squared distance to the three nearest neighbours, of n points p_i (binary32, AoS xyz xyz ...):
 *   valid       a point is valid if all three coordinates are finite; an invalid point is nobody's neighbour
 *   d2(i, j)    for valid i and valid j != i (another INDEX: coincident points are each other's neighbours at distance 0):
 *               ((dx dx + dy dy) + dz dz), dx = p_i.x - p_j.x etc., every operation binary32 round-to-nearest, nothing contracted
 *   a <= b <= c the m = min(3, valid others) smallest values of d2(i, .), as a multiset (ties are equal values: harmless)
 *   dist2_i     ((a + b) + c) / 3.0f for m = 3;  (a + b) / 2.0f for m = 2;  a for m = 1;  0.0f for m = 0 or an invalid i
 * The search is EXACT with respect to these computed binary32 values: dist2_i is a pure function of the multiset of points --
 * independent of input order, launch shape, chunking and context; same inputs -> same bits, equal bit for bit to a brute-force
 * binary32 restatement.  (What simple-knn's distCUDA2 computes, made exact and order-independent.) */
#define LCGS_KNN_CHUNK 256 /* sorted points per query workgroup: sizes around its multiples are the kernels' edge cases */
/* d_dist2[i] = dist2_i.  Device pointers; only enqueues.  num_points < 0 or > 2^31 - 1: LCGS_ERR_INVALID_ARG; 0: nothing is touched. */
LCGS_API lcgs_status lcgs_knn_mean_dist2(lcgs_context* ctx, int64_t num_points, const float* d_pos, float* d_dist2);
typedef struct lcgs_init_config {
    float initial_opacity; /* 3DGS: 0.1; must lie in (0, 1) */
    float min_dist2;       /* 3DGS: 1e-7; must be > 0 */
} lcgs_init_config;
/* 3DGS's create_from_pcd.  d_rgb: [n][3] in [0, 1].  Row i of out_raw / out_activated (layouts of lcgs_params; pos / sh of the two
 * packs may alias):
 *   pos          p_i (copied bit for bit)
 *   raw scale    logf(sqrtf(fmaxf(dist2_i, min_dist2))) in all three components;  activated: the optimiser step's exp of it
 *   raw rotq     (1, 0, 0, 0);  activated the same
 *   sh           coefficient 0 = (rgb - 0.5f) / 0.28209479177387814f per channel, every other coefficient of the (deg+1)^2 exactly 0
 *   raw opacity  log(p / (1 - p)), p = (double)initial_opacity, rounded once to binary32 on the host;  activated: the optimiser
 *                step's sigmoid of it
 * Moments are the caller's to zero.  The scene binding is not changed.  Only enqueues. */
LCGS_API lcgs_status lcgs_scene_init_from_points(lcgs_context* ctx, int num_points, int sh_degree, const float* d_pos, const float* d_rgb,
                                                 const lcgs_init_config* cfg, const lcgs_params* out_raw, const lcgs_params* out_activated);
/* 3DGS's getNerfppNorm, host only: center = mean of the camera positions, *radius = 1.1 max |position - center| (binary64 inside,
 * each output rounded once) -- the producer of lcgs_densify_config.scene_extent.  num_cameras >= 1. */
LCGS_API lcgs_status lcgs_scene_extent(int num_cameras, const lcgs_camera* cameras, float center[3], float* radius);
/* Host reader of a point-cloud PLY (binary little-endian or ascii): element vertex with x y z (float or double) and red green blue
 * (uchar -> / 255.0f; or float, taken as is); other properties skipped by their declared size.  malloc'd outputs ([n][3] each),
 * released with lcgs_points_free.  Status codes as lcgs_ply_read (missing file 6, format 7). */
LCGS_API lcgs_status lcgs_points_read_ply(const char* path, int64_t* num_points, float** pos, float** rgb);
LCGS_API void        lcgs_points_free(float* pos, float* rgb);

/* ---- a surface out of the trained scene: TSDF fusion of depth maps, marching tetrahedra (no reference counterpart) - */
/* The last step of 2DGS, GOF, RaDe-GS and PGSR: the rendered depth maps of the training views (lcgs_render_maps, LCGS_DEPTH_Z)
 * are fused into a truncated signed distance volume -- Curless & Levoy's running mean with projective distance and nearest-pixel
 * lookup, what Open3D's fusion does -- and the volume's zero level set is extracted as a welded, indexed, consistently oriented
 * triangle mesh.
 * The volume is the caller's: samples on an nx x ny x nz lattice, sample (i, j, k) at linear index s = (k ny + j) nx + i and at
 * world position X_c = fl(origin_c + fl(voxel_size * (float)i_c)); the caller zeroes d_tsdf and d_weight (and d_rgb) before the
 * first view. */
typedef struct lcgs_tsdf_volume {
    float  origin[3], voxel_size; /* voxel_size finite, > 0 */
    int    nx, ny, nz;            /* each >= 1; nx ny nz <= 2^31 - 1 */
    float *d_tsdf, *d_weight;     /* nx ny nz floats each */
    float *d_rgb;                 /* 3 floats per sample (sample-major), or NULL: no colour */
} lcgs_tsdf_volume;
typedef struct lcgs_tsdf_config {
    float trunc, depth_max, alpha_min; /* each finite and > 0 */
} lcgs_tsdf_config;
/* Integrates num_views views, in call order, into every sample.  Per view the constants are the frame's own (right, up, front,
 * tx, ty, tz, inv_tanx, inv_tany, W, H of the camera); d_depths[v] is W H floats in the library's layout, pixel (x, y) being the
 * ray rx(x), ry(y) of lcgs_normal_consistency_loss_backward (no row flip).  Every operation binary32, uncontracted, `/` one IEEE
 * division.  For sample X and each view:
 *     v_c = fl(fl(fl(r0 X0 + r1 X1) + r2 X2) + t_c) for the rows right / up / front;  z = v_2;  skip unless z > 0 (a NaN skips)
 *     ux = fl(fl(fl(fl(v_0 / z) * inv_tanx) + 1) * fl(0.5f * W)), uy likewise with v_1, inv_tany, H
 *     skip unless 0 <= ux < W and 0 <= uy < H (compared as floats);  px = (int)floorf(ux), py = (int)floorf(uy)
 *     d = depth[py W + px];  with an alpha map: a = alpha[py W + px], skip unless a >= alpha_min, d = fl(d / a)
 *     skip unless d is finite, d > 0, d <= depth_max;  sdf = fl(d - z);  skip if sdf < -trunc;  t = fminf(1.0f, fl(sdf / trunc))
 *     w = weight[s];  tsdf[s] = fl(fl(fl(tsdf[s] * w) + t) / fl(w + 1));  rgb[s][c] likewise from image[c H W + py W + px] where
 *     the volume and the view both have colour;  weight[s] = fl(w + 1)
 * A batch of views leaves the bits the same views leave passed one call at a time, in order.  d_alphas and d_images may be NULL
 * (no view has one) or hold NULL entries.  Only enqueues; needs no kept frame; num_views == 0: LCGS_OK, nothing touched.
 * LCGS_ERR_INVALID_ARG before any device work: a NULL context, volume, config, d_tsdf, d_weight, cameras, d_depths or depth map;
 * a lattice dimension < 1 or more than 2^31 - 1 samples; a voxel size, origin or config value that is not finite, or not > 0 where
 * required; num_views < 0; a camera with width or height < 1; a volume array that overlaps another volume array or an input map. */
#define LCGS_TSDF_VIEW_CHUNK 42 /* views per launch: view counts around its multiples are the kernel's edge cases */
LCGS_API lcgs_status lcgs_tsdf_integrate(lcgs_context* ctx, const lcgs_tsdf_volume* volume, const lcgs_tsdf_config* cfg, int num_views,
                                         const lcgs_camera* cameras, const float* const* d_depths, const float* const* d_alphas,
                                         const float* const* d_images);
/* The mesh, by marching tetrahedra on the 6-tetrahedron Kuhn split: no case table, no ambiguous case, a closed 2-manifold wherever
 * the volume is valid, and vertices welded by rank instead of by sorting or hashing.
 *   cells      cell (i, j, k), i < nx - 1 etc., is VALID iff all 8 corner samples have weight >= weight_min (finite, > 0); a sample is
 *              INSIDE iff tsdf < 0 (neither -0.0f nor a NaN is inside)
 *   split      tetrahedron q = 0 .. 5 of a cell belongs to the q-th permutation (a, b, c) of the axes in lexicographic order:
 *              corners c0 = (0,0,0), c1 = c0 + e_a, c2 = c1 + e_b, c3 = (1,1,1)
 *   edges      a tetrahedron's edge runs from a lower sample lo to lo + dir, dir in {0,1}^3 \ {0}, coded dx + 2 dy + 4 dz; it CROSSES
 *              iff exactly one endpoint is inside; its key is (s_lo, dir), ordered by s_lo, then dir
 *   vertices   one per crossing edge of at least one valid cell, numbered in ascending key order; with a = lo, b = lo + dir:
 *              lambda = fl(t_a / fl(t_a - t_b)), p_c = fl(X_a,c + fl(lambda * fl(X_b,c - X_a,c))); the colour by the same formula
 *   triangles  one corner against three: one triangle; two against two: a quad, split along the diagonal through its lowest vertex
 *              id.  Order: by cell linear index ((k (ny-1) + j) (nx-1) + i), then tetrahedron, then a quad's two triangles by their
 *              other two vertex ids, each pair sorted, compared lexicographically.  Each triangle is wound so that in exact
 *              arithmetic (v1 - v0) x (v2 - v0) points from the inside corners to the outside corners -- decided from the sign
 *              case, not from computed geometry -- and rotated so that its first index is its lowest vertex id.
 * Same inputs, same bits.  lcgs_tsdf_mesh_count reads the two counts back (one synchronisation).  lcgs_tsdf_mesh_extract writes
 * d_vertices (3 floats per vertex), d_vertex_rgb (nullable; needs volume->d_rgb) and d_triangles (3 indices per triangle) and
 * returns the counts; LCGS_ERR_CAPACITY with the needed counts in the two outputs and nothing written when either capacity is
 * too small, or when either count is 2^32 or more.  An empty mesh (any of nx, ny, nz equal to 1 included) is LCGS_OK with zeros.
 * Scratch is the context's: 12 bytes per sample, grown on demand.
 * Not offered: sparse or hashed volumes; weight caps; trilinear depth lookup; median depth; mesh decimation or smoothing; an
 * lcgs-app flag; any gradient. */
LCGS_API lcgs_status lcgs_tsdf_mesh_count(lcgs_context* ctx, const lcgs_tsdf_volume* volume, float weight_min, uint64_t* num_vertices,
                                          uint64_t* num_triangles);
LCGS_API lcgs_status lcgs_tsdf_mesh_extract(lcgs_context* ctx, const lcgs_tsdf_volume* volume, float weight_min, uint64_t cap_vertices,
                                            uint64_t cap_triangles, float* d_vertices, float* d_vertex_rgb, uint32_t* d_triangles,
                                            uint64_t* num_vertices, uint64_t* num_triangles);
/* Host: a binary little-endian PLY of nv vertices (float x y z; with h_rgb also uchar red green blue, clamp(rgb, 0, 1) * 255
 * rounded to nearest) and nt triangular faces (uchar 3, int indices).  LCGS_ERR_IO: the file cannot be opened or written. */
LCGS_API lcgs_status lcgs_mesh_write_ply(const char* path, uint64_t nv, const float* h_vertices, const float* h_rgb, uint64_t nt,
                                         const uint32_t* h_triangles);

/* ---- multi-GPU (no reference counterpart: one device, app/main.cpp:162-163) ------------------------ */
/* One process per GPU, scene replicated, one view per GPU; RCCL is bound at run time (absent: LCGS_ERR_NO_DEVICE). */
typedef struct lcgs_comm lcgs_comm;
typedef struct lcgs_comm_id {
    char bytes[128]; /* an ncclUniqueId: made by ONE rank, carried to the others by the host */
} lcgs_comm_id;
LCGS_API lcgs_status lcgs_comm_unique_id(lcgs_comm_id* out);
/* Collective (ncclCommInitRank).  Attached to ctx (one per context): its dense backward then runs in slices. */
LCGS_API lcgs_status lcgs_comm_create(lcgs_context* ctx, const lcgs_comm_id* id, int rank, int world_size, lcgs_comm** out);
LCGS_API lcgs_status lcgs_comm_destroy(lcgs_comm* comm);
LCGS_API lcgs_status lcgs_comm_info(const lcgs_comm* comm, int* rank, int* world_size);
/* LCGS_TRANSPORT_F32 (default, exact) / LCGS_TRANSPORT_F16 (opt-in: half the bytes, ~sqrt(N) x 5e-4 relative) for lcgs_grads_allreduce */
typedef enum lcgs_transport { LCGS_TRANSPORT_F32 = 0, LCGS_TRANSPORT_F16 = 1 } lcgs_transport;
LCGS_API lcgs_status lcgs_comm_set_transport(lcgs_comm* comm, int transport);
/* Sharded / sparse steps: rank r owns rows [first, first + floor(P / N)); the P mod N tail rows are everybody's. */
LCGS_API void lcgs_comm_shard_rows(int64_t num_gaussians, int world_size, int rank, int64_t* first, int64_t* count);
/* In-place f32 sum over the ranks of the five dense gradient arrays, chunked behind the backward's slices on the
 * communicator's stream; the context's stream waits for it.  EVERY rank calls it once per step with the same
 * num_gaussians / sh_degree / transport (a rank without a view passes zeros), directly behind its backward. */
LCGS_API lcgs_status lcgs_grads_allreduce(lcgs_context* ctx, lcgs_comm* comm, int num_gaussians, int sh_degree, const lcgs_grads* grads);
/* Reduce-scatter -> lcgs_adam_step on the own rows (+ tail) -> all-gather of the ACTIVATED arrays.  Dense (visible_only 0). */
LCGS_API lcgs_status lcgs_adam_step_sharded(lcgs_context* ctx, lcgs_comm* comm, int num_gaussians, int sh_degree,
                                            const lcgs_adam_config* cfg, const lcgs_grads* grads, const lcgs_params* raw,
                                            const lcgs_params* m, const lcgs_params* v, const lcgs_params* activated);
/* Sparse reduce half: only rows the step's views touched travel ((1 + 59) words a row).  track_touched_rows(1) on ALL ranks
 * before the step's first backward; lcgs_adam_step_sparse = the sharded step with that reduce half (one host read-back for
 * the message sizes).  The three stages are exported for a host with its own transport. */
#define LCGS_MAX_RANKS 64
typedef struct lcgs_sparse_rows {
    const uint32_t* d_rows; /* touched rows, ascending (communicator-owned, valid until the next call) */
    int64_t         num_rows;
    int64_t         owner_first[LCGS_MAX_RANKS + 2]; /* rows [owner_first[o], owner_first[o+1]) lie in rank o's shard; [N].. = tail */
} lcgs_sparse_rows;
typedef struct lcgs_comm_stats { /* what the last collective call (or ownership step) moved, per GPU */
    int64_t bytes_sent, bytes_received;
    int64_t touched_rows;      /* sparse step: rows touched; ownership step: rows on this rank's screen */
    int     collective_groups; /* RCCL groups / calls issued: identical on every rank */
} lcgs_comm_stats;
LCGS_API lcgs_status lcgs_comm_track_touched_rows(lcgs_comm* comm, int enable);
LCGS_API lcgs_status lcgs_comm_get_stats(const lcgs_comm* comm, lcgs_comm_stats* out);
LCGS_API lcgs_status lcgs_adam_step_sparse(lcgs_context* ctx, lcgs_comm* comm, int num_gaussians, int sh_degree,
                                           const lcgs_adam_config* cfg, const lcgs_grads* grads, const lcgs_params* raw,
                                           const lcgs_params* m, const lcgs_params* v, const lcgs_params* activated);
/* (touched_rows synchronises and consumes the set; accumulate drops indices outside [row_first, row_first + row_count) unwritten) */
LCGS_API lcgs_status lcgs_sparse_touched_rows(lcgs_context* ctx, lcgs_comm* comm, int num_gaussians, int world_size, lcgs_sparse_rows* out);
LCGS_API int64_t     lcgs_sparse_message_words(int64_t count, int sh_degree);
LCGS_API lcgs_status lcgs_sparse_pack(lcgs_context* ctx, int sh_degree, const lcgs_grads* grads, const uint32_t* d_rows, int64_t count,
                                      float* d_msg);
LCGS_API lcgs_status lcgs_sparse_accumulate(lcgs_context* ctx, int sh_degree, const lcgs_grads* grads, const float* d_msg, int64_t count,
                                            int64_t row_first, int64_t row_count);

/* ---- splat ownership: the frame in two halves ---------------------------------------------------- */
/* An OWNER of rows [row_first, row_first + row_count) runs the per-splat half of a view's frame on them and gets the packed
 * records (12 words: pixel mean 2, conic 3, opacity, rgb 3, depth, pruned rect 2 x u32) of the rows on that view's screen with
 * their global row indices, ascending; the view's RENDERER runs the rest on the rows of all owners concatenated in owner
 * order (same image as lcgs_render_forward, bit for bit) and returns 12-word 2-D gradient rows; the owner maps them to
 * parameter gradients at its rows.  slot < LCGS_MAX_OWNER_VIEWS: the view's index inside the step.
 * project: d_rows[row_count], d_records[row_count x 12] (16-byte aligned); num_rows = rows written (synchronises), NULL:
 * enqueue only and read all slots' counts with ONE synchronisation through lcgs_owner_counts.
 * backward: accumulate 0 clears the range first, 1 adds the rows. */
#define LCGS_MAX_OWNER_VIEWS 16
#define LCGS_OWNER_RECORD_FLOATS 12
#define LCGS_OWNER_GRAD_FLOATS 12
LCGS_API lcgs_status lcgs_owner_project(lcgs_context* ctx, int slot, const lcgs_camera* camera, float scale_modifier, int row_first,
                                        int row_count, int keep_state, uint32_t* d_rows, float* d_records, int* num_rows);
/* The N views of a step over ONE row range in one call (view k -> slot first_slot + k; d_rows / d_records: host arrays of N
 * device pointers): N independent pipelines run side by side and are joined on the context's stream; enqueue only. */
LCGS_API lcgs_status lcgs_owner_project_views(lcgs_context* ctx, int first_slot, int num_views, const lcgs_camera* cameras,
                                              float scale_modifier, int row_first, int row_count, int keep_state,
                                              uint32_t* const* d_rows, float* const* d_records);
LCGS_API lcgs_status lcgs_owner_counts(lcgs_context* ctx, int first_slot, int num_slots, int* num_rows);
LCGS_API lcgs_status lcgs_owner_render(lcgs_context* ctx, const lcgs_camera* camera, const float bg_color[3], int num_rows,
                                       const uint32_t* d_rows, const float* d_records, float* d_img, int keep_state);
LCGS_API lcgs_status lcgs_owner_render_backward(lcgs_context* ctx, const float* d_dL_dimg, float* d_grads2d);
LCGS_API lcgs_status lcgs_owner_backward(lcgs_context* ctx, int slot, const float* d_grads2d, const lcgs_grads* grads, int accumulate);
/* The step WITH its transport (RCCL send / recv on the communicator's stream): rank r owns lcgs_comm_owner_rows(P, N, r)
 * (equal shards, tail with the last rank) and renders cameras[r] (cameras: world_size entries).  Every rank calls forward
 * then backward once per step; gradients land at the own rows of `grads` (other rows untouched); lcgs_comm_get_stats has
 * the step's bytes. */
LCGS_API void        lcgs_comm_owner_rows(int64_t num_gaussians, int world_size, int rank, int64_t* first, int64_t* count);
LCGS_API lcgs_status lcgs_owner_step_forward(lcgs_context* ctx, lcgs_comm* comm, const lcgs_camera* cameras, const float bg_color[3],
                                             float scale_modifier, float* d_img);
LCGS_API lcgs_status lcgs_owner_step_backward(lcgs_context* ctx, lcgs_comm* comm, const float* d_dL_dimg, const lcgs_grads* grads);
/* Opt-in (every rank alike): from the second step on NOTHING is read back -- messages are sized from the previous step's
 * all-gathered counts (n + n/4 + 1024 rows), counts and the pair-buffer verdict stay on the device.  Such a step MUST be
 * closed with lcgs_owner_step_finish before its gradients are used: it waits for the forward half's max-reduced verdict
 * only; *redo = 1 on EVERY rank if ANY rank's message was clipped / frame truncated: call forward + backward again. */
LCGS_API lcgs_status lcgs_owner_step_set_async(lcgs_comm* comm, int enable);
LCGS_API lcgs_status lcgs_owner_step_finish(lcgs_context* ctx, lcgs_comm* comm, int* redo);
/* A collective self-test: 1 KB all-reduce; a zero- and a one-byte message to every peer in one group; an ownership step on a
 * 10 000-splat scratch scene (image = the fused frame bit for bit, gradients 1e-4).  Each phase against timeout_s; a phase
 * that never returns is reported (timed_out) and the process should exit.  The context's scene binding is put back. */
typedef struct lcgs_comm_selftest_report {
    int    world_size, rank;
    int    allreduce_ok;
    double allreduce_ms;
    int    p2p_ok;
    double p2p_ms;
    int    owner_step_ok; /* 1 right, 0 wrong, -1 not run (N > LCGS_MAX_OWNER_VIEWS) */
    double owner_step_ms;
    double owner_max_grad_err;
    int    timed_out; /* 0, or the phase (1..3) that did not finish */
    char   message[256];
} lcgs_comm_selftest_report;
LCGS_API lcgs_status lcgs_comm_selftest(lcgs_context* ctx, lcgs_comm* comm, double timeout_s, lcgs_comm_selftest_report* out);
/* In-process stand-in for RCCL (tests, single-GPU rehearsals): N communicators for N contexts ON ONE DEVICE, one host
 * thread each; every collective of this header runs the same code over device copies.  Not a production transport. */
typedef struct lcgs_loopback_group lcgs_loopback_group;
LCGS_API lcgs_status lcgs_loopback_group_create(int world_size, lcgs_loopback_group** out);
LCGS_API lcgs_status lcgs_loopback_group_destroy(lcgs_loopback_group* group); /* after its communicators */
LCGS_API lcgs_status lcgs_comm_create_loopback(lcgs_context* ctx, lcgs_loopback_group* group, int rank, lcgs_comm** out);

/* ---- scene ingest / image egress (host side of render(ply, camera) -> image) ------------------------------------ */
/* GaussiansData (app/gaussians.h:15-35) after read_gs_ply: activated host arrays.  Free with lcgs_scene_host_free. */
typedef struct lcgs_scene_host {
    int    num_gaussians;
    int    sh_degree; /* 3 */
    float* pos;       /* 3P */
    float* feature;   /* P*16*3, [j*48 + k*3 + c] */
    float* opacity;   /* P, sigmoid applied */
    float* scale;     /* 3P, exp applied */
    float* rotq;      /* 4P, (r,x,y,z) normalised */
} lcgs_scene_host;
/* read_gs_ply (app/gaussians.cpp:75-171): binary-LE or ascii PLY, properties by name, others ignored. */
LCGS_API lcgs_status lcgs_ply_read(const char* path, lcgs_scene_host* out);
/* Raw (un-activated) values, INRIA property order, nx ny nz = 0 (f_dc 3P, f_rest 45P channel-major): writes the stand-ins. */
LCGS_API lcgs_status lcgs_ply_write_raw(const char* path, int num_gaussians, const float* pos, const float* f_dc, const float* f_rest,
                                        const float* opacity_logit, const float* log_scale, const float* rot);
/* A pruned file for a viewer: the vertex records of a binary little-endian PLY whose keep byte is non-zero, copied bit for bit
 * in order behind the same header with the new vertex count (no activation is undone, so no bits change).  LCGS_ERR_IO: a file
 * cannot be opened; LCGS_ERR_FORMAT: an ascii file, a vertex count other than num_rows, elements after `vertex`, a truncated
 * payload. */
LCGS_API lcgs_status lcgs_ply_filter_rows(const char* in_path, const char* out_path, int64_t num_rows, const uint8_t* keep);
LCGS_API void lcgs_scene_host_free(lcgs_scene_host* scene);
/* Deterministic stand-ins for the BASELINE scenes: kind 0 object-like, 1 unbounded-like; counter-based RNG
 * (any sub-range independently); ACTIVATED arrays, caller-allocated (count * {3, 48, 1, 3, 4} floats). */
LCGS_API lcgs_status lcgs_synth_scene(int kind, uint64_t seed, int64_t first, int64_t count, float* pos, float* feature, float* opacity,
                                      float* scale, float* rotq);
/* app/main.cpp:323-335: CHW float -> HWC uint8, vertical flip, truncating *255 (host / device variants). */
LCGS_API void        lcgs_image_to_rgb8(int width, int height, const float* h_img_chw, uint8_t* h_rgb);
LCGS_API lcgs_status lcgs_image_to_rgb8_device(lcgs_context* ctx, int width, int height, const float* d_img_chw, uint8_t* d_rgb);
/* stbi_write_png(name, w, h, 3, data, 0) (app/main.cpp:339): 8-bit RGB PNG. */
LCGS_API lcgs_status lcgs_write_png(const char* path, int width, int height, const uint8_t* h_rgb);

#ifdef __cplusplus
}
#endif
#endif /* LCGS_HIP_H */
