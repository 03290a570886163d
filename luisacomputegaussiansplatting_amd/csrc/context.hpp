// context.hpp -- the (opaque to callers) lcgs_context, shared by the translation units behind the C ABI
// (abi_*.cpp: frames, scene, optimiser -- see abi_internal.hpp; host/comm_*.cpp: the RCCL gradient collectives).
#pragma once

#include <atomic>

#include "common.hpp"
#include "kernels/launch.hpp"

struct lcgs_comm;

namespace lcgs
{
constexpr int kMaxEvents    = LCGS_MAX_STAGES + 1;
constexpr int kMaxGradSlices = 16; // splat-range slices of the dense gradient rows (chunked all-reduce)
// (host/comm_wire.cpp) a context that goes away before its communicator: the communicator forgets it
void comm_forget_context(lcgs_comm* comm);
// (host/comm_grads.cpp) sparse exchange: a dense backward flags the rows of the frame it has just differentiated
lcgs_status comm_mark_touched(lcgs_comm* comm, const KeptRows& rows, bool accumulate, hipStream_t stream);
namespace abi
{
// (abi_scene.cpp) position / scale / rotation rows inside these arrays are being written: every live context drops the rows
// it derived from them (the cull pass's {position, extent bound} rows)
void scene_arrays_written(lcgs_context* ctx, const float* pos, const float* scale, const float* rotq);
} // namespace abi
} // namespace lcgs

using lcgs::CamParams;
using lcgs::DeviceBuffer;
using lcgs::Event;
using lcgs::Pinned;
using lcgs::Stream;

struct lcgs_context {
    int         device = 0;
    hipStream_t stream = nullptr;

    // scene (lcgs_scene_bind / lcgs_scene_upload)
    int          P = 0, sh_deg = 3;
    const float *pos = nullptr, *scale = nullptr, *rotq = nullptr, *sh = nullptr, *opacity = nullptr;
    DeviceBuffer owned[5];
    // Splat order of a context-owned scene: lcgs_scene_load_ply re-orders along a Morton curve unless told otherwise
    // (lcgs_set_ingest_order); scene_perm[r] = file index of splat r while perm_valid (lcgs_scene_permutation)
    int          lod_min_radius = 0; // lcgs_set_lod: opt-in footprint cull of the fused frame (0 = off)
    int          raster_mode = 0;    // lcgs_set_raster_mode: LCGS_RASTER_CLASSIC, or the opacity-compensated frame (a kept frame remembers its own: last.cp)
    int          ingest_order = 1; // LCGS_ORDER_SPATIAL
    DeviceBuffer scene_perm;
    bool         perm_valid = false;      // the BOUND arrays are owned[] in the order scene_perm describes
    bool         perm_for_owned = false;  // scene_perm describes the current contents of owned[] (bound or not)
    DeviceBuffer sh_half;            // opt-in f16 copy of sh for the fused forward's colour pass (lcgs_scene_use_half_sh)
    bool         use_half_sh = false;
    // {position, extent bound} rows of a scene the context OWNS (abi_scene.cpp refresh_cull_bound): the cull pass's phase 1
    // reads these 16 bytes instead of 40 bytes of position + scale + rotation.  cull_bound is what frames use -- the
    // context's own buffer, a sibling's borrowed pointer, or NULL (caller-bound arrays, or owned arrays the library has
    // written since: lcgs_adam_step & co. drop it; binding the owned arrays again rebuilds it)
    DeviceBuffer          cull_bound_buf;
    DeviceBuffer          verify_ws; // lcgs_debug_verify_derived: one counter
    const float4*         cull_bound = nullptr;
    // ... valid for exactly these arrays (the context's own, or caller arrays declared static: lcgs_scene_declare_static);
    // a frame uses the rows only when its position / scale / rotation arrays are these (cull_rows())
    struct {
        const float *pos = nullptr, *scale = nullptr, *rotq = nullptr;
        int          P = 0;
    } cull_key;
    // THREADING: a context (with its batch sibling) is used by one host thread at a time; the only cross-thread traffic is
    // this word.  Another thread's writer (an optimiser step through ITS context on arrays this one renders, or its
    // lcgs_scene_modified) never touches this context's fields: it compares against the copy of the keys this context
    // PUBLISHED under the registry mutex (abi_scene.cpp) and posts bits here; the owning thread honours them at its next
    // use -- kRowsStale at once (cull_rows() below; cleared when the rows are rebuilt), kSceneModified in
    // frame_state_valid() / note_foreign_writes().
    static constexpr uint32_t kRowsStale = 1u, kSceneModified = 2u;
    std::atomic<uint32_t>     foreign_writes{ 0 };
    const float4* cull_rows() const
    {
        if (foreign_writes.load(std::memory_order_acquire) & kRowsStale) return nullptr;
        return (cull_bound && pos == cull_key.pos && scale == cull_key.scale && rotq == cull_key.rotq && P == cull_key.P)
                   ? cull_bound
                   : nullptr;
    }
    // another thread declared the bound arrays modified: the f16 coefficient copy and the last frame's kept state are stale
    void note_foreign_writes()
    {
        if (foreign_writes.load(std::memory_order_acquire) & kSceneModified) {
            foreign_writes.fetch_and(~kSceneModified, std::memory_order_acq_rel);
            use_half_sh = false;
            last.valid  = false;
        }
    }
    bool frame_state_valid()
    {
        note_foreign_writes();
        return last.valid;
    }

    // workspace of the fused frame
    DeviceBuffer cull_slab, chunk_info, chunk_base; // the cull pass's per-chunk output (fused_forward.hip k_cull_compact)
    DeviceBuffer recs, sortk[2], sortv[2], vis_index, rects, rects_sorted, pairk[2], pairv[3], zero_ws[3], counts, sort_ws,
        expand_ws, final_T, n_contrib, grads2d, strip_masks, shjac, tie_ws, fused_grads, bwd_counter;
    bool         last_has_jac = false; // the last keep_state frame stored the colour Jacobian (degree 3)
    // zero_ws holds what a frame needs zeroed: the tile ranges.  Three
    // copies rotate: while frame N runs, the auxiliary stream clears the copy of frame N + 2.  Two frames ahead, not
    // one, so that no wait is needed when a frame starts: the fill issued during frame N - 1 sits on the auxiliary
    // stream in front of frame N's record builder, whose completion frame N's renderer waited for -- and frame N + 1
    // starts behind that renderer.
    size_t    zero_bytes      = 0;
    int       zero_cur        = 0;
    bool      zero_ready[3]   = { false, false, false };
    uint32_t* ranges          = nullptr; // tile ranges of the last frame (inside zero_ws[...])
    // device-resident per-call parameters + the captured frame graph (replayed while its key is unchanged)
    DeviceBuffer   frame_params;
    hipGraphExec_t graph_exec = nullptr;
    struct GraphKey {
        const void *pos = nullptr, *scale = nullptr, *rotq = nullptr, *sh = nullptr, *opacity = nullptr, *sh_half = nullptr,
                   *img = nullptr, *radii = nullptr, *cull_bound = nullptr;
        int         P = -1, sh_deg = -1, width = 0, height = 0, keep_state = -1, list_shift = -1;
        int64_t     hint_V = -1, hint_L = -1;
        uint32_t    capacity = 0;
        hipStream_t stream = nullptr;
        bool        operator==(const GraphKey& o) const
        {
            return pos == o.pos && scale == o.scale && rotq == o.rotq && sh == o.sh && opacity == o.opacity &&
                   sh_half == o.sh_half && img == o.img && radii == o.radii && cull_bound == o.cull_bound && P == o.P && sh_deg == o.sh_deg && width == o.width &&
                   height == o.height && keep_state == o.keep_state && list_shift == o.list_shift && hint_V == o.hint_V && hint_L == o.hint_L &&
                   capacity == o.capacity && stream == o.stream;
        }
    } graph_key;
    // Longest-list-first tile schedule: a scheduling hint, so a frame uses the order derived from the PREVIOUS
    // frame's list lengths (computed on the auxiliary stream while that frame rendered); only the first frame of a
    // resolution computes its own order in line.
    DeviceBuffer tile_order[2];
    int          order_cur = 0;  // tile_order[order_cur] is the newest complete order ...
    uint32_t     order_G   = 0;  // ... valid for this many tiles (0: none yet)
    uint32_t*    last_tile_order = nullptr; // the order the last frame rendered with (reused by the backward)
    // Persistent renderers (render.hip / backward.hip PERSIST): a bounded grid of `k x CUs` workgroups that pull tiles from a
    // counter, instead of one workgroup per tile.  Used while SEVERAL frames are in flight (camera batches, lcgs_fit_views):
    // the cap leaves wave slots, registers and LDS free on every CU, so the other frame's short sort-chain kernels start at
    // once instead of queueing behind thousands of pending tile workgroups.  0 = one workgroup per tile (in-order frames).
    int       num_cus = 0;
    int       persist_in_flight = 0;   // k while several frames are in flight (lcgs_render_forward_batch / lcgs_fit_views)
    int       persist_forced = -1;     // tuning hook LCGS_RENDER_WGS_PER_CU: k for EVERY frame when >= 0
    int       persist_bwd_in_flight = 0, persist_bwd_forced = -1; // the same for the render-backward (LCGS_BWD_WGS_PER_CU)
    bool      frames_in_flight = false; // set around the calls of a batch
    uint32_t* work_counters = nullptr; // [0] forward renderer, [1] render-backward: inside the frame's zeroed block
    bool use_graph = false; // opt-in (LCGS_GRAPH=1): measured no gain on MI355X, the short kernels are GPU-latency-bound
    // second stream: work that is independent of the sort chain (record building; gradient zero-fill) overlaps it
    Stream      aux_stream; // (the batch sibling's: borrowed, its parent's cull_stream)
    Event       ev_fork, ev_join, ev_ranges, ev_aux_done, ev_render, ev_counts;
    bool        aux_pending = false, counts_pending = false;
    hipEvent_t  aux_done_last = nullptr; // whichever of ev_aux_done / ev_pipe_aux[] the auxiliary stream recorded last
    // Pipelined in-order frames (abi_frame.cpp enqueue_forward): forward-only, enqueue-only frames run their head
    // -- cull, depth sort, expand, tile partition, ranges -- on head_stream, beside the PREVIOUS frame's renderer; the renderers
    // stay on the caller's stream in call order.  What renderer k reads survives head k + 1: the records alternate between
    // recs and recs_b, the final pair list is the one of pairv[0..2] the next head leaves alone, the renderer's two counter
    // words travel in the frame's zeroed block, and the auxiliary job that recycles frame k - 1's zeroed block and tile
    // schedule waits for renderer k - 1.  Events a LATER call waits for exist once per frame parity (a re-recorded event
    // names its latest record only).
    Stream      head_stream;
    Event       ev_pipe_entry;     // the caller's stream at entry (frames that do not chain)
    Event       ev_pipe_render[2]; // renderer of the last pipelined frame of that parity
    Event       ev_pipe_aux[2];    // ... and its auxiliary job (next schedule, cleared block)
    DeviceBuffer recs_b;                                 // the records of odd pipelined frames
    // A frame that CHAINS runs its cull pass one slot ahead, on cull_stream beside the previous head's sort chain: the pass reads
    // the call's camera and the context's own scene (which nothing writes while frames chain) and writes the chunk slabs,
    // chunk_info and cull_counts, whose last readers are the previous head's k_rowscan_first / k_scatter_first -- it waits for
    // that scatter (ev_fork) and for nothing else; the head waits for ev_cull in front of its k_rowscan_first.  Only while the
    // GPU is behind the host (the query that gates the bounded grid): a paced frame has nothing to run beside and would only
    // pay for the cross-stream waits.  The stream has the auxiliary stream's lowest priority and is ALSO the auxiliary stream
    // of the batch sibling (which borrows it): the two uses never coincide, and the process stays at four streams -- a fifth
    // shares a hardware queue with the caller's stream and costs the camera batch 12 % (profiles/early_cull_ab.txt).
    Stream      cull_stream;
    Event       ev_cull;
    DeviceBuffer cull_counts; // the cull pass's counts[digit][chunk], apart from sort_ws (which the previous head's passes still use)
    bool        early_cull  = true; // LCGS_EARLY_CULL=0: a chained frame's cull pass stays on the head stream (A/B and test hook)
    uint64_t    pipe_early  = 0;    // frames that culled early (lcgs_debug_early_cull_count)
    bool        pipeline    = true; // LCGS_PIPELINE=0: every frame in today's order (A/B and test hook)
    uint32_t    pipe_frames = 0;    // pipelined frames so far: the parity
    uint64_t    pipe_chained = 0, pipe_bounded = 0; // ... those that chained / rendered with the bounded grid (lcgs_debug_pipeline_counts)
    // the renderer of a frame that chains is a bounded persistent grid of this many workgroups per CU (see persist_in_flight):
    // measured on the bicycle stand-in at 1080p, frames/s with 2 / 3 / 4 / 6 per CU and one workgroup per tile:
    // 1513 / 1619 / 1459 / 1357 and 1428, against 1445 in single-stream order (profiles/pipelined_frames_ab.txt)
    int         pipe_render_wgs = 3;
    // every C ABI entry point counts itself; a pipelined frame notes the count it left, so the next one knows whether anything
    // else was asked of the context in between (then its head first waits for the caller's stream, which is today's order)
    uint64_t    op_seq = 0, pipe_left_seq = ~(uint64_t)0;
    // keep_state frames clear the 2-D gradient rows on the auxiliary stream (beside the renderer) so that the backward
    // does not start with a 40 us zero-fill; consumed by the first backward of that frame
    bool        g2d_zeroed  = false;
    // a backward has run on the last keep-state frame: until then its 2-D gradient rows are only zeros (lcgs_densify_accumulate)
    bool        g2d_backward_done = false;
    // ... and the depth mode of the backward that wrote their value slot (kG2DValueSlot), -1: none did (lcgs_camera_backward)
    int         g2d_value_mode = -1;
    // ... and whether it passed a normal gradient: the camera gradient lacks that channel's direct term (lcgs_camera_backward refuses)
    bool        g2d_normal_channel = false;
    // lcgs_render_normals / lcgs_render_backward_normals: the on-screen rows' normals and dL/dn (splat_normals_bytes each)
    DeviceBuffer splat_normals, splat_normal_grads;
    // lcgs_render_features / lcgs_render_backward_features: measurement hook LCGS_FEATURES_CH (4, 8, 16: that chunk width for every K)
    int         features_ch_forced = 0;
    DeviceBuffer cam_slab; // lcgs_camera_backward: per-block partial sums (camera_grad_slab_bytes)
    DeviceBuffer contrib_slab; // lcgs_contrib_accumulate: {sum, max bits, count} per on-screen row (contrib_slab_bytes)
    DeviceBuffer absgrad_ws;   // lcgs_absgrad_accumulate: (sum |g_x|, sum |g_y|) per on-screen row (absgrad_ws_bytes)
    // lcgs_densify: emit counts, their inclusive sums, actions (one entry per source row)
    DeviceBuffer dn_emit, dn_incl, dn_action;
    // lcgs_mcmc_relocate / lcgs_mcmc_add (abi_mcmc.cpp): per row the weight, the dead flag, its inclusive sums, the u64 sums of
    // the weights and the draws that landed on the row; per draw the dead row it fills and its source; the u64 scan's block
    // sums; one status word (kernels/launch.hpp launch_mcmc_draw)
    DeviceBuffer mc_w, mc_dead, mc_dead_incl, mc_cdf, mc_count, mc_dead_list, mc_draw, mc_status;
    // lcgs_filter3d_finalize (abi_filter3d.cpp): the word its reduction leaves the largest finite min_z in
    DeviceBuffer f3_word;
    // lcgs_tsdf_mesh_count / _extract (abi_tsdf.cpp): per sample the edge-mask / triangle-count word, the vertex counts and the
    // triangle counts (scanned in place); the scan's block sums; the two u64 totals
    DeviceBuffer ts_word, ts_vcount, ts_tcount, ts_scan_temp, ts_totals;
    // lcgs_knn_mean_dist2 / lcgs_scene_init_from_points (abi_init.cpp): Morton keys and original indices (the sort's ping-pong),
    // the sort's workspace, the sorted points, the per-chunk boxes, the box partials + grid, the init call's dist2
    DeviceBuffer knn_keys[2], knn_vals[2], knn_sort_ws, knn_sorted, knn_boxes, knn_grid, knn_dist2;
    // lcgs_render_forward_batch: a sibling context (own workspace, own streams) that renders every other view, so
    // that one view's latency-bound sort chain overlaps the other's bandwidth- and VALU-bound kernels
    lcgs_context* twin         = nullptr;
    Event         ev_batch_fork, ev_batch_join;
    // lcgs_fit_views: the view's image and loss gradient (per context: two views are in flight), the order of the
    // backward passes across the two contexts
    DeviceBuffer fit_img, fit_dL;
    // lcgs_photometric_loss_backward: per-workgroup partial sums, then the planes a, b, c (loss.hip); the loss lcgs_fit_views
    // applies (lcgs_set_fit_loss; handed to the sibling in prepare_twin)
    // (lcgs_normal_consistency_loss_backward: its per-workgroup partial sums)
    // (lcgs_depth_prior_loss_backward: the tiles' and groups' sums and the groups' coefficients, kernels/launch.hpp)
    // (lcgs_bilagrid_backward: the row slices' partial sums of dL/dgrid; lcgs_bilagrid_tv_loss_backward: per-workgroup partials)
    DeviceBuffer loss_ws;
    int          fit_loss   = LCGS_LOSS_L2;
    float        fit_lambda = 0.2f;
    Event        ev_fit_bwd;
    // launch-size hints from the last synchronised frame (live counts stay on the device; larger counts are
    // still handled correctly by chunk striding)
    int64_t hint_V = 0, hint_L = 0, hint_Lb = 0; // (hint_L: frames with per-tile lists; hint_Lb: per 2 x 2-tile block)
    // workspace of the stage-level path / primitives
    DeviceBuffer st_keys_tmp, st_vals_tmp, st_sort_temp, st_scan_temp, st_scalar;
    DeviceBuffer st_flags, st_u32[8], st_keys_exp, st_vals_exp; // the splatter's sort-before-duplicate (lcgs_tile_splat_forward)
    DeviceBuffer st_win, st_win2, st_offs; // ... and the output-balanced pair copies' window table (one word per 1024 pairs) and offsets
    uint32_t     pair_capacity = 0;
    Pinned<uint32_t> h_counts;            // 16 x u32
    Pinned<uint32_t> h_stage;             // 4 x u32, coherent and mapped: the stage-level splatter's one read-back (num_rendered & co.)
    uint32_t*    h_stage_dev   = nullptr; // the same words as the device sees them (posted by the compaction's scan launch)

    // state of the last forward (for backward and stats)
    struct {
        bool      valid = false;
        bool      has_state = false;
        CamParams cp;
        float     bg[3];
        float     scale_modifier;
        int       list_buf = 0; // pairv[list_buf] holds the sorted per-tile lists (dense ids)
    } last;
    lcgs_frame_stats stats{};

    // Chunked gradient all-reduce (host/comm_grads.cpp).  With a communicator attached, the dense backward splits its
    // preprocess pass into `grad_slices` splat-range slices and records an event behind each; lcgs_grads_allreduce
    // starts reducing a slice's rows when its event fires, while the later slices are still being computed.
    lcgs_comm*   comm = nullptr;        // attached by lcgs_comm_create (not owned)
    int          grad_slices = 1;       // > 1: slice the dense preprocess-backward
    DeviceBuffer slice_bounds;          // (grad_slices + 1) x u32, dense-id boundaries of the slices (device)
    Event        ev_slice[lcgs::kMaxGradSlices];
    int          slices_recorded = 0;   // slices of the last dense backward whose events are valid (0: not sliced)
    const void*  slices_of = nullptr;   // the dL_dpos array those events belong to

    // Stage-level operators in DEFERRED mode (lcgs_set_stage_mode): SHProcessor::process and GSProjector::forward record
    // their arguments instead of running; a GSTileSplatter::forward whose inputs are exactly their outputs then renders
    // the fused frame from the 3-D arrays (same image, radii, num_rendered); anything else runs the recorded calls first.
    int stage_mode = 0; // LCGS_STAGES_EXACT
    uint32_t stage_serial = 0;   // lcgs_tile_splat_forward's per-frame mark of the "unwritten pair slots" word
    bool stage_side_copy = true; // the unsorted pair buffers' copy beside the depth sort (A/B hook LCGS_STAGE_SIDE_COPY=0)
    // Frames that keep no backward state may list their pairs per block of 2 x 2 tiles (CamParams::list_shift; frames that
    // keep it never do: that was built in round 6 and lost 1.1 % on forward+backward, REJECTED.md).  It pays from
    // ~3 M per-tile pairs up (-2 % at 0.2-0.9 M, 0 at 2.5 M, +2.5 % at 4-8 M, +6 % at 10 M, +15 % at 17 M: profiles/
    // r05_coarse_lists_ab.txt), so the default decides per context from the last synchronised frame's pair count, with hysteresis;
    // LCGS_COARSE_LISTS=0 / 1 force it off / on (A/B and test hook).
    int  coarse_mode     = 2;     // 0 never, 1 always, 2 by the pair count
    bool coarse_on       = false; // (mode 2) the current decision
    double coarse_yield  = 0.6;   // pruned per-tile pairs / reference num_rendered, from this context's last per-tile frame
    bool bwd_use_masks   = true; // the render-backward walks the forward's kept strip bits (test hook LCGS_BWD_USE_MASKS=0: it repeats the strip tests)
    bool stage_mailbox   = true; // the splatter's scalars posted to pinned memory and polled (A/B hook LCGS_STAGE_MAILBOX=0: copy + sync)
    int stage_sort = 0; // lcgs_tile_splat_forward's sort route: 0 = by frame size, 1 = literal six passes, 2 = sort-before-duplicate
                        // (LCGS_STAGE_SORT=literal|splats, read once when the context is created)
    struct {
        bool         pending = false;
        int          num = 0, level = 3;
        const float *pos = nullptr, *sh = nullptr;
        float*       color = nullptr;
        lcgs_camera  cam{};
    } def_sh;
    struct {
        bool         pending = false;
        int          num = 0, use_focal = 1;
        const float *pos = nullptr, *scale = nullptr, *rotq = nullptr;
        float        scale_modifier = 1.0f;
        float *      means = nullptr, *covs = nullptr, *depth = nullptr;
        lcgs_camera  cam{};
    } def_proj;

    // Splat ownership (abi_owner.cpp): per view of a step, what this context computed as an OWNER of a row range
    // (kept for that view's backward), and -- as the RENDERER of a view -- the received records the last frame was drawn from
    struct OwnerSlot {
        bool         valid = false, has_jac = false;
        CamParams    cp;
        float        scale_modifier = 1.0f;
        int          row_first = 0, row_count = 0, num = 0;
        DeviceBuffer vis, shjac, counts;
    } owner[LCGS_MAX_OWNER_VIEWS];
    Pinned<uint32_t>         h_owner_counts; // LCGS_MAX_OWNER_VIEWS words (lcgs_owner_counts)
    // lcgs_owner_project_views: the N views of a step are N INDEPENDENT short pipelines over the rank's P / N rows (five launches
    // of a few hundred workgroups each); they run side by side on kOwnerLanes streams at most (two by default), each lane with its own scratch of
    // the cull / first-sort-pass stages (sized by the row range), joined on the context's stream at the end of the call
    static constexpr int kOwnerLanes = 4;
    struct OwnerLane {
        DeviceBuffer slab, chunk_info, chunk_base, sortk[2], sortv[2], rects, sort_ws;
        Stream       stream;
        Event        done;
    } owner_lane[kOwnerLanes];
    Event                    ev_owner_fork;
    const lcgs::SplatRecord* owner_recs = nullptr;
    int                      owner_rows = 0;

    // per-stage timing
    bool             profiling = false;
    Event            events[lcgs::kMaxEvents]; // (the timing kind, made by the first mark that records them)
    int              n_marks        = 0;
    const char*      mark_names[lcgs::kMaxEvents]{};
    lcgs_stage_times times{};
};

