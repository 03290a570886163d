// comm_owner.cpp -- lcgs_owner_step_forward / _backward / _finish and the row ranges the owners hold.
// ---------------------------------------------------------------------------------------------------------------------
// The splat-ownership step with its transport (the device halves are abi_owner.cpp's).  What travels: per
// view v, from every owner o to rank v, the rows of o's range that reach v's screen -- [row index u32] + [48-byte packed
// record] -- and back, from rank v to every owner, the 48-byte 2-D gradient row of each of them.  Sizes are agreed through
// ONE small all-gather (the N counts of every owner) and one read-back: the step's only host synchronisation besides the
// view's own pair-buffer check.  Point-to-point over RCCL (ncclSend / ncclRecv in one group per direction); the same code
// runs over the in-process loopback with N contexts on one device.
// ---------------------------------------------------------------------------------------------------------------------
#include "comm_internal.hpp"

using namespace lcgs;

namespace
{
// bytes of one message row
constexpr size_t kRecBytes = LCGS_OWNER_RECORD_FLOATS * 4, kG2dBytes = LCGS_OWNER_GRAD_FLOATS * 4;

// rows every owner holds (lcgs_comm_owner_rows' counts), once per step
void owner_counts(int64_t P, int N, int64_t* oc)
{
    for (int o = 0; o < N; ++o) lcgs_comm_owner_rows(P, N, o, nullptr, &oc[o]);
}

// One array of a message: where my rows lie, where the peers' rows land, bytes per row.
struct RowLane {
    const char* out;
    char*       in;
    size_t      bytes;
};
// ONE grouped exchange of rows with every peer, the only place that lays messages out: to rank o the n_out[o] rows at row
// off_out[o] of every lane's `out`, from rank o n_in[o] rows to row off_in[o] of its `in`; lane by lane, sends before
// receives.  EVERY rank must pass a table that mirrors its peers' (ncclSend / ncclRecv sizes have to match).  My own share
// stays on the device: copied in front of the group, so that nothing but RCCL calls sits inside it (n_in[me] == n_out[me];
// the test hook self_p2p sends it through the wire instead).  alias: nothing moves (one rank whose view reads its own rows
// where they lie) -- the group is still opened and closed.  Hands back to the context's stream; adds the bytes to the stats.
lcgs_status exchange_rows(lcgs_comm* c, Wire& wire, const RowLane* lanes, int n_lanes, const int64_t* n_out, const int64_t* off_out,
                          const int64_t* n_in, const int64_t* off_in, bool alias)
{
    const int N = c->world, me = c->rank;
    if (!alias && !c->self_p2p && n_in[me] > 0)
        for (const RowLane* l = lanes; l < lanes + n_lanes; ++l)
            LCGS_HIP_CHECK(hipMemcpyAsync(l->in + (size_t)off_in[me] * l->bytes, l->out + (size_t)off_out[me] * l->bytes,
                                          (size_t)n_in[me] * l->bytes, hipMemcpyDeviceToDevice, c->stream));
    LCGS_TRY(wire.group_begin());
    for (int o = 0; o < N && !alias; ++o) {
        if (o == me && !c->self_p2p) continue;
        for (const RowLane* l = lanes; n_out[o] > 0 && l < lanes + n_lanes; ++l) {
            LCGS_TRY(wire.send(l->out + (size_t)off_out[o] * l->bytes, (size_t)n_out[o] * l->bytes, o));
            c->stats.bytes_sent += n_out[o] * (int64_t)l->bytes;
        }
        for (const RowLane* l = lanes; n_in[o] > 0 && l < lanes + n_lanes; ++l) {
            LCGS_TRY(wire.recv(l->in + (size_t)off_in[o] * l->bytes, (size_t)n_in[o] * l->bytes, o));
            c->stats.bytes_received += n_in[o] * (int64_t)l->bytes;
        }
    }
    LCGS_TRY(wire.group_end());
    return c->comm_to_compute();
}

// The forward's exchange: [row index u32] + [48-byte record] of my rows on view o's screen (n_out[o], in own_rows / own_recs
// at o * count) to rank o, owner o's rows on my screen (n_in[o]) to own.in_off[o] of in_rows / in_recs.  The sizes' table
// (one all-gather in front of this) is counted here too.
lcgs_status exchange_records(lcgs_comm* c, Wire& wire, int64_t count, const int64_t* n_in, const int64_t* n_out, bool alias)
{
    const int N = c->world;
    if (!alias) {
        LCGS_TRY(c->in_rows.ensure((size_t)c->own.in_off[N] * 4 + 16));
        LCGS_TRY(c->in_recs.ensure((size_t)c->own.in_off[N] * kRecBytes + 16));
    }
    const RowLane lanes[2] = { { c->own_rows.as<char>(), c->in_rows.as<char>(), 4 },
                               { c->own_recs.as<char>(), c->in_recs.as<char>(), kRecBytes } };
    int64_t       off_out[LCGS_MAX_RANKS];
    for (int o = 0; o < N; ++o) off_out[o] = (int64_t)o * count;
    c->stats.bytes_sent = c->stats.bytes_received = (int64_t)(N - 1) * N * 4;
    return exchange_rows(c, wire, lanes, 2, n_out, off_out, n_in, c->own.in_off, alias);
}
} // namespace

extern "C" {

void lcgs_comm_owner_rows(int64_t num_gaussians, int world_size, int rank, int64_t* first, int64_t* count)
{
    // equal contiguous shards of floor(P / N) rows, the P mod N tail with the last rank (multi_gpu.owner_range)
    const int64_t c = world_size > 0 ? num_gaussians / world_size : num_gaussians;
    if (first) *first = c * rank;
    if (count) *count = rank < world_size - 1 ? c : num_gaussians - c * rank;
}

static_assert(LCGS_MAX_OWNER_VIEWS <= lcgs::kMaxOwnerSegs, "OwnerSegs holds one segment per view slot");
// rows a padded message from an owner of `owner_count` rows holds when it carried n rows in the last step
static int64_t padded_rows(int64_t n, int64_t owner_count) { return std::min(owner_count, n + n / 4 + 1024); }

lcgs_status lcgs_owner_step_set_async(lcgs_comm* c, int enable)
{
    LCGS_REQUIRE(c != nullptr, "comm is NULL");
    c->owner_async = enable != 0;
    return LCGS_OK;
}

lcgs_status lcgs_owner_step_forward(lcgs_context* ctx, lcgs_comm* c, const lcgs_camera* cameras, const float bg_color[3],
                                    float scale_modifier, float* d_img)
{
    LCGS_REQUIRE(ctx && c && cameras && bg_color && d_img, "NULL argument");
    LCGS_REQUIRE(c->ctx == ctx, "the communicator belongs to another (or a destroyed) context");
    LCGS_REQUIRE(c->world <= LCGS_MAX_OWNER_VIEWS, "world_size above LCGS_MAX_OWNER_VIEWS (one view slot per rank)");
    LCGS_ENTRY(ctx);
    LCGS_REQUIRE(ctx->pos != nullptr && ctx->P > 0, "no scene bound");
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    const int N = c->world, me = c->rank;
    int64_t   first = 0, count = 0, oc[LCGS_MAX_RANKS];
    lcgs_comm_owner_rows(ctx->P, N, me, &first, &count);
    owner_counts(ctx->P, N, oc);
    c->own.valid = false; // (kept as it is: a step without read-back that was never finished is not noticed here)
    c->own.async = false;
    c->stats     = lcgs_comm_stats{};
    Wire      wire{ c };
    LoopGuard guard{ c };

    // ---- 1. my rows, every view of the step (view v = rank v's): N asynchronous projections, side by side
    LCGS_TRY(c->own_rows.ensure((size_t)N * (size_t)count * 4 + 16));
    LCGS_TRY(c->own_recs.ensure((size_t)N * (size_t)count * kRecBytes + 16));
    {
        uint32_t* rows_v[LCGS_MAX_OWNER_VIEWS];
        float*    recs_v[LCGS_MAX_OWNER_VIEWS];
        for (int v = 0; v < N; ++v) {
            rows_v[v] = c->own_rows.as<uint32_t>() + (size_t)v * count;
            recs_v[v] = c->own_recs.as<float>() + (size_t)v * count * LCGS_OWNER_RECORD_FLOATS;
        }
        // (the N pipelines side by side on the context's lanes, joined on its stream: abi_owner.cpp)
        LCGS_TRY(lcgs_owner_project_views(ctx, 0, N, cameras, scale_modifier, (int)first, (int)count, /*keep_state=*/1, rows_v, recs_v));
    }
    // ---- 2. everybody learns everybody's counts: table[o][v] = rows of owner o on view v's screen
    LCGS_TRY(c->bounds.ensure((size_t)(N + 2) * 4));
    LCGS_TRY(c->matrix.ensure((size_t)N * N * 4));
    LCGS_TRY(c->ensure_h_matrix());
    LCGS_HIP_CHECK(hipMemsetAsync(c->bounds.ptr, 0, (size_t)N * 4, ctx->stream));
    for (int v = 0; v < N; ++v)
        if (ctx->owner[v].valid && ctx->owner[v].row_count > 0)
            LCGS_HIP_CHECK(hipMemcpyAsync(c->bounds.as<uint32_t>() + v, ctx->owner[v].counts.ptr, 4, hipMemcpyDeviceToDevice, ctx->stream));

    // The step WITHOUT a read-back (lcgs_owner_step_set_async): possible once a previous step's table is known, for the
    // same scene and world, and while the padded segments of my view fit the workspace the scene sizes
    bool    async = c->owner_async && !c->force_sync_once && c->prev.have && c->prev.world == N && c->prev.P == ctx->P;
    int64_t cap_total = 0;
    if (async) {
        for (int o = 0; o < N; ++o) {
            c->own.cap_in[o]  = padded_rows(c->prev.table[(size_t)o * N + me], oc[o]);
            c->own.in_off[o]  = cap_total;
            cap_total += c->own.cap_in[o];
            c->own.cap_out[o] = padded_rows(c->prev.table[(size_t)me * N + o], count);
        }
        c->own.in_off[N] = cap_total;
        // EVERY rank must take the same branch (the branches size their messages differently): the test runs over every
        // view's padded segments, computed from the table all ranks share -- not over this rank's own column alone
        for (int v = 0; v < N && async; ++v) {
            int64_t total_v = 0;
            for (int o = 0; o < N; ++o) total_v += padded_rows(c->prev.table[(size_t)o * N + v], oc[o]);
            if (total_v > ctx->P || total_v >= (int64_t)0x7FFFFFFF) async = false;
        }
    }
    c->force_sync_once = false;

    if (async) {
        LCGS_TRY(c->h_next.ensure(((size_t)LCGS_MAX_RANKS * LCGS_MAX_RANKS + 4) * 4));
        LCGS_TRY(c->ev_checked.ensure());
        LCGS_TRY(c->flag_dev.ensure(16));
        LCGS_HIP_CHECK(hipMemsetAsync(c->flag_dev.ptr, 0, 16, ctx->stream));
        LCGS_TRY(c->compute_to_comm());
        LCGS_TRY(wire.allgather_u32(c->bounds.as<uint32_t>(), c->matrix.as<uint32_t>(), (size_t)N));
        // (for lcgs_owner_step_finish and the next step's sizes: nobody waits for this copy here)
        LCGS_HIP_CHECK(hipMemcpyAsync(c->h_next, c->matrix.ptr, (size_t)N * N * 4, hipMemcpyDeviceToHost, c->stream));
        // ---- 3'. padded messages: sizes from the last step's table, true counts on the device
        const bool alias = N == 1 && !c->self_p2p; // one rank: my view reads my own projection where it lies
        LCGS_TRY(exchange_records(c, wire, count, c->own.cap_in, c->own.cap_out, alias)); // (cap_in[me] == cap_out[me])
        c->stats.touched_rows      = cap_total; // (the capacity: the row count itself is on the device)
        c->stats.collective_groups = 3;         // the counts, the records, the flag
        c->own.n_all               = cap_total;
        for (int v = 0; v < N; ++v) {
            c->own.out[v] = (uint32_t)c->own.cap_out[v];
            if (ctx->owner[v].valid && ctx->owner[v].row_count > 0) ctx->owner[v].num = (int)c->own.cap_out[v]; // (a launch bound)
        }
        // ---- 4'. my view from everybody's rows: no read-back, the verdicts go into the flag word
        abi::OwnerAsyncFrame af;
        af.segs.n = (uint32_t)N;
        for (int o = 0; o <= N; ++o) af.segs.off[o] = (uint32_t)c->own.in_off[o];
        af.table    = c->matrix.as<uint32_t>();
        af.view     = (uint32_t)me;
        af.overflow = c->flag_dev.as<uint32_t>();
        const uint32_t* rows_v = alias ? c->own_rows.as<uint32_t>() : c->in_rows.as<uint32_t>();
        const float*    recs_v = alias ? c->own_recs.as<float>() : c->in_recs.as<float>();
        if (cap_total > 0)
            LCGS_TRY(abi::owner_render_frame(ctx, &cameras[me], bg_color, (int)cap_total, rows_v, recs_v, d_img, /*keep_state=*/1, &af));
        // ---- 5'. one verdict for everybody: the flag, max-reduced; with the table it reaches pinned memory behind ev_checked
        LCGS_TRY(c->compute_to_comm());
        LCGS_TRY(wire.allreduce_max_u32(c->flag_dev.as<uint32_t>(), 1));
        LCGS_HIP_CHECK(hipMemcpyAsync(c->h_next + (size_t)N * N, c->flag_dev.ptr, 4, hipMemcpyDeviceToHost, c->stream));
        LCGS_HIP_CHECK(hipEventRecord(c->ev_checked, c->stream)); // (no hand-back: lcgs_owner_step_finish waits for it on the host)
        c->own.valid = true;
        c->own.async = true;
        guard.ok     = true;
        return LCGS_OK;
    }

    LCGS_TRY(c->compute_to_comm());
    LCGS_TRY(wire.allgather_u32(c->bounds.as<uint32_t>(), c->matrix.as<uint32_t>(), (size_t)N));
    LCGS_HIP_CHECK(hipMemcpyAsync(c->h_matrix, c->matrix.ptr, (size_t)N * N * 4, hipMemcpyDeviceToHost, c->stream));
    LCGS_HIP_CHECK(hipStreamSynchronize(c->stream)); // the step's one host synchronisation for message sizes
    auto table = [&](int o, int v) -> int64_t { return (int64_t)c->h_matrix[o * N + v]; };
    int64_t n_all = 0, n_in[LCGS_MAX_RANKS], n_out[LCGS_MAX_RANKS];
    for (int o = 0; o < N; ++o) {
        for (int v = 0; v < N; ++v) LCGS_REQUIRE(table(o, v) <= oc[o], "an owner reports more on-screen rows than it owns");
        c->own.in_off[o] = n_all;
        n_all += n_in[o] = table(o, me);
    }
    c->own.in_off[N] = n_all;
    for (int v = 0; v < N; ++v) {
        c->own.out[v] = (uint32_t)(n_out[v] = table(me, v));
        if (ctx->owner[v].valid && ctx->owner[v].row_count > 0) ctx->owner[v].num = (int)table(me, v);
    }
    // (what the next step sizes its padded messages from, if it runs without a read-back)
    c->prev.table.assign(c->h_matrix + 0, c->h_matrix + (size_t)N * N);
    c->prev.have = true, c->prev.world = N, c->prev.P = ctx->P;
    // ---- 3. the records travel: mine to every view's rank, every owner's to me (owner order = ascending rows)
    LCGS_TRY(exchange_records(c, wire, count, n_in, n_out, /*alias=*/false));
    c->stats.touched_rows      = n_all; // rows on this rank's screen
    c->stats.collective_groups = 2;     // the counts, the records
    c->own.n_all               = n_all;
    // ---- 4. my view from everybody's rows
    LCGS_TRY(lcgs_owner_render(ctx, &cameras[me], bg_color, (int)n_all, c->in_rows.as<uint32_t>(), c->in_recs.as<float>(), d_img,
                               /*keep_state=*/1));
    c->own.valid = true;
    guard.ok     = true;
    return LCGS_OK;
}

lcgs_status lcgs_owner_step_backward(lcgs_context* ctx, lcgs_comm* c, const float* d_dL_dimg, const lcgs_grads* grads)
{
    LCGS_REQUIRE(ctx && c && d_dL_dimg && grads, "NULL argument");
    LCGS_REQUIRE(c->ctx == ctx, "the communicator belongs to another (or a destroyed) context");
    if (!c->own.valid) {
        set_last_error("lcgs_owner_step_backward needs a preceding lcgs_owner_step_forward");
        return LCGS_ERR_STATE;
    }
    LCGS_ENTRY(ctx);
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    const int     N = c->world, me = c->rank;
    const int64_t n_all = c->own.n_all; // (a step without read-back: the padded segments' total capacity)
    const bool    alias = c->own.async && N == 1 && !c->self_p2p;
    c->own.valid        = false;
    Wire      wire{ c };
    LoopGuard guard{ c };
    // ---- 1. my view's 2-D gradients, one 48-byte row per received row (owner order; padded segments keep their positions)
    int64_t first = 0, count = 0;
    lcgs_comm_owner_rows(ctx->P, N, me, &first, &count);
    // (a step without read-back: the per-splat kernel of step 3 walks a view's TRUE row count, which a clipped message falls
    // short of -- the step is then repeated, but until the verdict is read nothing may be read out of bounds: every view's
    // rows get room for my whole range)
    LCGS_TRY(c->g2d_all.ensure((size_t)std::max(n_all, alias ? count : (int64_t)0) * kG2dBytes + 16));
    // (the own rows of the dense gradient arrays are cleared as a side job of the render-backward: view 0 then ADDS like the rest)
    DenseFill  fill;
    const bool filled = n_all > 0 && count > 0 && grads->d_dL_dpos && grads->d_dL_dscale && grads->d_dL_drotq && grads->d_dL_dsh &&
                        grads->d_dL_dopacity &&
                        abi::dense_fill_rows(abi::rows_from(*grads, ctx->sh_deg, (size_t)first), ctx->sh_deg, (size_t)count, &fill);
    if (n_all > 0) LCGS_TRY(abi::owner_render_backward_into(ctx, d_dL_dimg, c->g2d_all.as<float>(), filled ? &fill : nullptr));
    // ---- 2. every owner gets its rows' share back; I get my rows' share of every view
    int64_t gin_off[LCGS_MAX_RANKS + 1], n_out[LCGS_MAX_RANKS], n_in[LCGS_MAX_RANKS], total_in = 0;
    for (int v = 0; v < N; ++v) {
        gin_off[v] = total_in;
        total_in += c->own.async ? count : (int64_t)c->own.out[v];
        n_out[v] = c->own.in_off[v + 1] - c->own.in_off[v]; // owner v's rows on my screen: their gradients go back
        n_in[v]  = c->own.out[v];                           // my rows on view v's screen: their gradients come in
    }
    if (!alias) LCGS_TRY(c->g_in.ensure((size_t)total_in * kG2dBytes + 16));
    const float* g_in = alias ? c->g2d_all.as<float>() : c->g_in.as<float>();
    LCGS_TRY(c->compute_to_comm());
    const RowLane lane = { c->g2d_all.as<char>(), c->g_in.as<char>(), kG2dBytes };
    LCGS_TRY(exchange_rows(c, wire, &lane, 1, n_out, c->own.in_off, n_in, gin_off, alias));
    c->stats.collective_groups += 1;
    // ---- 3. my rows: the 2-D gradients of every view -> parameter gradients, summed in view order
    for (int v = 0; v < N; ++v)
        LCGS_TRY(abi::owner_backward_rows(ctx, v, g_in + (size_t)gin_off[v] * LCGS_OWNER_GRAD_FLOATS, grads, v > 0 ? 1 : (filled ? 2 : 0)));
    guard.ok = true;
    return LCGS_OK;
}

lcgs_status lcgs_owner_step_finish(lcgs_context* ctx, lcgs_comm* c, int* redo)
{
    LCGS_REQUIRE(ctx && c && redo, "NULL argument");
    LCGS_REQUIRE(c->ctx == ctx, "the communicator belongs to another (or a destroyed) context");
    *redo = 0;
    LCGS_ENTRY(ctx);
    if (!c->own.async) return LCGS_OK; // a step that read its sizes back has nothing left to report
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    c->own.async = false;
    // waits for the FORWARD half of the step at most (the flag's reduction sits behind every rank's frame, in front of the
    // backward's messages on the communicator's stream): by now the device is normally far into the backward
    LCGS_HIP_CHECK(hipEventSynchronize(c->ev_checked));
    const int N = c->world, me = c->rank;
    c->prev.table.assign(c->h_next + 0, c->h_next + (size_t)N * N);
    c->prev.have = true, c->prev.world = N, c->prev.P = ctx->P;
    abi::owner_frame_settle(ctx);
    int64_t rows = 0;
    for (int o = 0; o < N; ++o) rows += std::min<int64_t>(c->h_next[(size_t)o * N + me], c->own.cap_in[o]);
    c->stats.touched_rows = rows; // rows on this rank's screen
    if (c->h_next[(size_t)N * N] != 0u) { // somebody's message was clipped, or somebody's frame truncated: everybody redoes
        *redo              = 1;
        c->force_sync_once = true; // (the redo reads its sizes back: exact, and the frame grows its own buffers)
    }
    return LCGS_OK;
}

} // extern "C"
