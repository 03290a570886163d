// comm_grads.cpp -- the three dense-gradient steps of a communicator: the chunked all-reduce, the sharded Adam step and the
// sparse exchange (touched rows to their owners) with the helpers they share.
#include "comm_internal.hpp"

using namespace lcgs;

namespace
{
// lcgs_adam_step on the rank's own rows [first, first + count) and on the tail rows every rank keeps (fewer than N)
lcgs_status adam_own_rows(lcgs_context* ctx, lcgs_comm* c, int64_t P, int sh_degree, const lcgs_adam_config* cfg,
                          const lcgs_grads* g, const lcgs_params* raw, const lcgs_params* m, const lcgs_params* v,
                          const lcgs_params* activated)
{
    int64_t first = 0, count = 0;
    lcgs_comm_shard_rows(P, c->world, c->rank, &first, &count);
    const int64_t tail0 = count * c->world, tail = P - tail0;
    auto sub = [&](const lcgs_params* p, int64_t row) { return abi::rows_from(*p, sh_degree, (size_t)row); };
    auto step_rows = [&](int64_t row, int64_t rows) -> lcgs_status {
        if (rows <= 0) return LCGS_OK;
        const lcgs_grads  gg = abi::rows_from(*g, sh_degree, (size_t)row);
        const lcgs_params r_ = sub(raw, row), m_ = sub(m, row), v_ = sub(v, row), a_ = sub(activated, row);
        return lcgs_adam_step(ctx, (int)rows, sh_degree, cfg, &gg, &r_, &m_, &v_, &a_);
    };
    LCGS_TRY(step_rows(first, count));
    return step_rows(tail0, tail);
}

// all-gather of the refreshed ACTIVATED rows (what every rank's renderer reads).  Raw parameters and moments stay
// authoritative on their owner only (plus the tail everywhere).
lcgs_status allgather_activated(lcgs_context* ctx, lcgs_comm* c, int64_t P, int sh_degree, const AttrRows& act)
{
    int64_t first = 0, count = 0;
    lcgs_comm_shard_rows(P, c->world, c->rank, &first, &count);
    // the other ranks' rows land in these arrays: whatever a context derived from them (the cull pass's 16-byte rows) is
    // stale from here on -- also on a rank whose own shard is empty and whose lcgs_adam_step therefore wrote nothing
    abi::scene_arrays_written(ctx, act.ptr[0], act.ptr[1], act.ptr[2]);
    LCGS_TRY(c->compute_to_comm());
    if (count > 0) {
        Wire wire{ c };
        LCGS_TRY(wire.group_begin());
        for (int i = 0; i < 5; ++i)
            LCGS_TRY(wire.allgather(act.ptr[i] + (size_t)first * act.width[i], act.ptr[i], (size_t)count * act.width[i]));
        LCGS_TRY(wire.group_end());
        c->stats.collective_groups += 1;
        const int64_t b = (int64_t)((uint64_t)(c->world - 1) * (uint64_t)count * act.row_bytes());
        c->stats.bytes_sent += b;
        c->stats.bytes_received += b;
    }
    LCGS_TRY(c->comm_to_compute());
    return LCGS_OK;
}
} // namespace

extern "C" {

void lcgs_comm_shard_rows(int64_t num_gaussians, int world_size, int rank, int64_t* first, int64_t* count)
{
    // equal shards of floor(P / N) rows; the P mod N rows behind them ("the tail") belong to every rank
    const int64_t c = world_size > 0 ? num_gaussians / world_size : num_gaussians;
    if (first) *first = c * rank;
    if (count) *count = c;
}

lcgs_status lcgs_grads_allreduce(lcgs_context* ctx, lcgs_comm* c, int num_gaussians, int sh_degree,
                                 const lcgs_grads* grads)
{
    LCGS_REQUIRE(ctx && c && grads, "NULL argument");
    LCGS_REQUIRE(c->ctx == ctx, "the communicator belongs to another (or a destroyed) context");
    LCGS_REQUIRE(c->loop == nullptr || c->transport == LCGS_TRANSPORT_F32, "the in-process (loopback) transport moves f32 only");
    LCGS_REQUIRE(num_gaussians >= 0 && sh_degree >= 0 && sh_degree <= 3, "bad num_gaussians / sh_degree");
    LCGS_REQUIRE(grads->d_dL_dpos && grads->d_dL_dscale && grads->d_dL_drotq && grads->d_dL_dsh && grads->d_dL_dopacity,
                 "NULL gradient buffer");
    if (num_gaussians == 0) return LCGS_OK;
    LCGS_ENTRY(ctx);
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    const AttrRows a = attr_rows(grads, sh_degree);
    const int64_t  P = num_gaussians;
    c->stats = lcgs_comm_stats{}; // "what the LAST collective call moved": reset on every path
    if (c->transport == LCGS_TRANSPORT_F16) {
        // Opt-in: the sum crosses the wire as f16 with one power-of-two scale per attribute, agreed by all ranks (the
        // magnitudes are max-reduced first).  One chunk behind the backward's tail: the scales need every row.
        // (kept as it is: this path calls rccl() itself and has no LoopGuard -- the loopback is refused above)
        size_t total = 0, start[5]; // (halfs; every attribute's region starts 16-byte aligned: vector stores on that side)
        for (int i = 0; i < 5; ++i) {
            start[i] = total;
            total += ((size_t)P * a.width[i] + 7) & ~(size_t)7;
        }
        const void* had = c->packed.ptr;
        LCGS_TRY(c->packed.ensure(total * 2));
        if (c->packed.ptr != had) LCGS_HIP_CHECK(hipMemsetAsync(c->packed.ptr, 0, total * 2, c->stream)); // the padding is summed too
        LCGS_TRY(c->scales.ensure(16 * sizeof(float)));
        float*    amax  = c->scales.as<float>();
        float*    scale = amax + 5;
        float*    inv   = amax + 10;
        uint16_t* pk    = c->packed.as<uint16_t>();
        LCGS_TRY(c->compute_to_comm());
        ctx->slices_recorded = 0;
        LCGS_HIP_CHECK(hipMemsetAsync(amax, 0, 5 * sizeof(float), c->stream));
        for (int i = 0; i < 5; ++i) launch_absmax(a.ptr[i], (size_t)P * a.width[i], reinterpret_cast<uint32_t*>(amax + i), c->stream);
        LCGS_RCCL_CHECK(rccl().AllReduce(amax, amax, 5, ncclFloat32, ncclMax, c->comm, c->stream));
        launch_transport_scales(amax, c->world, scale, inv, c->stream);
        for (int i = 0; i < 5; ++i) launch_pack_f16(a.ptr[i], (size_t)P * a.width[i], scale + i, pk + start[i], c->stream);
        LCGS_RCCL_CHECK(rccl().AllReduce(pk, pk, total, ncclFloat16, ncclSum, c->comm, c->stream));
        for (int i = 0; i < 5; ++i) launch_unpack_f16(pk + start[i], (size_t)P * a.width[i], inv + i, a.ptr[i], c->stream);
        LCGS_HIP_CHECK(hipGetLastError());
        LCGS_TRY(c->comm_to_compute());
        c->stats.collective_groups = 2; // the magnitudes, the packed sum
        c->stats.bytes_sent = c->stats.bytes_received =
            (int64_t)(2 * (uint64_t)(c->world - 1) * ((uint64_t)total * 2 + 5 * 4) / (uint64_t)c->world);
        return LCGS_OK;
    }
    // The NUMBER and the row ranges of the chunks come from values every rank shares (P, the slice count set when the
    // communicator was created) -- never from what this rank happened to do before the call: a rank without a view in
    // the last round of a batch, or with an empty frame, has run no backward and must still issue the very same
    // sequence of collectives as its peers (RCCL: mismatched counts are undefined behaviour).  Only what a chunk WAITS
    // for is local: the event of the backward slice that produced its rows when those events belong to these arrays,
    // else the tail of the context's stream.
    const int  K         = (ctx->grad_slices > 1 && P >= 4096) ? ctx->grad_slices : 1; // (render_backward's own rule)
    const bool by_slice  = K > 1 && ctx->slices_recorded == K && ctx->slices_of == (const void*)grads->d_dL_dpos &&
                          ctx->P == num_gaussians;
    LCGS_HIP_CHECK(hipEventRecord(c->ev_in, ctx->stream));
    if (!by_slice) LCGS_HIP_CHECK(hipStreamWaitEvent(c->stream, c->ev_in, 0));
    Wire      wire{ c };
    LoopGuard guard{ c };
    for (int k = 0; k < K; ++k) {
        if (by_slice) LCGS_HIP_CHECK(hipStreamWaitEvent(c->stream, ctx->ev_slice[k], 0));
        // the last chunk also waits for whatever was enqueued on the context's stream behind the backward
        if (by_slice && k == K - 1) LCGS_HIP_CHECK(hipStreamWaitEvent(c->stream, c->ev_in, 0));
        const int64_t r0 = (int64_t)(((uint64_t)P * (uint64_t)k) / (uint64_t)K);       // (k_slice_bounds' split)
        const int64_t r1 = (int64_t)(((uint64_t)P * (uint64_t)(k + 1)) / (uint64_t)K);
        if (r1 <= r0) continue;
        LCGS_TRY(wire.group_begin());
        for (int i = 0; i < 5; ++i) LCGS_TRY(wire.allreduce_sum(a.ptr[i] + (size_t)r0 * a.width[i], (size_t)(r1 - r0) * a.width[i]));
        LCGS_TRY(wire.group_end());
        c->stats.collective_groups += 1;
    }
    c->stats.bytes_sent = c->stats.bytes_received =
        (int64_t)(2 * (uint64_t)(c->world - 1) * (uint64_t)P * a.row_bytes() / (uint64_t)c->world);
    ctx->slices_recorded = 0; // consumed
    // whatever the caller enqueues next on the context's stream (the optimiser) sees the sums
    LCGS_TRY(c->comm_to_compute());
    guard.ok = true;
    return LCGS_OK;
}

lcgs_status lcgs_adam_step_sharded(lcgs_context* ctx, lcgs_comm* c, int num_gaussians, int sh_degree,
                                   const lcgs_adam_config* cfg, const lcgs_grads* grads, const lcgs_params* raw,
                                   const lcgs_params* m, const lcgs_params* v, const lcgs_params* activated)
{
    LCGS_REQUIRE(ctx && c && cfg && grads && raw && m && v && activated, "NULL argument");
    LCGS_REQUIRE(c->ctx == ctx, "the communicator belongs to another context");
    LCGS_REQUIRE(c->loop == nullptr || c->transport == LCGS_TRANSPORT_F32, "the in-process (loopback) transport moves f32 only");
    LCGS_REQUIRE(cfg->visible_only == 0, "the sharded step is dense (per-splat rows): visible_only must be 0");
    LCGS_REQUIRE(num_gaussians >= 0 && sh_degree >= 0 && sh_degree <= 3, "bad num_gaussians / sh_degree");
    if (num_gaussians == 0) return LCGS_OK;
    LCGS_ENTRY(ctx);
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    const int64_t P = num_gaussians, N = c->world;
    int64_t       first = 0, count = 0;
    lcgs_comm_shard_rows(P, c->world, c->rank, &first, &count);
    const int64_t  tail0 = count * N, tail = P - tail0; // rows every rank keeps (fewer than N)
    const AttrRows g = attr_rows(grads, sh_degree), act = attr_rows(activated, sh_degree);
    for (int i = 0; i < 5; ++i) LCGS_REQUIRE(g.ptr[i] && act.ptr[i], "NULL device pointer");

    // ---- 1. reduce-scatter: rank r ends up with the summed gradient rows [r c, (r + 1) c); the tail is all-reduced
    LCGS_TRY(c->compute_to_comm());
    ctx->slices_recorded = 0;
    Wire      wire{ c };
    LoopGuard guard{ c };
    LCGS_TRY(wire.group_begin());
    for (int i = 0; i < 5; ++i) {
        if (count > 0)
            LCGS_TRY(wire.reduce_scatter_sum(g.ptr[i], g.ptr[i] + (size_t)first * g.width[i], (size_t)count * g.width[i]));
        if (tail > 0) LCGS_TRY(wire.allreduce_sum(g.ptr[i] + (size_t)tail0 * g.width[i], (size_t)tail * g.width[i]));
    }
    LCGS_TRY(wire.group_end());
    LCGS_TRY(c->comm_to_compute());

    c->stats                   = lcgs_comm_stats{}; // (kept as it is: reset BEHIND the group here, in front of it in the sparse step)
    c->stats.collective_groups = 1;
    c->stats.bytes_sent = c->stats.bytes_received = (int64_t)((uint64_t)(N - 1) * (uint64_t)count * g.row_bytes());

    // ---- 2. Adam on the own rows (and on the tail, identically on every rank); 3. all-gather of the ACTIVATED rows
    LCGS_TRY(adam_own_rows(ctx, c, P, sh_degree, cfg, grads, raw, m, v, activated));
    LCGS_TRY(allgather_activated(ctx, c, P, sh_degree, act));
    guard.ok = true;
    return LCGS_OK;
}


// ------------------------------------------------------------------------------------------------------------------
// Sparse gradient exchange (round 3).  Dense rows stay the layout; what crosses xGMI in the REDUCE half of the step is
// only what a rank's views touched: rank r hands owner o the touched rows of o's shard (indices + 59 floats each),
// the owner adds them to its own rows in rank order, runs Adam on its shard and the refreshed activated rows are
// all-gathered as in the sharded step.  Exact in f32 up to the order of the sum.
// ------------------------------------------------------------------------------------------------------------------
lcgs_status lcgs_comm_track_touched_rows(lcgs_comm* c, int enable)
{
    LCGS_REQUIRE(c != nullptr, "comm is NULL");
    c->track_rows = enable != 0;
    c->flags_P    = 0; // the next marking backward starts from a cleared array
    return LCGS_OK;
}

int64_t lcgs_sparse_message_words(int64_t count, int sh_degree) { return sparse_message_words(count, sh_degree); }

lcgs_status lcgs_sparse_pack(lcgs_context* ctx, int sh_degree, const lcgs_grads* grads, const uint32_t* d_rows, int64_t count,
                             float* d_msg)
{
    LCGS_REQUIRE(ctx && grads && (count == 0 || (d_rows && d_msg)) && count >= 0 && sh_degree >= 0 && sh_degree <= 3,
                 "bad argument");
    LCGS_ENTRY(ctx);
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    launch_sparse_pack(attr_rows(grads, sh_degree).ptr, sh_degree, d_rows, count, d_msg, ctx->stream);
    LCGS_HIP_CHECK(hipGetLastError());
    return LCGS_OK;
}

lcgs_status lcgs_sparse_accumulate(lcgs_context* ctx, int sh_degree, const lcgs_grads* grads, const float* d_msg, int64_t count,
                                   int64_t row_first, int64_t row_count)
{
    LCGS_REQUIRE(ctx && grads && (count == 0 || d_msg) && count >= 0 && sh_degree >= 0 && sh_degree <= 3, "bad argument");
    LCGS_REQUIRE(row_first >= 0 && row_count >= 0 && row_first + row_count <= ((int64_t)1 << 30), "bad row range");
    LCGS_ENTRY(ctx);
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    launch_sparse_accumulate(attr_rows(grads, sh_degree).ptr, sh_degree, d_msg, count, row_first, row_count, ctx->stream);
    LCGS_HIP_CHECK(hipGetLastError());
    return LCGS_OK;
}

} // extern "C"

namespace
{
// flags -> ascending rows + owner bounds, on the context's stream; the flags are consumed (cleared) behind it
lcgs_status compact_touched(lcgs_context* ctx, lcgs_comm* c, int64_t P, int world)
{
    LCGS_REQUIRE(c->track_rows, "lcgs_comm_track_touched_rows(comm, 1) must be set before the step's backward passes");
    const size_t fb = sparse_flag_bytes(P);
    if (c->flags_P != P) { // no backward has marked anything for this scene since tracking began: an empty set
        LCGS_TRY(c->flags.ensure(fb));
        LCGS_HIP_CHECK(hipMemsetAsync(c->flags.ptr, 0, fb, ctx->stream));
        c->flags_P = P;
    }
    LCGS_TRY(c->chunk_ws.ensure((size_t)sparse_flag_chunks(P) * 4 + 4));
    LCGS_TRY(c->rows.ensure((size_t)P * 4 + 4));
    LCGS_TRY(c->bounds.ensure((size_t)(LCGS_MAX_RANKS + 3) * 4));
    uint32_t* bounds = c->bounds.as<uint32_t>();
    uint32_t* total  = bounds + LCGS_MAX_RANKS + 2;
    launch_compact_flags(c->flags.as<uint8_t>(), P, c->chunk_ws.as<uint32_t>(), c->rows.as<uint32_t>(), total, ctx->stream);
    int64_t first = 0, shard = 0;
    lcgs_comm_shard_rows(P, world, 0, &first, &shard);
    // (P < N: shards are empty, every row is a tail row -- the bounds all sit at 0 and the tail starts there)
    launch_owner_bounds(c->rows.as<uint32_t>(), total, shard, world, bounds, ctx->stream);
    LCGS_HIP_CHECK(hipMemsetAsync(c->flags.ptr, 0, fb, ctx->stream)); // consumed: the next step starts empty
    LCGS_HIP_CHECK(hipGetLastError());
    return LCGS_OK;
}
} // namespace

namespace lcgs
{
// (abi_backward.cpp render_backward) flag the rows of the frame a dense backward has just differentiated
lcgs_status comm_mark_touched(lcgs_comm* c, const KeptRows& rows, bool accumulate, hipStream_t stream)
{
    const int64_t P = rows.P;
    if (!c || !c->track_rows || P <= 0) return LCGS_OK;
    const size_t fb = sparse_flag_bytes(P);
    if (c->flags_P != P || !accumulate) {
        LCGS_TRY(c->flags.ensure(fb));
        LCGS_HIP_CHECK(hipMemsetAsync(c->flags.ptr, 0, fb, stream));
        c->flags_P = P;
    }
    launch_mark_rows(rows, c->flags.as<uint8_t>(), stream);
    return LCGS_OK;
}
} // namespace lcgs

extern "C" {

lcgs_status lcgs_sparse_touched_rows(lcgs_context* ctx, lcgs_comm* c, int num_gaussians, int world_size, lcgs_sparse_rows* out)
{
    LCGS_REQUIRE(ctx && c && out, "NULL argument");
    LCGS_REQUIRE(c->ctx == ctx, "the communicator belongs to another context");
    LCGS_REQUIRE(num_gaussians >= 0 && world_size >= 1 && world_size <= LCGS_MAX_RANKS, "bad num_gaussians / world_size");
    LCGS_ENTRY(ctx);
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    memset(out, 0, sizeof(*out));
    if (num_gaussians == 0) return LCGS_OK;
    LCGS_TRY(compact_touched(ctx, c, num_gaussians, world_size));
    LCGS_TRY(c->ensure_h_matrix());
    LCGS_HIP_CHECK(hipMemcpyAsync(c->h_matrix, c->bounds.ptr, (size_t)(world_size + 2) * 4, hipMemcpyDeviceToHost, ctx->stream));
    LCGS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    out->d_rows = c->rows.as<uint32_t>();
    for (int o = 0; o <= world_size + 1; ++o) out->owner_first[o] = c->h_matrix[o];
    out->num_rows = out->owner_first[world_size + 1];
    return LCGS_OK;
}

lcgs_status lcgs_adam_step_sparse(lcgs_context* ctx, lcgs_comm* c, int num_gaussians, int sh_degree,
                                  const lcgs_adam_config* cfg, const lcgs_grads* grads, const lcgs_params* raw,
                                  const lcgs_params* m, const lcgs_params* v, const lcgs_params* activated)
{
    LCGS_REQUIRE(ctx && c && cfg && grads && raw && m && v && activated, "NULL argument");
    LCGS_REQUIRE(c->ctx == ctx, "the communicator belongs to another context");
    LCGS_REQUIRE(c->loop == nullptr || c->transport == LCGS_TRANSPORT_F32, "the in-process (loopback) transport moves f32 only");
    LCGS_REQUIRE(cfg->visible_only == 0, "the sparse step keeps dense-Adam semantics (every row decays): visible_only must be 0");
    LCGS_REQUIRE(num_gaussians >= 0 && sh_degree >= 0 && sh_degree <= 3, "bad num_gaussians / sh_degree");
    if (num_gaussians == 0) return LCGS_OK;
    LCGS_ENTRY(ctx);
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    const int64_t  P = num_gaussians;
    const int      N = c->world, me = c->rank;
    int64_t        first = 0, count = 0;
    lcgs_comm_shard_rows(P, N, me, &first, &count);
    const int64_t  tail0 = count * N, tail = P - tail0;
    const AttrRows g = attr_rows(grads, sh_degree), act = attr_rows(activated, sh_degree);
    for (int i = 0; i < 5; ++i) LCGS_REQUIRE(g.ptr[i] && act.ptr[i], "NULL device pointer");
    ctx->slices_recorded = 0;
    c->stats             = lcgs_comm_stats{};

    // ---- 1. this rank's touched rows, ascending, and where each owner's shard begins in that list
    LCGS_TRY(compact_touched(ctx, c, P, N));
    const int W = N + 2; // positions per rank: N shard starts, the tail's start, the total
    LCGS_TRY(c->matrix.ensure((size_t)N * W * 4));
    LCGS_TRY(c->ensure_h_matrix());
    LCGS_TRY(c->compute_to_comm());
    // ---- 2. everybody learns everybody's counts (message sizes are host arguments of send / recv): one small
    //         all-gather + read-back, the step's only host synchronisation
    Wire      wire{ c };
    LoopGuard guard{ c };
    LCGS_TRY(wire.allgather_u32(c->bounds.as<uint32_t>(), c->matrix.as<uint32_t>(), (size_t)W));
    LCGS_HIP_CHECK(hipMemcpyAsync(c->h_matrix, c->matrix.ptr, (size_t)N * W * 4, hipMemcpyDeviceToHost, c->stream));
    LCGS_HIP_CHECK(hipStreamSynchronize(c->stream));
    auto rows_of = [&](int src, int owner) -> int64_t { // rows rank `src` holds for owner's shard
        return (int64_t)c->h_matrix[src * W + owner + 1] - (int64_t)c->h_matrix[src * W + owner];
    };
    c->stats.touched_rows = (int64_t)c->h_matrix[me * W + N + 1];
    int64_t send_words = 0, recv_words = 0, send_off[LCGS_MAX_RANKS], recv_off[LCGS_MAX_RANKS];
    for (int o = 0; o < N; ++o) {
        send_off[o] = send_words;
        recv_off[o] = recv_words;
        if (o == me) continue;
        send_words += sparse_message_words(rows_of(me, o), sh_degree);
        recv_words += sparse_message_words(rows_of(o, me), sh_degree);
    }
    LCGS_TRY(c->sendbuf.ensure((size_t)send_words * 4 + 16));
    LCGS_TRY(c->recvbuf.ensure((size_t)recv_words * 4 + 16));

    // ---- 3. pack one message per peer (context's stream), exchange (communicator's stream); the tail rows -- fewer than
    //         N, kept by everyone -- are all-reduced densely behind it
    for (int o = 0; o < N; ++o)
        if (o != me)
            launch_sparse_pack(g.ptr, sh_degree, c->rows.as<uint32_t>() + c->h_matrix[me * W + o], rows_of(me, o),
                               c->sendbuf.as<float>() + send_off[o], ctx->stream);
    LCGS_HIP_CHECK(hipGetLastError());
    LCGS_TRY(c->compute_to_comm());
    LCGS_TRY(wire.group_begin());
    for (int o = 0; o < N; ++o) {
        if (o == me) continue;
        const int64_t sw = sparse_message_words(rows_of(me, o), sh_degree), rw = sparse_message_words(rows_of(o, me), sh_degree);
        if (sw > 0) LCGS_TRY(wire.send(c->sendbuf.as<float>() + send_off[o], (size_t)sw * 4, o));
        if (rw > 0) LCGS_TRY(wire.recv(c->recvbuf.as<float>() + recv_off[o], (size_t)rw * 4, o));
    }
    LCGS_TRY(wire.group_end());
    if (tail > 0) { // (its own group: point-to-point and collective calls are not mixed in one)
        LCGS_TRY(wire.group_begin());
        for (int i = 0; i < 5; ++i) LCGS_TRY(wire.allreduce_sum(g.ptr[i] + (size_t)tail0 * g.width[i], (size_t)tail * g.width[i]));
        LCGS_TRY(wire.group_end());
    }
    c->stats.collective_groups = 2 + (tail > 0 ? 1 : 0); // the counts, the messages, the tail
    c->stats.bytes_sent        = send_words * 4 + (int64_t)(N - 1) * W * 4;
    c->stats.bytes_received    = recv_words * 4 + (int64_t)(N - 1) * W * 4;
    LCGS_TRY(c->comm_to_compute());

    // ---- 4. the owner adds what it received, message by message in rank order (a fixed order: reproducible sums)
    for (int o = 0; o < N; ++o)
        if (o != me) // (only rows of the own shard are accepted, whatever the message says)
            launch_sparse_accumulate(g.ptr, sh_degree, c->recvbuf.as<float>() + recv_off[o], rows_of(o, me), first, count, ctx->stream);
    LCGS_HIP_CHECK(hipGetLastError());

    // ---- 5. Adam on the own rows (+ the tail), 6. all-gather of the refreshed ACTIVATED rows: as in the sharded step
    LCGS_TRY(adam_own_rows(ctx, c, P, sh_degree, cfg, grads, raw, m, v, activated));
    LCGS_TRY(allgather_activated(ctx, c, P, sh_degree, act));
    guard.ok = true;
    return LCGS_OK;
}

} // extern "C"
