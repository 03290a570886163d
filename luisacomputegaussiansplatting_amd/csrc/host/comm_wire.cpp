// comm_wire.cpp -- the run-time RCCL binding, the transport of one communicator (Wire: RCCL, or the in-process loopback
// with its rendezvous in group_end) and the life of communicators and loopback groups.
#include "comm_internal.hpp"

using namespace lcgs;

namespace lcgs
{

RcclApi& rccl()
{
    static RcclApi       api;
    static std::once_flag once;
    std::call_once(once, [] {
        const char* names[] = { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1" };
        for (const char* n : names) // a copy the process already carries (torch's) wins
            if (!api.handle) api.handle = dlopen(n, RTLD_NOW | RTLD_NOLOAD);
        for (const char* n : names)
            if (!api.handle) api.handle = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (!api.handle) {
            const char* e = dlerror();
            api.error     = std::string("RCCL is not available (dlopen librccl.so.1: ") + (e ? e : "?") + ")";
            return;
        }
        bool ok = true;
        auto bind = [&](auto& fn, const char* sym) {
            fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(dlsym(api.handle, sym));
            if (!fn) {
                ok        = false;
                api.error = std::string("librccl lacks ") + sym;
            }
        };
        bind(api.GetUniqueId, "ncclGetUniqueId");
        bind(api.CommInitRank, "ncclCommInitRank");
        bind(api.CommDestroy, "ncclCommDestroy");
        bind(api.AllReduce, "ncclAllReduce");
        bind(api.ReduceScatter, "ncclReduceScatter");
        bind(api.AllGather, "ncclAllGather");
        bind(api.Send, "ncclSend");
        bind(api.Recv, "ncclRecv");
        bind(api.GroupStart, "ncclGroupStart");
        bind(api.GroupEnd, "ncclGroupEnd");
        bind(api.GetErrorString, "ncclGetErrorString");
        if (!ok) api.handle = nullptr;
    });
    return api;
}

lcgs_status rccl_fail(ncclResult_t r, const char* what, const char* file, int line)
{
    char buf[384];
    const char* base = strrchr(file, '/');
    snprintf(buf, sizeof(buf), "RCCL error %d (%s) in `%s` at %s:%d", (int)r,
             rccl().GetErrorString ? rccl().GetErrorString(r) : "?", what, base ? base + 1 : file, line);
    set_last_error(buf);
    return LCGS_ERR_HIP;
}

lcgs_status need_rccl()
{
    if (rccl().handle) return LCGS_OK;
    set_last_error(rccl().error.empty() ? "RCCL is not available" : rccl().error);
    return LCGS_ERR_NO_DEVICE;
}

void comm_forget_context(lcgs_comm* c)
{
    if (!c) return;
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    c->ctx = nullptr;
}

lcgs_status Wire::loop_failed()
{
    set_last_error("loopback: another member of the group failed");
    return LCGS_ERR_STATE;
}
lcgs_status Wire::group_begin()
{
    if (!c->loop) LCGS_RCCL_CHECK(rccl().GroupStart());
    else {
        c->own.recvs.clear();
        c->loop_ops.clear();
    }
    return LCGS_OK;
}
// (RCCL: an error inside an open group closes it before it is reported)
lcgs_status Wire::rccl_call(ncclResult_t r, const char* what, const char* file, int line)
{
    if (r == ncclSuccess) return LCGS_OK;
    (void)rccl().GroupEnd();
    return rccl_fail(r, what, file, line);
}
lcgs_status Wire::allreduce_sum(float* p, size_t count) // in place
{
    if (!c->loop) return rccl_call(rccl().AllReduce(p, p, count, ncclFloat32, ncclSum, c->comm, c->stream), "ncclAllReduce", __FILE__, __LINE__);
    c->loop_ops.push_back({ 0, p, p, count });
    return LCGS_OK;
}
lcgs_status Wire::reduce_scatter_sum(const float* send, float* recv, size_t count_per_rank)
{
    if (!c->loop)
        return rccl_call(rccl().ReduceScatter(send, recv, count_per_rank, ncclFloat32, ncclSum, c->comm, c->stream),
                         "ncclReduceScatter", __FILE__, __LINE__);
    c->loop_ops.push_back({ 1, send, recv, count_per_rank });
    return LCGS_OK;
}
lcgs_status Wire::allgather(const float* send, float* recv, size_t count_per_rank)
{
    if (!c->loop)
        return rccl_call(rccl().AllGather(send, recv, count_per_rank, ncclFloat32, c->comm, c->stream), "ncclAllGather", __FILE__, __LINE__);
    c->loop_ops.push_back({ 2, send, recv, count_per_rank });
    return LCGS_OK;
}
lcgs_status Wire::send(const void* d_buf, size_t bytes, int peer)
{
    if (!c->loop) return rccl_call(rccl().Send(d_buf, bytes, ncclUint8, peer, c->comm, c->stream), "ncclSend", __FILE__, __LINE__);
    lcgs_loopback_group::Msg m{ d_buf, bytes, {} };
    LCGS_TRY(m.ready.ensure());
    LCGS_HIP_CHECK(hipEventRecord(m.ready, c->stream));
    std::lock_guard<std::mutex> lock(c->loop->mu);
    c->loop->box[(size_t)peer * c->loop->world + c->rank].push_back(std::move(m));
    return LCGS_OK;
}
lcgs_status Wire::recv(void* d_buf, size_t bytes, int peer)
{
    if (!c->loop) return rccl_call(rccl().Recv(d_buf, bytes, ncclUint8, peer, c->comm, c->stream), "ncclRecv", __FILE__, __LINE__);
    c->own.recvs.push_back({ d_buf, { bytes, peer } });
    return LCGS_OK;
}
// a small all-gather of `count` words per rank, outside any group (message sizes: the host reads the result back)
lcgs_status Wire::allgather_u32(const uint32_t* d_send, uint32_t* d_recv, size_t count)
{
    if (!c->loop) {
        LCGS_RCCL_CHECK(rccl().AllGather(d_send, d_recv, count, ncclUint32, c->comm, c->stream));
        return LCGS_OK;
    }
    lcgs_loopback_group* g = c->loop;
    std::vector<uint32_t> mine(count);
    LCGS_HIP_CHECK(hipMemcpyAsync(mine.data(), d_send, count * 4, hipMemcpyDeviceToHost, c->stream));
    LCGS_HIP_CHECK(hipStreamSynchronize(c->stream));
    {
        std::lock_guard<std::mutex> lock(g->mu);
        if (g->table.size() < (size_t)g->world * count) g->table.resize((size_t)g->world * count);
        std::copy(mine.begin(), mine.end(), g->table.begin() + (size_t)c->rank * count);
    }
    if (!g->barrier()) return loop_failed();
    std::vector<uint32_t> all;
    {
        std::lock_guard<std::mutex> lock(g->mu);
        all.assign(g->table.begin(), g->table.begin() + (size_t)g->world * count);
    }
    LCGS_HIP_CHECK(hipMemcpy(d_recv, all.data(), all.size() * 4, hipMemcpyHostToDevice));
    if (!g->barrier()) return loop_failed(); // nobody overwrites the table before everybody has read it
    return LCGS_OK;
}
// a few words max-reduced in place, outside any group (the ownership step's redo flag)
lcgs_status Wire::allreduce_max_u32(uint32_t* d_buf, size_t count)
{
    if (!c->loop) {
        LCGS_RCCL_CHECK(rccl().AllReduce(d_buf, d_buf, count, ncclUint32, ncclMax, c->comm, c->stream));
        return LCGS_OK;
    }
    LCGS_REQUIRE(count <= 8, "loopback: the flag reduction carries a few words");
    const int N = c->loop->world;
    DeviceBuffer all;
    LCGS_TRY(all.ensure((size_t)N * count * 4));
    LCGS_TRY(allgather_u32(d_buf, all.as<uint32_t>(), count)); // (the loopback's rendezvous is host-side anyway)
    uint32_t h[8 * LCGS_MAX_RANKS], m[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    LCGS_HIP_CHECK(hipMemcpy(h, all.ptr, (size_t)N * count * 4, hipMemcpyDeviceToHost));
    for (int r = 0; r < N; ++r)
        for (size_t k = 0; k < count; ++k) m[k] = std::max(m[k], h[(size_t)r * count + k]);
    LCGS_HIP_CHECK(hipMemcpyAsync(d_buf, m, count * 4, hipMemcpyHostToDevice, c->stream));
    LCGS_HIP_CHECK(hipStreamSynchronize(c->stream)); // (m lives on this stack)
    return LCGS_OK;
}
lcgs_status Wire::group_end()
{
    if (!c->loop) {
        LCGS_RCCL_CHECK(rccl().GroupEnd());
        return LCGS_OK;
    }
    lcgs_loopback_group* g  = c->loop;
    const int            N  = g->world, me = c->rank;
    hipStream_t          st = c->stream;
    // ---- what this rank's collectives of the group need as scratch: its slice of every all-reduce
    size_t scratch_elems = 0;
    for (const auto& op : c->loop_ops)
        if (op.kind == 0) scratch_elems += (op.count + N - 1) / N;
    LCGS_TRY(c->loop_scratch.ensure(scratch_elems * 4 + 16));
    {
        std::lock_guard<std::mutex> lock(g->mu);
        if (g->coll.size() < c->loop_ops.size()) g->coll.resize(c->loop_ops.size());
        for (size_t k = 0; k < c->loop_ops.size(); ++k) {
            g->coll[k].resize(N);
            g->coll[k][me] = { c->loop_ops[k].send, c->loop_ops[k].recv };
        }
        g->scratch[me] = c->loop_scratch.as<float>();
    }
    LCGS_HIP_CHECK(hipEventRecord(g->ready[me], st)); // my inputs (and my posted sends) are complete behind this
    if (!g->barrier()) return loop_failed();           // every rank has posted its sends and its collectives' buffers
    for (int r = 0; r < N; ++r)
        if (r != me) LCGS_HIP_CHECK(hipStreamWaitEvent(st, g->ready[r], 0));
    // ---- point-to-point: copy what was sent to me
    std::vector<Event> consumed; // (alive until everybody's copies have been waited for)
    for (auto& r : c->own.recvs) {
        lcgs_loopback_group::Msg m{};
        {
            std::lock_guard<std::mutex> lock(g->mu);
            auto& q = g->box[(size_t)me * N + r.second.second];
            if (q.empty() || q.front().bytes != r.second.first) {
                g->failed = true;
                g->cv.notify_all();
                set_last_error("loopback: a receive has no matching send of the same size (ranks disagree on the message table)");
                return LCGS_ERR_STATE;
            }
            m = std::move(q.front());
            q.pop_front();
        }
        LCGS_HIP_CHECK(hipStreamWaitEvent(st, m.ready, 0));
        if (m.bytes) LCGS_HIP_CHECK(hipMemcpyAsync(r.first, m.ptr, m.bytes, hipMemcpyDeviceToDevice, st));
        consumed.push_back(std::move(m.ready));
    }
    // ---- collectives, phase 1: reductions that only READ the other ranks' buffers (sums in rank order)
    std::vector<lcgs_loopback_group::CollArgs> args; // (a private copy: the shared table is re-used by the next group)
    size_t                                      at = 0;
    for (size_t k = 0; k < c->loop_ops.size(); ++k) {
        const auto& op = c->loop_ops[k];
        {
            std::lock_guard<std::mutex> lock(g->mu);
            args = g->coll[k];
        }
        const float* srcs[16];
        if (op.kind == 0) { // all-reduce: I reduce slice `me` of everybody's array into my scratch
            const size_t per = (op.count + N - 1) / N, lo = std::min(op.count, per * (size_t)me),
                         n = std::min(op.count, lo + per) - lo;
            for (int r = 0; r < N; ++r) srcs[r] = args[r].send + lo;
            launch_sum_sources(srcs, N, n, c->loop_scratch.as<float>() + at, st);
            at += per;
        } else if (op.kind == 1) { // reduce-scatter: my slice of everybody's send array, straight into my recv
            for (int r = 0; r < N; ++r) srcs[r] = args[r].send + op.count * (size_t)me;
            launch_sum_sources(srcs, N, op.count, op.recv, st);
        }
    }
    LCGS_HIP_CHECK(hipGetLastError());
    LCGS_HIP_CHECK(hipEventRecord(g->reduced[me], st));
    if (!g->barrier()) return loop_failed(); // every rank's phase 1 is enqueued
    for (int r = 0; r < N; ++r)
        if (r != me) LCGS_HIP_CHECK(hipStreamWaitEvent(st, g->reduced[r], 0));
    // ---- phase 2: gathers that WRITE my own arrays from what the others left (their scratch slices / send arrays)
    std::vector<float*> scr;
    {
        std::lock_guard<std::mutex> lock(g->mu);
        scr = g->scratch;
    }
    at = 0;
    for (size_t k = 0; k < c->loop_ops.size(); ++k) {
        const auto& op = c->loop_ops[k];
        {
            std::lock_guard<std::mutex> lock(g->mu);
            args = g->coll[k];
        }
        if (op.kind == 0) {
            const size_t per = (op.count + N - 1) / N;
            for (int r = 0; r < N; ++r) {
                const size_t lo = std::min(op.count, per * (size_t)r), n = std::min(op.count, lo + per) - lo;
                if (n) LCGS_HIP_CHECK(hipMemcpyAsync(op.recv + lo, scr[r] + at, n * 4, hipMemcpyDeviceToDevice, st));
            }
            at += per;
        } else if (op.kind == 2) {
            for (int r = 0; r < N; ++r)
                if (op.count && args[r].send != op.recv + op.count * (size_t)r) // (in place: my own slice is where it belongs)
                    LCGS_HIP_CHECK(hipMemcpyAsync(op.recv + op.count * (size_t)r, args[r].send, op.count * 4,
                                                  hipMemcpyDeviceToDevice, st));
        }
    }
    LCGS_HIP_CHECK(hipEventRecord(g->done[me], st));
    if (!g->barrier()) return loop_failed(); // every copy out of my buffers / scratch has been enqueued
    for (int p = 0; p < N; ++p)               // ... and has run before I touch them again
        if (p != me) LCGS_HIP_CHECK(hipStreamWaitEvent(st, g->done[p], 0));
    if (!g->barrier()) return loop_failed(); // (the shared events are not re-recorded before everybody has waited on them)
    return LCGS_OK;
}

} // namespace lcgs

namespace
{
// What both constructors give a communicator: its own stream and the two events of the hand-offs.  highest_priority: the
// collective's workgroups should get their slots as soon as a chunk is ready, not queue behind the backward's remaining
// slices (the auxiliary stream of the context has the LOWEST, for the opposite reason); the loopback asks for none.
lcgs_status create_stream_and_events(lcgs_comm* c, bool highest_priority)
{
    int lo = 0, hi = 0;
    if (highest_priority) (void)hipDeviceGetStreamPriorityRange(&lo, &hi); // hi = numerically smallest = highest priority
    LCGS_TRY(highest_priority ? c->stream.ensure_priority(hi) : c->stream.ensure());
    LCGS_TRY(c->ev_in.ensure());
    return c->ev_out.ensure();
}

// chunked all-reduce: the dense backward slices its preprocess pass (tuning hook LCGS_GRAD_SLICES; 1 = one chunk)
void set_grad_slices(lcgs_context* ctx)
{
    int slices = 4;
    if (const char* s = getenv("LCGS_GRAD_SLICES")) slices = atoi(s);
    ctx->grad_slices = std::min(std::max(slices, 1), kMaxGradSlices);
}
} // namespace

extern "C" {

lcgs_status lcgs_comm_unique_id(lcgs_comm_id* out)
{
    LCGS_REQUIRE(out != nullptr, "out is NULL");
    static_assert(sizeof(lcgs_comm_id) == sizeof(ncclUniqueId), "lcgs_comm_id must hold an ncclUniqueId");
    LCGS_TRY(need_rccl());
    ncclUniqueId id;
    LCGS_RCCL_CHECK(rccl().GetUniqueId(&id));
    memcpy(out->bytes, id.internal, sizeof(id.internal));
    return LCGS_OK;
}

lcgs_status lcgs_comm_create(lcgs_context* ctx, const lcgs_comm_id* id, int rank, int world_size, lcgs_comm** out)
{
    LCGS_REQUIRE(ctx && id && out, "NULL argument");
    *out = nullptr;
    LCGS_REQUIRE(world_size >= 1 && rank >= 0 && rank < world_size, "rank / world_size out of range");
    LCGS_REQUIRE(world_size <= LCGS_MAX_RANKS, "world_size above LCGS_MAX_RANKS");
    LCGS_ENTRY(ctx);
    LCGS_REQUIRE(ctx->comm == nullptr, "the context already has a communicator attached");
    LCGS_TRY(need_rccl());
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    lcgs_comm* c = new (std::nothrow) lcgs_comm();
    if (!c) return LCGS_ERR_OUT_OF_MEMORY;
    c->ctx    = ctx;
    c->device = ctx->device;
    c->rank   = rank;
    c->world = world_size;
    if (const lcgs_status s = create_stream_and_events(c, /*highest_priority=*/true); s != LCGS_OK) {
        (void)lcgs_comm_destroy(c);
        return s;
    }
    ncclUniqueId nid;
    memcpy(nid.internal, id->bytes, sizeof(nid.internal));
    ncclResult_t r = rccl().CommInitRank(&c->comm, world_size, nid, rank);
    if (r != ncclSuccess) {
        c->comm = nullptr;
        (void)lcgs_comm_destroy(c);
        return rccl_fail(r, "ncclCommInitRank", __FILE__, __LINE__);
    }
    ctx->comm = c;
    if (const char* s = getenv("LCGS_OWNER_SELF_P2P")) c->self_p2p = s[0] == '1'; // test hook (see lcgs_owner_step_forward)
    set_grad_slices(ctx);
    *out = c;
    return LCGS_OK;
}

lcgs_status lcgs_comm_destroy(lcgs_comm* c)
{
    if (!c) return LCGS_OK;
    (void)hipSetDevice(c->device); // (also after the context has gone: comm_forget_context)
    if (c->ctx) {
        if (c->ctx->comm == c) {
            c->ctx->comm        = nullptr;
            c->ctx->grad_slices = 1;
        }
    }
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->comm && rccl().CommDestroy) (void)rccl().CommDestroy(c->comm);
    if (c->loop) {
        std::lock_guard<std::mutex> lock(c->loop->mu);
        --c->loop->members;
        if (c->rank >= 0 && (size_t)c->rank < c->loop->taken.size()) c->loop->taken[(size_t)c->rank] = 0;
    }
    delete c; // (its buffers, events, pinned blocks and stream free themselves)
    return LCGS_OK;
}

lcgs_status lcgs_comm_set_transport(lcgs_comm* c, int transport)
{
    LCGS_REQUIRE(c != nullptr, "comm is NULL");
    LCGS_REQUIRE(transport == LCGS_TRANSPORT_F32 || transport == LCGS_TRANSPORT_F16, "unknown transport");
    c->transport = transport;
    return LCGS_OK;
}

lcgs_status lcgs_comm_info(const lcgs_comm* c, int* rank, int* world_size)
{
    LCGS_REQUIRE(c != nullptr, "comm is NULL");
    if (rank) *rank = c->rank;
    if (world_size) *world_size = c->world;
    return LCGS_OK;
}

lcgs_status lcgs_comm_get_stats(const lcgs_comm* c, lcgs_comm_stats* out)
{
    LCGS_REQUIRE(c && out, "NULL argument");
    *out = c->stats;
    return LCGS_OK;
}

lcgs_status lcgs_loopback_group_create(int world_size, lcgs_loopback_group** out)
{
    LCGS_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    LCGS_REQUIRE(world_size >= 1 && world_size <= LCGS_MAX_OWNER_VIEWS, "world_size out of range");
    lcgs_loopback_group* g = new (std::nothrow) lcgs_loopback_group();
    if (!g) return LCGS_ERR_OUT_OF_MEMORY;
    g->world = world_size;
    g->box.resize((size_t)world_size * world_size);
    g->done.resize(world_size);
    g->ready.resize(world_size);
    g->reduced.resize(world_size);
    g->scratch.assign(world_size, nullptr);
    g->taken.assign(world_size, 0);
    *out = g;
    return LCGS_OK;
}

lcgs_status lcgs_loopback_group_destroy(lcgs_loopback_group* g)
{
    if (!g) return LCGS_OK;
    LCGS_REQUIRE(g->members == 0, "communicators of this group are still alive");
    delete g;
    return LCGS_OK;
}

lcgs_status lcgs_comm_create_loopback(lcgs_context* ctx, lcgs_loopback_group* group, int rank, lcgs_comm** out)
{
    LCGS_REQUIRE(ctx && group && out, "NULL argument");
    *out = nullptr;
    LCGS_REQUIRE(rank >= 0 && rank < group->world, "rank out of range");
    LCGS_ENTRY(ctx);
    LCGS_REQUIRE(ctx->comm == nullptr, "the context already has a communicator attached");
    {
        std::lock_guard<std::mutex> lock(group->mu);
        LCGS_REQUIRE(!group->taken[(size_t)rank], "this rank of the loopback group already has a communicator");
        LCGS_REQUIRE(group->device < 0 || group->device == ctx->device, "the members of a loopback group share ONE device");
        group->taken[(size_t)rank] = 1;
        group->device              = ctx->device;
    }
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    lcgs_comm* c = new (std::nothrow) lcgs_comm();
    if (!c) return LCGS_ERR_OUT_OF_MEMORY;
    c->ctx = ctx, c->device = ctx->device, c->rank = rank, c->world = group->world, c->loop = group;
    lcgs_status s = create_stream_and_events(c, /*highest_priority=*/false);
    {
        std::lock_guard<std::mutex> lock(group->mu);
        for (auto* evs : { &group->done, &group->ready, &group->reduced })
            if (s == LCGS_OK) s = (*evs)[rank].ensure();
        if (s == LCGS_OK) ++group->members;
    }
    if (s != LCGS_OK) {
        {
            std::lock_guard<std::mutex> lock(group->mu);
            group->taken[(size_t)rank] = 0;
        }
        c->loop = nullptr;
        (void)lcgs_comm_destroy(c);
        return s;
    }
    ctx->comm = c; // (kept as it is: the test hook LCGS_OWNER_SELF_P2P is lcgs_comm_create's alone and is not read here)
    set_grad_slices(ctx);
    *out = c;
    return LCGS_OK;
}

} // extern "C"
