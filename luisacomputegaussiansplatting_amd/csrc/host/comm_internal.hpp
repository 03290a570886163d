// comm_internal.hpp -- the types and helpers the host/comm_*.cpp files share.
// Multi-GPU side of the C ABI: one process per GPU, the scene replicated, every rank renders
// its own view(s); the dense per-splat gradients are summed over the ranks with RCCL over xGMI.  The reference is
// single-device (app/main.cpp:162-163): everything here is new functionality behind the same boundary.
//
// RCCL is bound at run time (dlopen), not at link time: a process that already carries a copy -- torch ships its own
// librccl.so next to its libamdhip64.so -- keeps using that one (two copies of a HIP-facing runtime in one process do
// not end well), a process without one loads the ROCm installation's, and liblcgs_hip.so still loads on a machine
// where RCCL is absent (the lcgs_comm_* calls then fail with a message; nothing else needs it).
//
// Two ways through a training step at N > 1, both exact in f32:
//   lcgs_grads_allreduce     in-place sum of the five dense gradient arrays, issued as splat-range CHUNKS on a
//                            dedicated stream: the dense backward runs its preprocess pass as slices and records an event
//                            behind each (abi_backward.cpp render_backward), so chunk k is on the wire while slices k+1.. are
//                            still being computed.  (SURVEY 8e sketched per-attribute chunks; one kernel writes all five
//                            attributes of a splat, so the chunks are row ranges -- same idea, same bytes.)
//   lcgs_adam_step_sharded   reduce-scatter -> Adam on the rank's own rows -> all-gather of the refreshed activated
//                            arrays.  The wire carries what the all-reduce carries ((N-1)/N S out and in per GPU, twice),
//                            but the optimiser touches P/N rows per GPU instead of P (2.2 ms -> 0.27 ms at N = 8 for the
//                            bicycle stand-in), and moments / raw parameters are only ever needed for the own rows.
#pragma once
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include <rccl/rccl.h> // types and enums only: every entry point is resolved with dlsym

#include "../abi_internal.hpp"

namespace lcgs
{

struct RcclApi {
    void* handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*)                                                                = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int)                                         = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t)                                                                   = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*ReduceScatter)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t)            = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t)                    = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t)                          = nullptr;
    ncclResult_t (*GroupStart)()                                                                              = nullptr;
    ncclResult_t (*GroupEnd)()                                                                                = nullptr;
    const char* (*GetErrorString)(ncclResult_t)                                                               = nullptr;
    std::string error; // why loading failed
};

RcclApi& rccl(); // comm_wire.cpp: one binding (one dlopen) per process

lcgs_status rccl_fail(ncclResult_t r, const char* what, const char* file, int line);

#define LCGS_RCCL_CHECK(expr)                                                   \
    do {                                                                        \
        ncclResult_t _r = (expr);                                               \
        if (_r != ncclSuccess) return rccl_fail(_r, #expr, __FILE__, __LINE__); \
    } while (0)

#define LCGS_TRY(expr)                    \
    do {                                  \
        lcgs_status _s = (expr);          \
        if (_s != LCGS_OK) return _s;     \
    } while (0)

lcgs_status need_rccl();

struct AttrRows {
    float*         ptr[5];
    abi::RowFloats width; // floats per splat: pos 3, scale 3, rotq 4, sh (deg+1)^2*3, opacity 1
    size_t         row_bytes() const { return (width[0] + width[1] + width[2] + width[3] + width[4]) * 4; }
};

inline AttrRows attr_rows(const lcgs_grads* g, int sh_degree)
{
    return { { g->d_dL_dpos, g->d_dL_dscale, g->d_dL_drotq, g->d_dL_dsh, g->d_dL_dopacity }, abi::row_floats(sh_degree) };
}
inline AttrRows attr_rows(const lcgs_params* p, int sh_degree)
{
    return { { p->pos, p->scale, p->rotq, p->sh, p->opacity }, abi::row_floats(sh_degree) };
}

} // namespace lcgs

// An in-process rendezvous for N communicators on ONE device (lcgs_loopback_*): N contexts, one host thread each, standing in
// for N ranks.  Carries what the ownership step needs -- a small all-gather and grouped sends / receives, as device-to-
// device copies ordered by events -- so that the step's C code path (message layout, offsets, slot state, ordering) runs
// with N > 1 participants on a single GPU, where RCCL refuses a second rank.  Not a transport for production.
struct lcgs_loopback_group {
    int                     world = 0;
    std::mutex              mu;
    std::condition_variable cv;
    int                     arrived = 0;
    uint64_t                generation = 0;
    bool                    failed = false; // a member gave up: everybody leaves the barriers with an error
    std::vector<uint32_t>   table;          // all-gather staging: world x count words
    struct Msg {
        const void* ptr;
        size_t      bytes;
        Event       ready; // recorded on the sender's stream behind the data
    };
    std::vector<std::deque<Msg>> box;  // box[dst * world + src]: the sends posted in the open group, in order
    std::vector<Event>           done; // per rank: behind the copies of its receives of the last group
    int                          members = 0;
    int                          device  = -1;  // every member's device (one GPU: that is the point)
    std::vector<char>            taken;         // ranks that have a communicator
    // messages nobody received (a member gave up mid-group)
    void drop_unconsumed()
    {
        for (auto& q : box) q.clear();
    }
    // collectives of the open group (all-reduce / reduce-scatter / all-gather): what every rank passed, op by op
    struct CollArgs {
        const float* send;
        float*       recv;
    };
    std::vector<std::vector<CollArgs>> coll;    // coll[op][rank]
    std::vector<float*>                scratch; // per rank: where it leaves its reduced slices (phase 1 of an all-reduce)
    std::vector<Event>                 ready, reduced; // per rank: inputs complete / phase 1 complete

    bool barrier() // false: the group failed
    {
        std::unique_lock<std::mutex> lock(mu);
        if (failed) return false;
        const uint64_t g = generation;
        if (++arrived == world) {
            arrived = 0;
            ++generation;
            cv.notify_all();
        } else {
            cv.wait(lock, [&] { return generation != g || failed; });
        }
        return !failed;
    }
    void fail()
    {
        std::lock_guard<std::mutex> lock(mu);
        failed = true;
        drop_unconsumed();
        cv.notify_all();
    }
};

struct lcgs_comm {
    lcgs_context* ctx    = nullptr;
    ncclComm_t    comm   = nullptr;
    int           rank   = 0, world = 1;
    Stream        stream; // the collectives' own stream: they overlap the compute stream's tail
    Event         ev_in, ev_out;
    // The two plain hand-offs between the context's stream (compute) and this one.  A place that orders the streams in any
    // other way -- the chunked all-reduce's per-slice waits, the async ownership step's ev_checked -- writes it out.
    lcgs_status compute_to_comm() // what comes next on the communicator's stream runs behind the context's stream as it stands
    {
        LCGS_HIP_CHECK(hipEventRecord(ev_in, ctx->stream));
        LCGS_HIP_CHECK(hipStreamWaitEvent(stream, ev_in, 0));
        return LCGS_OK;
    }
    lcgs_status comm_to_compute() // ... and the other way round
    {
        LCGS_HIP_CHECK(hipEventRecord(ev_out, stream));
        LCGS_HIP_CHECK(hipStreamWaitEvent(ctx->stream, ev_out, 0));
        return LCGS_OK;
    }
    // opt-in f16 transport (lcgs_comm_set_transport): staging for the packed gradients and the five scales
    int          transport = LCGS_TRANSPORT_F32;
    DeviceBuffer packed, scales; // 59 P halfs; 5 magnitudes | 5 scales | 5 inverses (floats)
    int          device = 0;     // (kept beyond the context's life: lcgs_comm_destroy selects it)
    // sparse exchange (lcgs_adam_step_sparse): touched-row flags of the current step, their compaction, the messages
    bool         track_rows = false;
    int64_t      flags_P    = 0;     // rows the flag array covers
    DeviceBuffer flags, chunk_ws, rows, bounds, matrix, sendbuf, recvbuf; // bounds: [world + 2] positions + [1] total
    Pinned<uint32_t> h_matrix; // world x (world + 2) positions (row r = rank r's owner bounds)
    lcgs_status      ensure_h_matrix() { return h_matrix.ensure((size_t)LCGS_MAX_RANKS * (LCGS_MAX_RANKS + 2) * 4); }
    lcgs_comm_stats stats{};
    // splat-ownership step (lcgs_owner_step_forward / _backward): my rows' records for every view of the step, what I
    // received for my view (owner order), its 2-D gradients, and the 2-D gradients of my rows that came back
    lcgs_loopback_group* loop = nullptr; // set: an in-process communicator (lcgs_comm_create_loopback), comm == NULL
    bool         self_p2p = false;       // test hook LCGS_OWNER_SELF_P2P=1: my own share travels through send / recv too
    DeviceBuffer own_rows, own_recs, in_rows, in_recs, g2d_all, g_in;
    DeviceBuffer loop_scratch; // loopback: this rank's reduced slices of the open group's all-reduces
    struct LoopOp {
        int          kind; // 0 all-reduce (in place), 1 reduce-scatter, 2 all-gather
        const float* send;
        float*       recv;
        size_t       count; // all-reduce: elements; the others: elements per rank
    };
    std::vector<LoopOp> loop_ops; // loopback: the collectives of the open group, executed at its end
    // ... without a read-back (lcgs_owner_step_set_async): message sizes come from the PREVIOUS step's all-gathered counts
    // (x 1.25 + 1024: every rank derives the same table), the true counts stay on the device, a clipped message or a
    // truncated frame raises a flag that is max-reduced over the ranks and read by lcgs_owner_step_finish -- the redo is
    // everybody's or nobody's
    bool         owner_async = false, force_sync_once = false;
    struct {
        bool                  have = false;
        int                   world = 0;
        int64_t               P = 0;
        std::vector<uint32_t> table; // [o * N + v]: rows of owner o on view v's screen, last step
    } prev;
    Pinned<uint32_t> h_next;     // the table of the step in flight [N x N] + the reduced flag [1]
    DeviceBuffer flag_dev;           // u32: bit 0 a message was clipped, bit 1 a frame's pairs were truncated (any rank)
    Event        ev_checked; // behind the flag's reduction and the copies to h_next
    struct {
        bool     valid = false;
        bool     async = false;                 // the step in flight used padded messages (sizes below)
        int64_t  cap_in[LCGS_MAX_RANKS]{};      // rows owner o's message to me holds (>= its true count, else clipped)
        int64_t  cap_out[LCGS_MAX_RANKS]{};     // rows my message to view v holds
        int64_t  n_all = 0;                     // rows on my view's screen (all owners)
        int64_t  in_off[LCGS_MAX_RANKS + 1]{};  // owner o's rows start here in in_rows / in_recs / g2d_all
        uint32_t out[LCGS_MAX_RANKS]{};         // my rows on view v's screen (= table[me][v])
        std::vector<std::pair<void*, std::pair<size_t, int>>> recvs; // loopback: receives of the open group
    } own;
};

namespace lcgs
{
// ---------------------------------------------------------------------------------------------------------------------
// The transport of one communicator: RCCL over xGMI, or the in-process loopback (N contexts on one device, one host thread
// each).  Every collective and point-to-point call of comm_*.cpp goes through it, so the code above this seam -- chunking,
// shard and message arithmetic, stream ordering -- is the same whichever carries the bytes.  Calls between group_begin and
// group_end form one group (RCCL: ncclGroupStart / End; loopback: recorded, executed by group_end, which every member of
// the group reaches with the same sequence of calls).  Streams: everything is enqueued on the communicator's stream.
// ---------------------------------------------------------------------------------------------------------------------
struct Wire {
    lcgs_comm* c;

    lcgs_status loop_failed();
    lcgs_status group_begin();
    lcgs_status rccl_call(ncclResult_t r, const char* what, const char* file, int line);
    lcgs_status allreduce_sum(float* p, size_t count); // in place
    lcgs_status reduce_scatter_sum(const float* send, float* recv, size_t count_per_rank);
    lcgs_status allgather(const float* send, float* recv, size_t count_per_rank);
    lcgs_status send(const void* d_buf, size_t bytes, int peer);
    lcgs_status recv(void* d_buf, size_t bytes, int peer);
    lcgs_status allgather_u32(const uint32_t* d_send, uint32_t* d_recv, size_t count);
    lcgs_status allreduce_max_u32(uint32_t* d_buf, size_t count);
    lcgs_status group_end();
};

// a member of a loopback group that leaves a step early (any error) releases the others from their barriers
struct LoopGuard {
    lcgs_comm* c;
    bool       ok = false;
    ~LoopGuard()
    {
        if (!ok && c && c->loop) c->loop->fail();
    }
};

} // namespace lcgs
