// common.hpp -- host-side plumbing shared by the C-ABI translation units.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/lcgs_hip.h"
#include "kernels/gs_math.hpp"

namespace lcgs
{

void        set_last_error(const std::string& msg);
lcgs_status hip_fail(hipError_t e, const char* what, const char* file, int line);

#define LCGS_HIP_CHECK(expr)                                                       \
    do {                                                                           \
        hipError_t _e = (expr);                                                    \
        if (_e != hipSuccess) return ::lcgs::hip_fail(_e, #expr, __FILE__, __LINE__); \
    } while (0)

#define LCGS_REQUIRE(cond, msg)                                  \
    do {                                                         \
        if (!(cond)) {                                           \
            ::lcgs::set_last_error(std::string("invalid argument: ") + (msg)); \
            return LCGS_ERR_INVALID_ARG;                         \
        }                                                        \
    } while (0)

// The one ownership rule of the host code: a member or local that owns a device resource releases it in its destructor.
// The owning types below are move-only (a move leaves the source empty); one that BORROWS somebody else's resource never
// releases it.  None may live at namespace scope: their destructors call into the HIP runtime.  (Bodies: device_owned.cpp.)

// A device allocation that only ever grows (geometric growth, like the reference's
// ensure_*_temp_buffer, lcgs/src/gs_tile_splatter/impl.cpp:31-61).
struct DeviceBuffer {
    void*  ptr   = nullptr;
    size_t bytes = 0;
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer&& o) noexcept : ptr(o.ptr), bytes(o.bytes), borrowed(o.borrowed) { o.forget(); }
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept
    {
        if (this != &o) {
            release();
            ptr = o.ptr, bytes = o.bytes, borrowed = o.borrowed;
            o.forget();
        }
        return *this;
    }
    DeviceBuffer(const DeviceBuffer&)            = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    ~DeviceBuffer() { release(); }
    lcgs_status ensure(size_t need); // (on a borrowed buffer: LCGS_ERR_STATE, the lender's memory is not touched)
    void        release();
    // reads the lender's memory where it lies now: never grown or freed through this buffer
    void borrow(const DeviceBuffer& lender)
    {
        release();
        ptr = lender.ptr, bytes = lender.bytes, borrowed = true;
    }
    template <typename T>
    T* as() const { return reinterpret_cast<T*>(ptr); }

private:
    bool borrowed = false;
    void forget() { ptr = nullptr, bytes = 0, borrowed = false; }
};

// An event, a stream or a pinned host block: owned (made by ensure()) or borrowed; converts to the raw handle for the HIP calls.
template <typename H, void (*Drop)(H)>
struct Handle {
    Handle() = default;
    Handle(Handle&& o) noexcept : h(o.h), borrowed(o.borrowed) { o.forget(); }
    Handle& operator=(Handle&& o) noexcept
    {
        if (this != &o) {
            release();
            h = o.h, borrowed = o.borrowed;
            o.forget();
        }
        return *this;
    }
    Handle(const Handle&)            = delete;
    Handle& operator=(const Handle&) = delete;
    ~Handle() { release(); }
    void release()
    {
        if (h && !borrowed) Drop(h);
        forget();
    }
    void borrow(H other)
    {
        release();
        h = other, borrowed = true;
    }
    operator H() const { return h; }

protected:
    H    h        = nullptr;
    bool borrowed = false;
    void forget() { h = nullptr, borrowed = false; }
};
void drop_event(hipEvent_t ev);
void drop_stream(hipStream_t st);
void drop_pinned(void* p);
struct Event : Handle<hipEvent_t, drop_event> {
    lcgs_status ensure(unsigned flags = hipEventDisableTiming); // (the profiling marks ask for the timing kind: 0)
};
struct Stream : Handle<hipStream_t, drop_stream> {
    lcgs_status ensure();                      // non-blocking, default priority
    lcgs_status ensure_priority(int priority); // ... with this priority where the device grants it
};
lcgs_status ensure_pinned(void** p, size_t bytes, unsigned flags);
template <typename T>
void drop_pinned_as(T* p) { drop_pinned(p); }
template <typename T>
struct Pinned : Handle<T*, drop_pinned_as<T>> { // a block of fixed size
    lcgs_status ensure(size_t bytes, unsigned flags = hipHostMallocDefault)
    {
        return ensure_pinned(reinterpret_cast<void**>(&this->h), bytes, flags);
    }
};

// host camera -> kernel constants (lcgs/src/gs_projector/impl.cpp:34-42, util/camera.h:38-72)
CamParams make_cam_params(const lcgs_camera& cam);

// stream of an (opaque) context, for translation units that only see the forward declaration
hipStream_t context_stream(lcgs_context* ctx);
int         context_device(lcgs_context* ctx);
void        context_count_call(lcgs_context* ctx);
// Every C ABI entry point that takes a context says LCGS_ENTRY(ctx) in front of its first use of the context (behind the
// argument checks that refuse a call before the context is read): the per-context operation count by which a pipelined
// forward frame knows that nothing else was asked of the context since the frame before it (context.hpp op_seq).  An entry
// point without it could race with a chained frame's head; tests/test_abi_entry_count.py reads the sources for it.
#define LCGS_ENTRY(ctx)                                \
    do {                                               \
        if (ctx) lcgs::context_count_call(ctx);        \
    } while (0)

// what the device ingest path needs to know about a PLY file (host/ply.cpp)
struct PlyProbe {
    int64_t  num_vertices = 0;
    size_t   stride = 0, payload_offset = 0;
    uint32_t column_offset[59] = {};
    bool     device_ok = false;
};
lcgs_status ply_probe(const char* path, PlyProbe* out);

inline uint32_t div_up(uint32_t a, uint32_t b) { return (a + b - 1u) / b; }
inline int64_t  div_up64(int64_t a, int64_t b) { return (a + b - 1) / b; }

} // namespace lcgs
