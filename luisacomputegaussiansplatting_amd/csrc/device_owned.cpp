// device_owned.cpp -- the bodies of the owning types of common.hpp: the only place of the library that frees device memory,
// pinned memory, events or streams.  Knows nothing of the context (tests/helpers/device_owned_san_main.cpp links it alone).
#include <stdlib.h>

#include <algorithm>

#include "common.hpp"

namespace lcgs
{

lcgs_status DeviceBuffer::ensure(size_t need)
{
    if (borrowed) {
        set_last_error("internal error: a borrowed device buffer was asked to grow");
        return LCGS_ERR_STATE;
    }
    if (need <= bytes) return LCGS_OK;
    // geometric growth, like ensure_*_temp_buffer (lcgs/src/gs_tile_splatter/impl.cpp:38-41)
    size_t new_bytes = bytes == 0 ? need : std::max(need, bytes * 2);
    new_bytes        = (new_bytes + 255) & ~(size_t)255;
    if (ptr) {
        LCGS_HIP_CHECK(hipFree(ptr));
        forget();
    }
    if (const hipError_t e = hipMalloc(&ptr, new_bytes); e != hipSuccess) {
        ptr = nullptr; // (empty, whatever the failed call left there)
        return hip_fail(e, "hipMalloc(&ptr, new_bytes)", __FILE__, __LINE__);
    }
    bytes = new_bytes;
    // test hook: fresh workspace starts as garbage instead of whatever the allocator hands out (usually zeros), so
    // that a kernel reading what no kernel wrote shows up in the parity tests
    static const bool poison = getenv("LCGS_POISON") != nullptr;
    if (poison) {
        LCGS_HIP_CHECK(hipMemset(ptr, 0xA5, new_bytes)); // (legacy stream: not ordered against non-blocking streams,
        LCGS_HIP_CHECK(hipDeviceSynchronize());          //  so finish it before anybody writes real data)
    }
    return LCGS_OK;
}

void DeviceBuffer::release()
{
    if (ptr && !borrowed) (void)hipFree(ptr);
    forget();
}

void drop_event(hipEvent_t ev) { (void)hipEventDestroy(ev); }
void drop_stream(hipStream_t st) { (void)hipStreamDestroy(st); }
void drop_pinned(void* p) { (void)hipHostFree(p); }

lcgs_status Event::ensure(unsigned flags)
{
    if (!h) LCGS_HIP_CHECK(flags ? hipEventCreateWithFlags(&h, flags) : hipEventCreate(&h));
    return LCGS_OK;
}

lcgs_status Stream::ensure()
{
    if (!h) LCGS_HIP_CHECK(hipStreamCreateWithFlags(&h, hipStreamNonBlocking));
    return LCGS_OK;
}

lcgs_status Stream::ensure_priority(int priority)
{
    if (!h && hipStreamCreateWithPriority(&h, hipStreamNonBlocking, priority) != hipSuccess) {
        (void)hipGetLastError();
        h = nullptr;
    }
    return ensure();
}

lcgs_status ensure_pinned(void** p, size_t bytes, unsigned flags)
{
    if (!*p) LCGS_HIP_CHECK(hipHostMalloc(p, bytes, flags));
    return LCGS_OK;
}

} // namespace lcgs
