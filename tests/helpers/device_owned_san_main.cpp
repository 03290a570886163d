// Sanitizer driver for the owning types of csrc/common.hpp (tests/test_device_owned_sanitizers.py builds it with the product's
// csrc/device_owned.cpp under -fsanitize=address,undefined).  TEST HELPER, not part of the product library.
// The HIP calls the holders make are stand-ins over malloc / free that count live objects: a double free, a use after a move,
// a leak or a freed lender shows up in the counts, or in the sanitizer's report.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <type_traits>
#include <utility>

#include "../../luisacomputegaussiansplatting_amd/csrc/device_owned.cpp"

namespace lcgs
{
static std::string g_err;
void        set_last_error(const std::string& m) { g_err = m; }
lcgs_status hip_fail(hipError_t e, const char* what, const char*, int)
{
    g_err = what;
    return e == hipErrorOutOfMemory ? LCGS_ERR_OUT_OF_MEMORY : LCGS_ERR_HIP;
}
} // namespace lcgs

static int  live_dev = 0, live_pinned = 0, live_events = 0, live_streams = 0, frees_dev = 0;
static bool fail_malloc = false, fail_priority = false;
static unsigned last_pinned_flags = 0, last_event_flags = ~0u;

extern "C" {
hipError_t hipMalloc(void** p, size_t n)
{
    if (fail_malloc) return hipErrorOutOfMemory;
    *p = malloc(n);
    ++live_dev;
    return hipSuccess;
}
hipError_t hipFree(void* p)
{
    free(p);
    --live_dev, ++frees_dev;
    return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t n, unsigned flags)
{
    *p = malloc(n);
    ++live_pinned, last_pinned_flags = flags;
    return hipSuccess;
}
hipError_t hipHostFree(void* p)
{
    free(p);
    --live_pinned;
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags)
{
    *e = static_cast<hipEvent_t>(malloc(1));
    ++live_events, last_event_flags = flags;
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* e) { return hipEventCreateWithFlags(e, 0); }
hipError_t hipEventDestroy(hipEvent_t e)
{
    free(e);
    --live_events;
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned)
{
    *s = static_cast<hipStream_t>(malloc(1));
    ++live_streams;
    return hipSuccess;
}
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned flags, int)
{
    return fail_priority ? hipErrorInvalidValue : hipStreamCreateWithFlags(s, flags);
}
hipError_t hipStreamDestroy(hipStream_t s)
{
    free(s);
    --live_streams;
    return hipSuccess;
}
hipError_t hipMemset(void* p, int v, size_t n)
{
    memset(p, v, n);
    return hipSuccess;
}
hipError_t hipDeviceSynchronize(void) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
}

using namespace lcgs;

static_assert(!std::is_copy_constructible_v<DeviceBuffer> && !std::is_copy_assignable_v<DeviceBuffer>, "DeviceBuffer copies");
static_assert(!std::is_copy_constructible_v<Event> && !std::is_copy_assignable_v<Event>, "Event copies");
static_assert(!std::is_copy_constructible_v<Stream> && !std::is_copy_assignable_v<Stream>, "Stream copies");
static_assert(!std::is_copy_constructible_v<Pinned<uint32_t>> && !std::is_copy_assignable_v<Pinned<uint32_t>>, "Pinned copies");
static_assert(std::is_nothrow_move_constructible_v<DeviceBuffer> && std::is_nothrow_move_constructible_v<Event>, "moves");

static int failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            ++failures;                                               \
        }                                                             \
    } while (0)

static void test_buffer()
{
    {
        DeviceBuffer b;
        CHECK(b.ensure(100) == LCGS_OK && b.ptr && b.bytes == 256 && live_dev == 1); // 256-byte rounding
        memset(b.ptr, 1, b.bytes);
        void* first = b.ptr;
        CHECK(b.ensure(200) == LCGS_OK && b.ptr == first && frees_dev == 0); // fits: nothing happens
        CHECK(b.ensure(300) == LCGS_OK && b.bytes == 512 && live_dev == 1 && frees_dev == 1); // grown (x 2): old block freed once
        CHECK(b.ensure(5000) == LCGS_OK && b.bytes == 5120 && live_dev == 1 && frees_dev == 2);
        memset(b.ptr, 2, b.bytes);
        CHECK(b.as<char>() == b.ptr);
        b.release();
        b.release(); // twice is harmless
        CHECK(!b.ptr && b.bytes == 0 && live_dev == 0 && frees_dev == 3);
        CHECK(b.ensure(16) == LCGS_OK && live_dev == 1); // usable again
    }
    CHECK(live_dev == 0); // scope end frees
    { // moves: one owner
        DeviceBuffer a;
        CHECK(a.ensure(64) == LCGS_OK);
        void*        p = a.ptr;
        DeviceBuffer b(std::move(a));
        CHECK(!a.ptr && a.bytes == 0 && b.ptr == p && b.bytes == 256 && live_dev == 1);
        DeviceBuffer c;
        CHECK(c.ensure(64) == LCGS_OK && live_dev == 2);
        const int before = frees_dev;
        c = std::move(b); // onto a non-empty target: the target's block goes
        CHECK(!b.ptr && c.ptr == p && live_dev == 1 && frees_dev == before + 1);
        DeviceBuffer& self = c;
        c = std::move(self);
        CHECK(c.ptr == p && live_dev == 1);
        CHECK(a.ensure(32) == LCGS_OK && live_dev == 2); // a moved-from buffer is an empty one
    }
    CHECK(live_dev == 0);
    { // borrowing
        DeviceBuffer lender;
        CHECK(lender.ensure(1000) == LCGS_OK);
        {
            DeviceBuffer view;
            view.borrow(lender);
            CHECK(view.ptr == lender.ptr && view.bytes == lender.bytes && live_dev == 1);
            CHECK(view.ensure(10) != LCGS_OK && view.ensure(1 << 20) != LCGS_OK); // never grown through the borrower
            CHECK(view.ptr == lender.ptr && live_dev == 1);
            memset(lender.ptr, 3, lender.bytes); // (alive: the sanitizer would say otherwise)
            DeviceBuffer moved(std::move(view)); // a moved borrower still borrows
            CHECK(moved.ptr == lender.ptr && !view.ptr);
            moved.release();
            CHECK(!moved.ptr && live_dev == 1);
            view.borrow(lender);
            view.borrow(lender); // again (every camera batch does)
            DeviceBuffer own;
            CHECK(own.ensure(8) == LCGS_OK && live_dev == 2);
            own.borrow(lender); // what it owned goes first
            CHECK(live_dev == 1);
        } // scope end of three borrowers
        CHECK(live_dev == 1);
        memset(lender.ptr, 4, lender.bytes);
    }
    CHECK(live_dev == 0);
    { // a failed allocation: empty, and a status
        DeviceBuffer b;
        fail_malloc = true;
        CHECK(b.ensure(64) == LCGS_ERR_OUT_OF_MEMORY && !b.ptr && b.bytes == 0 && live_dev == 0);
        fail_malloc = false;
        CHECK(b.ensure(64) == LCGS_OK);
        fail_malloc = true; // growth that fails: the old block is gone, the buffer is empty, nothing is freed twice
        CHECK(b.ensure(4096) == LCGS_ERR_OUT_OF_MEMORY && !b.ptr && b.bytes == 0 && live_dev == 0);
        fail_malloc = false;
    }
    CHECK(live_dev == 0);
}

static void test_handles()
{
    {
        Event e;
        CHECK(!e && live_events == 0);
        CHECK(e.ensure() == LCGS_OK && e && live_events == 1 && last_event_flags == hipEventDisableTiming);
        hipEvent_t raw = e; // converts to the raw handle
        CHECK(e.ensure() == LCGS_OK && e == raw && live_events == 1); // made once
        Event t;
        CHECK(t.ensure(0) == LCGS_OK && last_event_flags == 0u && live_events == 2); // the timing kind
        Event m(std::move(e));
        CHECK(!e && m == raw && live_events == 2);
        t = std::move(m); // the target's event goes
        CHECK(!m && t == raw && live_events == 1);
        {
            Event view;
            view.borrow(t);
            CHECK(view == raw);
            view.release();
            view.release();
            CHECK(live_events == 1);
            view.borrow(t);
        }
        CHECK(live_events == 1);
        Event arr[4]; // (arrays of members: ev_slice[], events[])
        for (Event& a : arr) CHECK(a.ensure() == LCGS_OK);
        CHECK(live_events == 5);
    }
    CHECK(live_events == 0);
    {
        Stream s, lo;
        CHECK(s.ensure() == LCGS_OK && s && live_streams == 1);
        CHECK(lo.ensure_priority(3) == LCGS_OK && lo && live_streams == 2);
        hipStream_t raw = lo;
        CHECK(lo.ensure_priority(3) == LCGS_OK && lo == raw && live_streams == 2);
        Stream fb;
        fail_priority = true; // no priorities on this device: a plain stream
        CHECK(fb.ensure_priority(3) == LCGS_OK && fb && live_streams == 3);
        fail_priority = false;
        {
            Stream sibling; // the batch sibling's auxiliary stream
            sibling.borrow(lo);
            CHECK(sibling == raw && sibling.ensure() == LCGS_OK && sibling == raw && live_streams == 3);
            Stream moved(std::move(sibling));
            CHECK(!sibling && moved == raw);
            moved.release();
            CHECK(!moved && live_streams == 3);
            sibling.borrow(lo);
        }
        CHECK(live_streams == 3);
        s = std::move(fb);
        CHECK(live_streams == 2 && !fb);
    }
    CHECK(live_streams == 0);
    {
        Pinned<uint32_t> h;
        CHECK(!h && h.ensure(64, hipHostMallocCoherent | hipHostMallocMapped) == LCGS_OK && h && live_pinned == 1);
        CHECK(last_pinned_flags == (hipHostMallocCoherent | hipHostMallocMapped));
        uint32_t* raw = h;
        h[3] = h[15] = 7u;
        CHECK(raw[3] == 7u && *(h + 15) == 7u);
        CHECK(h.ensure(64) == LCGS_OK && h == raw && live_pinned == 1); // allocated once
        Pinned<uint32_t> m(std::move(h));
        CHECK(!h && m == raw && live_pinned == 1);
        Pinned<unsigned char> b;
        CHECK(b.ensure(10) == LCGS_OK && last_pinned_flags == hipHostMallocDefault && live_pinned == 2);
        b.release();
        b.release();
        CHECK(live_pinned == 1);
    }
    CHECK(live_pinned == 0);
}

int main()
{
    test_buffer();
    test_handles();
    CHECK(live_dev == 0 && live_pinned == 0 && live_events == 0 && live_streams == 0);
    printf("failures %d\n", failures);
    return failures ? 1 : 0;
}
