// call_frame_driver.cpp -- oversim_amd/csrc/call_frame.hpp against a fake HIP runtime, under ASan/UBSan
// (tests/test_sanitizers.py).  The fakes below stand in for the runtime functions the header calls:
// device memory is host memory, a copy is a memcpy, every call is counted, and the k-th call whose
// result the header can report may be told to fail.  hipFree, hipEventDestroy and hipEventRecord
// clean up or close a lease; nothing can be reported from there, so they are counted and never fail.
//
// One call in the shape of a C ABI entry point (2 inputs, 2 outputs, 1 temporary, a lease of the
// cached buffer, finish) runs in host mode with every k failing in turn: each run must report an
// error, free every allocation, record the event of every lease it got and leave the caller's
// outputs untouched.  The same call in device-pointer mode must not touch the runtime at all.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

#include "call_frame.hpp"

namespace {

std::set<void*> g_live;          // fake device allocations and events not yet freed
long g_calls = 0;                // reportable runtime calls so far
long g_fail_at = 0;              // the reportable call that fails (0: none)
long g_all = 0;                  // every runtime call, cleanup included
long g_mallocs = 0, g_frees = 0, g_records = 0, g_stream_waits = 0, g_event_syncs = 0, g_stream_syncs = 0, g_d2h = 0;
int g_bad = 0;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_bad; } \
    } while (0)

bool fails()
{
    ++g_all;
    return ++g_calls == g_fail_at;
}

void* fake_alloc(size_t bytes)
{
    void* p = std::malloc(bytes ? bytes : 1);
    g_live.insert(p);
    return p;
}

void fake_free(void* p)
{
    CHECK(g_live.erase(p) == 1);          // freed once, and only what the fakes handed out
    std::free(p);
}

void reset(long fail_at)
{
    g_calls = g_all = 0;
    g_fail_at = fail_at;
    g_mallocs = g_frees = g_records = g_stream_waits = g_event_syncs = g_stream_syncs = g_d2h = 0;
}

}  // namespace

extern "C" {

hipError_t hipMalloc(void** p, size_t bytes)
{
    if (fails()) return hipErrorOutOfMemory;
    ++g_mallocs;
    *p = fake_alloc(bytes);
    return hipSuccess;
}

hipError_t hipFree(void* p)
{
    ++g_all; ++g_frees;
    fake_free(p);
    return hipSuccess;
}

hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t)
{
    if (fails()) return hipErrorUnknown;
    if (kind == hipMemcpyDeviceToHost) ++g_d2h;
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}

hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t)
{
    if (fails()) return hipErrorUnknown;
    std::memset(dst, value, bytes);
    return hipSuccess;
}

hipError_t hipStreamSynchronize(hipStream_t)
{
    if (fails()) return hipErrorUnknown;
    ++g_stream_syncs;
    return hipSuccess;
}

hipError_t hipEventCreateWithFlags(hipEvent_t* ev, unsigned)
{
    if (fails()) return hipErrorUnknown;
    *ev = static_cast<hipEvent_t>(fake_alloc(1));
    return hipSuccess;
}

hipError_t hipEventDestroy(hipEvent_t ev)
{
    ++g_all;
    fake_free(ev);
    return hipSuccess;
}

hipError_t hipEventRecord(hipEvent_t ev, hipStream_t)
{
    ++g_all; ++g_records;
    CHECK(g_live.count(ev) == 1);
    return hipSuccess;
}

hipError_t hipEventSynchronize(hipEvent_t ev)
{
    if (fails()) return hipErrorUnknown;
    ++g_event_syncs;
    CHECK(g_live.count(ev) == 1);
    return hipSuccess;
}

hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t ev, unsigned)
{
    if (fails()) return hipErrorUnknown;
    ++g_stream_waits;
    CHECK(g_live.count(ev) == 1);
    return hipSuccess;
}

}  // extern "C"

namespace {

using ovs::CachedBuf;
using ovs::CallFrame;
using ovs::DynSlots;

constexpr uint64_t N = 37;
const hipStream_t S1 = reinterpret_cast<hipStream_t>(0x10), S2 = reinterpret_cast<hipStream_t>(0x20);

struct Arrays {
    uint32_t a[N], x[N];
    uint64_t b[N], y[N];
    Arrays()
    {
        for (uint64_t i = 0; i < N; ++i) { a[i] = (uint32_t)(3 * i + 1); b[i] = 1000 + i; x[i] = 0xDEADBEEFu; y[i] = ~0ull; }
    }
    bool outputs_untouched() const
    {
        for (uint64_t i = 0; i < N; ++i)
            if (x[i] != 0xDEADBEEFu || y[i] != ~0ull) return false;
        return true;
    }
    bool outputs_right() const
    {
        for (uint64_t i = 0; i < N; ++i)
            if (x[i] != 2 * a[i] + 7 || y[i] != b[i] + a[i]) return false;
        return true;
    }
};

// the "kernel": x = 2 a + 7 through a temporary and the cached buffer, y = b + a
void kernel(const uint32_t* a, const uint64_t* b, uint32_t* x, uint64_t* y, uint32_t* tmp, uint32_t* cached)
{
    for (uint64_t i = 0; i < N; ++i) {
        uint32_t v = 2 * a[i];
        if (tmp) { tmp[i] = v; v = tmp[i]; }
        if (cached) { cached[i] = v + 7; v = cached[i]; } else v += 7;
        x[i] = v;
        y[i] = b[i] + a[i];
    }
}

// one call as the entry points of ovs_route.cpp make it; *leases counts the leases it got
hipError_t call(bool dev, CachedBuf* cache, Arrays& h, int* leases)
{
    CallFrame F(dev, S1);
    CachedBuf::Lease vis;
    const uint32_t* a = F.in(h.a, N);
    const uint64_t* b = F.in(h.b, N);
    uint32_t* x = F.out(h.x, N);
    uint64_t* y = F.out(h.y, N);
    uint32_t* tmp = dev ? nullptr : F.scratch<uint32_t>(N);
    if (!F.ok()) return F.error();
    if (cache) {
        vis = cache->acquire(sizeof(uint32_t) * N, S1);
        if (!vis) return vis.error();
        ++*leases;
    }
    kernel(a, b, x, y, tmp, reinterpret_cast<uint32_t*>(vis.data()));
    vis.release();
    return F.finish();
}

void test_host_mode_failures()
{
    // a clean run: 5 allocations + 2 uploads, the lease (event, allocation), 2 copy-backs, 1 synchronise
    long clean = 0;
    {
        CachedBuf cache;
        Arrays h;
        int leases = 0;
        reset(0);
        CHECK(call(false, &cache, h, &leases) == hipSuccess);
        clean = g_calls;
        CHECK(clean == 12);
        CHECK(h.outputs_right());
        CHECK(g_mallocs == 6 && g_frees == 5 && g_d2h == 2 && g_stream_syncs == 1);
        CHECK(leases == 1 && g_records == 1);
        cache.destroy();
        CHECK(g_live.empty());
    }
    for (long k = 1; k <= clean; ++k) {
        CachedBuf cache;
        Arrays h;
        int leases = 0;
        reset(k);
        const hipError_t e = call(false, &cache, h, &leases);
        CHECK(e != hipSuccess);                          // reported
        CHECK(g_calls >= k);                             // ... because call k was reached
        CHECK(g_records == leases);                      // every lease recorded its event
        // no copy-back is issued after a failure: the outputs stay the caller's, unless it is the
        // second copy-back or the final synchronise itself that fails
        CHECK(k == clean || (g_d2h < 2 && g_stream_syncs == 0));
        CHECK(k > clean - 2 || (g_d2h == 0 && h.outputs_untouched()));
        cache.destroy();
        CHECK(g_live.empty());                           // every allocation freed
    }
    // a second call on a warm cache fails in every place too (the lease then waits on the event)
    for (long k = 1; k <= clean; ++k) {
        CachedBuf cache;
        Arrays h0, h;
        int leases = 0;
        reset(0);
        CHECK(call(false, &cache, h0, &leases) == hipSuccess);
        const long rec0 = g_records;
        reset(k);
        leases = 0;
        const hipError_t e = call(false, &cache, h, &leases);
        if (g_calls >= k) CHECK(e != hipSuccess);
        else CHECK(e == hipSuccess && h.outputs_right());    // the warm call makes fewer calls than k
        CHECK(g_records == leases && rec0 == 1);
        cache.destroy();
        CHECK(g_live.empty());
    }
}

void test_device_mode_is_free()
{
    Arrays h;
    int leases = 0;
    reset(0);
    CHECK(call(true, nullptr, h, &leases) == hipSuccess);
    CHECK(g_all == 0);                                   // no runtime call of any kind
    CHECK(h.outputs_right());                            // the caller's pointers went through
    CHECK(g_live.empty());
}

void test_limit_and_inout()
{
    uint32_t host[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    reset(0);
    {
        CallFrame F(false, S1);
        uint32_t* d = F.inout(host, 8);
        CHECK(F.ok() && d && d != host && d[3] == 4);
        for (int i = 0; i < 8; ++i) d[i] += 10;
        F.limit(d, 3);                                   // the kernel reported 3 elements
        CHECK(F.finish() == hipSuccess);
    }
    CHECK(host[0] == 11 && host[2] == 13 && host[3] == 4 && host[7] == 8);
    CHECK(g_live.empty());
    // an empty array still gets a (one-element) buffer and no copy
    reset(0);
    {
        CallFrame F(false, S1);
        const uint32_t* d = F.in(host, 0);
        CHECK(F.ok() && d);
        CHECK(g_calls == 1);
    }
    CHECK(g_live.empty());
    // more buffers than a frame holds: an error, not an overrun
    reset(0);
    {
        CallFrame F(false, S1);
        for (int i = 0; i < 40; ++i) F.scratch<uint8_t>(4);
        CHECK(!F.ok() && F.error() == hipErrorInvalidValue);
        CHECK(F.finish() != hipSuccess);
    }
    CHECK(g_live.empty());
}

// the cached buffer as kvis uses it: kept while large enough, grown after the last use only
void test_cached_buffer_growth()
{
    CachedBuf cache;
    reset(0);
    uint8_t* p1;
    {
        CachedBuf::Lease l = cache.acquire(100, S1);
        CHECK(l && l.data());
        p1 = l.data();
        CHECK(g_mallocs == 1 && g_stream_waits == 0 && g_event_syncs == 0);    // first use: nothing to wait for
    }
    CHECK(g_records == 1);
    {
        CachedBuf::Lease l = cache.acquire(50, S2);      // fits: the same buffer, after the event
        CHECK(l && l.data() == p1);
        CHECK(g_mallocs == 1 && g_stream_waits == 1 && g_event_syncs == 0);
        CachedBuf::Lease m(static_cast<CachedBuf::Lease&&>(l));               // a moved lease records once
        CHECK(!l && m);
    }
    CHECK(g_records == 2);
    {
        CachedBuf::Lease l = cache.acquire(200, S1);     // grows: waits for the last use, frees, allocates
        CHECK(l);
        CHECK(g_mallocs == 2 && g_frees == 1 && g_event_syncs == 1 && g_stream_waits == 1);
    }
    CHECK(g_records == 3);
    cache.free();                                        // as free_tables: the event stays
    CHECK(g_live.size() == 1);
    {
        CachedBuf::Lease l = cache.acquire(10, S1);      // a fresh buffer has no last use
        CHECK(l && g_mallocs == 3 && g_event_syncs == 1 && g_stream_waits == 1);
    }
    cache.destroy();
    CHECK(g_live.empty());
}

void test_dyn_slots()
{
    // a clean first lease: the slots' allocation, the slot's event, the counter's memset
    long clean = 0;
    {
        DynSlots dyn;
        reset(0);
        {
            DynSlots::Lease l = dyn.acquire(S1);
            CHECK(l.get() != nullptr && *l.get() == 0);
            *l.get() = 99;
        }
        clean = g_calls;
        CHECK(clean == 3 && g_records == 1);
        // the slot comes round again after SLOTS leases: ordered by its event, zeroed again
        for (int i = 1; i < DynSlots::SLOTS; ++i) { DynSlots::Lease l = dyn.acquire(S1); CHECK(l.get()); }
        CHECK(g_stream_waits == 0);
        {
            DynSlots::Lease l = dyn.acquire(S2);
            CHECK(l.get() && *l.get() == 0 && g_stream_waits == 1);
        }
        CHECK(g_records == DynSlots::SLOTS + 1);
        dyn.destroy();
        CHECK(g_live.empty());
    }
    // a failure anywhere gives no counter (the kernel runs static slices) and records nothing
    for (long k = 1; k <= clean; ++k) {
        DynSlots dyn;
        reset(k);
        {
            DynSlots::Lease l = dyn.acquire(S1);
            CHECK(l.get() == nullptr);
        }
        CHECK(g_records == 0);
        dyn.destroy();
        CHECK(g_live.empty());
    }
}

}  // namespace

int main()
{
    test_host_mode_failures();
    test_device_mode_is_free();
    test_limit_and_inout();
    test_cached_buffer_growth();
    test_dyn_slots();
    if (g_bad) { std::printf("%d checks failed\n", g_bad); return 1; }
    std::printf("call frame clean\n");
    return 0;
}
