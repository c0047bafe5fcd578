// call_frame.hpp -- the device memory of one C ABI call, and the context's cached buffers.
//
// CallFrame owns what a call allocates: staged copies of host inputs and outputs, and temporaries.
// Its destructor frees them on every path.  In device-pointer mode in() and out() hand the caller's
// pointers through and finish() does nothing: no allocation, no synchronisation, no runtime call.
// CachedBuf is one device buffer that every call on a context shares, ordered across streams by an
// event; DynSlots are the persistent route kernels' work counters.  Both are handed out as leases
// whose destructors record the event, so no return path leaves queued work unordered.
// Runtime API only: no kernels, and plain g++ compiles it (tests/call_frame_driver.cpp).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace ovs {

class CallFrame {
public:
    CallFrame(bool device_ptrs, hipStream_t s) : dev_(device_ptrs), s_(s) {}
    CallFrame(const CallFrame&) = delete;
    CallFrame& operator=(const CallFrame&) = delete;
    ~CallFrame()
    {
        for (int i = 0; i < nown_; ++i) (void)hipFree(own_[i]);
    }

    // The first error sticks: every later request returns nullptr, so a caller asks for all its
    // buffers and checks once before it launches.
    bool ok() const { return err_ == hipSuccess; }
    hipError_t error() const { return err_; }
    const char* what() const { return what_; }

    // a temporary of count elements (at least one), owned in both modes
    template <class T>
    T* scratch(uint64_t count)
    {
        void* d = nullptr;
        if (!ok()) return nullptr;
        if (nown_ == MAX_OWN) { set(hipErrorInvalidValue, "call frame: too many buffers"); return nullptr; }
        if (!set(hipMalloc(&d, sizeof(T) * (count ? count : 1)), "call frame: allocation")) return nullptr;
        own_[nown_++] = d;
        return static_cast<T*>(d);
    }

    // an input: host mode uploads a copy on the frame's stream
    template <class T>
    const T* in(const T* p, uint64_t count)
    {
        if (dev_) return p;
        T* d = scratch<T>(count);
        if (d && count && !set(hipMemcpyAsync(d, p, sizeof(T) * count, hipMemcpyHostToDevice, s_), "call frame: upload"))
            return nullptr;
        return d;
    }

    // an output: host mode allocates it and finish() copies it back to p
    template <class T>
    T* out(T* p, uint64_t count)
    {
        if (dev_) return p;
        T* d = scratch<T>(count);
        if (!d) return nullptr;
        if (nback_ == MAX_BACK) { set(hipErrorInvalidValue, "call frame: too many outputs"); return nullptr; }
        back_[nback_++] = Back{p, d, sizeof(T) * count};
        return d;
    }

    // an array the kernel updates in place: in() and out() of the same copy
    template <class T>
    T* inout(T* p, uint64_t count)
    {
        T* d = out(p, count);
        if (!dev_ && d && count && !set(hipMemcpyAsync(d, p, sizeof(T) * count, hipMemcpyHostToDevice, s_), "call frame: upload"))
            return nullptr;
        return d;
    }

    // copy back only the first count elements of the output d (a kernel that reports how many it wrote)
    template <class T>
    void limit(const T* d, uint64_t count)
    {
        for (int i = 0; i < nback_; ++i)
            if (back_[i].dev == d && sizeof(T) * count < back_[i].bytes) back_[i].bytes = sizeof(T) * count;
    }

    // host mode: the copy-backs and one synchronisation of the stream, after which the outputs are the
    // caller's; nothing is copied once an error stuck.  Device mode: nothing.
    hipError_t finish()
    {
        if (dev_ || !ok()) return err_;
        for (int i = 0; i < nback_; ++i)
            if (back_[i].bytes &&
                !set(hipMemcpyAsync(back_[i].host, back_[i].dev, back_[i].bytes, hipMemcpyDeviceToHost, s_), "call frame: copy-back"))
                return err_;
        set(hipStreamSynchronize(s_), "call frame: synchronize");
        return err_;
    }

private:
    static constexpr int MAX_OWN = 16, MAX_BACK = 8;
    struct Back { void* host; const void* dev; size_t bytes; };

    bool set(hipError_t e, const char* what)
    {
        if (e != hipSuccess && ok()) { err_ = e; what_ = what; }
        return e == hipSuccess;
    }

    const bool dev_;
    const hipStream_t s_;
    hipError_t err_ = hipSuccess;
    const char* what_ = "";
    int nown_ = 0, nback_ = 0;
    void* own_[MAX_OWN];
    Back back_[MAX_BACK];
};

// One device buffer shared by every call on a context.  A call on stream s first waits for the last
// launch that used it (the event, on whichever stream that was) and its lease records its own use
// when it ends, so calls on different streams -- device-pointer calls return while their kernels
// run -- never rewrite each other's rows.  Growing the buffer waits for that last use only, not for
// the whole device.
class CachedBuf {
public:
    class Lease {
    public:
        Lease() = default;
        Lease(Lease&& o) noexcept : b_(o.b_), s_(o.s_), err_(o.err_), what_(o.what_) { o.b_ = nullptr; }
        Lease& operator=(Lease&& o) noexcept
        {
            if (this != &o) {
                release();
                b_ = o.b_; s_ = o.s_; err_ = o.err_; what_ = o.what_;
                o.b_ = nullptr;
            }
            return *this;
        }
        ~Lease() { release(); }

        explicit operator bool() const { return b_ != nullptr; }
        uint8_t* data() const { return b_ ? static_cast<uint8_t*>(b_->p_) : nullptr; }
        hipError_t error() const { return err_; }      // of a failed acquire: which step, and why
        const char* what() const { return what_; }
        // orders the next use of the buffer after the work queued on the lease's stream so far
        void release()
        {
            if (b_ && hipEventRecord(b_->ev_, s_) == hipSuccess) b_->used_ = true;
            b_ = nullptr;
        }

    private:
        friend class CachedBuf;
        Lease(hipError_t e, const char* what) : err_(e), what_(what) {}
        Lease(CachedBuf* b, hipStream_t s) : b_(b), s_(s) {}
        CachedBuf* b_ = nullptr;
        hipStream_t s_ = nullptr;
        hipError_t err_ = hipSuccess;
        const char* what_ = "";
    };

    // at least `bytes` of the buffer for work on stream s; a false lease carries the error
    Lease acquire(uint64_t bytes, hipStream_t s)
    {
        hipError_t e;
        if (!ev_ && (e = hipEventCreateWithFlags(&ev_, hipEventDisableTiming)) != hipSuccess) {
            ev_ = nullptr;
            return Lease(e, "event");
        }
        if (cap_ < bytes) {
            if (p_) {
                if (used_ && (e = hipEventSynchronize(ev_)) != hipSuccess) return Lease(e, "wait");
                free();
            }
            if ((e = hipMalloc(&p_, bytes)) != hipSuccess) { p_ = nullptr; return Lease(e, "allocation"); }
            cap_ = bytes;
        } else if (used_ && (e = hipStreamWaitEvent(s, ev_, 0)) != hipSuccess) {
            return Lease(e, "stream wait");
        }
        return Lease(this, s);
    }

    // drops the buffer (hipFree waits for the launches that use it) and keeps the event
    void free()
    {
        if (p_) (void)hipFree(p_);
        p_ = nullptr; cap_ = 0; used_ = false;
    }

    void destroy()
    {
        free();
        if (ev_) (void)hipEventDestroy(ev_);
        ev_ = nullptr;
    }

private:
    void* p_ = nullptr;
    uint64_t cap_ = 0;
    hipEvent_t ev_ = nullptr;       // recorded after the last launch that used the buffer
    bool used_ = false;
};

// The persistent route kernels' dynamic-tail counters: one 64 B slot per launch, a slot's previous
// launch ordered before its reuse by an event, so concurrent calls on different streams never
// share a counter.
class DynSlots {
public:
    static constexpr int SLOTS = 32;

    class Lease {
    public:
        Lease() = default;
        Lease(Lease&& o) noexcept : d_(o.d_), k_(o.k_), s_(o.s_) { o.d_ = nullptr; }
        Lease& operator=(Lease&&) = delete;
        ~Lease()
        {
            if (!d_) return;
            if (hipEventRecord(d_->ev_[k_], s_) == hipSuccess) d_->used_[k_] = true;
            else (void)hipStreamSynchronize(s_);           // no event: the slot is free once the stream is
        }
        // the zeroed counter; nullptr when none could be had -- the kernel then runs static slices only
        unsigned long long* get() const { return d_ ? d_->base_ + 8 * k_ : nullptr; }

    private:
        friend class DynSlots;
        Lease(DynSlots* d, int k, hipStream_t s) : d_(d), k_(k), s_(s) {}
        DynSlots* d_ = nullptr;
        int k_ = 0;
        hipStream_t s_ = nullptr;
    };

    Lease acquire(hipStream_t s)
    {
        void* b = nullptr;
        if (!base_) {
            if (hipMalloc(&b, 64 * SLOTS) != hipSuccess) return Lease();
            base_ = static_cast<unsigned long long*>(b);
        }
        const int k = (int)(seq_++ % SLOTS);
        if (!ev_[k] && hipEventCreateWithFlags(&ev_[k], hipEventDisableTiming) != hipSuccess) {
            ev_[k] = nullptr;
            return Lease();
        }
        if (used_[k] && hipStreamWaitEvent(s, ev_[k], 0) != hipSuccess) return Lease();
        if (hipMemsetAsync(base_ + 8 * k, 0, sizeof *base_, s) != hipSuccess) return Lease();
        return Lease(this, k, s);
    }

    void destroy()
    {
        for (int i = 0; i < SLOTS; ++i) {
            if (ev_[i]) (void)hipEventDestroy(ev_[i]);
            ev_[i] = nullptr; used_[i] = false;
        }
        if (base_) (void)hipFree(base_);
        base_ = nullptr;
    }

private:
    unsigned long long* base_ = nullptr;
    hipEvent_t ev_[SLOTS] = {};
    bool used_[SLOTS] = {};
    uint32_t seq_ = 0;
};

}  // namespace ovs
