// dst_owner.h — the one owner of every device and page-locked allocation (Grown) and of every ordering event (Event) of
// the library: the context's buffers (dst_ctx.h), a set's (DeviceSet, dst_internal.h), a stream's slots and a call's own.
// grow() and release() are in dst_api.cpp; nothing here is called by the host-only code (dst_host.cpp).
#pragma once
#include <cstddef>
#include <utility>

#include <hip/hip_runtime.h>

struct dst_ctx;

namespace dst {

// Device memory, or page-locked host memory.  Grow-only between uses: grow() keeps what is big enough, else frees and
// allocates exactly `want` bytes (a caller that wants slack asks for it).  A failure leaves it empty (capacity 0), with
// the runtime's sticky error cleared.  Without `what` it is reported as the runtime's (fail_hip: DST_ERR_NOMEM or
// DST_ERR_HIP); `what` names the caller in a refusal that is always DST_ERR_NOMEM ("links: cannot allocate N bytes of
// page-locked memory", "neighbour joining: cannot allocate N bytes of device memory").  Released when its owner goes —
// a context (dst_destroy has waited for the device by then), a set (free_set), a call (behind its wait for its stream) —
// so a new buffer is one member or local and its grow() calls, nothing else.
struct GrownBase {
    void *ptr = nullptr;
    size_t bytes = 0;   // capacity
    const bool pinned;
    explicit GrownBase(bool pinned_) : pinned(pinned_) {}
    GrownBase(GrownBase &&o) noexcept : ptr(o.ptr), bytes(o.bytes), pinned(o.pinned) { o.ptr = nullptr, o.bytes = 0; }
    GrownBase &operator=(GrownBase &&o) noexcept
    {
        std::swap(ptr, o.ptr);   // (both of one kind: what was here goes with `o`)
        std::swap(bytes, o.bytes);
        return *this;
    }
    ~GrownBase() { (void)release(); }
    int grow(dst_ctx *ctx, size_t want, const char *what = nullptr);
    hipError_t release();
};
template <typename T = void, bool kPinned = false>
struct Grown : GrownBase {
    Grown() : GrownBase(kPinned) {}
    operator T *() const { return static_cast<T *>(ptr); }
};

// An ordering event (no timing): made by its first record, destroyed with its owner.
struct Event {
    hipEvent_t e = nullptr;   // NULL: never recorded, nothing to wait for
    Event() = default;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    Event &operator=(Event &&o) noexcept
    {
        std::swap(e, o.e);
        return *this;
    }
    ~Event()
    {
        if (e)
            (void)hipEventDestroy(e);
    }
    hipError_t record(hipStream_t stream)
    {
        if (!e)
            if (const hipError_t err = hipEventCreateWithFlags(&e, hipEventDisableTiming))
                return err;
        return hipEventRecord(e, stream);
    }
    operator hipEvent_t() const { return e; }
};

}  // namespace dst
