// dev_buf.h -- owning holders for what a Device context allocates: device memory (DevBuf), pinned host memory (PinBuf), events
// and streams.  A holder is its pointer and, for memory, its capacity in elements: there is no second place that says how big a
// buffer is, and nothing to list in a destructor.  Move-only.
//
// The failure contract: after an allocation that failed the holder is EMPTY (get() == nullptr, cap() == 0), the error string is
// set (set_dev_error) and grow() returned false -- so the next call asks again instead of trusting a capacity whose block is gone.
//
// This header names no HIP type (device_backend.h is included by host-only units).  The templates sit on the few functions
// declared first; device_backend.hip defines them with the HIP calls, and a host program may define them with malloc / free
// (tools/host_sanitize/harness.cpp runs the holders under AddressSanitizer that way).
#pragma once
#include <cstddef>
#include <utility>

namespace hnsw {

// nullptr on failure, with the error string set; the free / destroy calls take what these returned (never nullptr)
void *dev_mem_alloc(size_t bytes);
bool dev_mem_free(void *p);
void *pin_mem_alloc(size_t bytes, unsigned flags); // flags: hipHostMalloc's (0 = default)
bool pin_mem_free(void *p);
void *dev_event_create(bool timing);          // timing == false: hipEventDisableTiming
void dev_event_destroy(void *e);
void *dev_stream_create(bool high_priority);  // non-blocking; high_priority: the device's highest stream priority
void dev_stream_destroy(void *s);

struct DevMem {
    static void *alloc(size_t bytes, unsigned) { return dev_mem_alloc(bytes); }
    static bool free(void *p) { return dev_mem_free(p); }
};
struct PinMem {
    static void *alloc(size_t bytes, unsigned flags) { return pin_mem_alloc(bytes, flags); }
    static bool free(void *p) { return pin_mem_free(p); }
};

template <class T, class Mem>
class Buf {
public:
    Buf() = default;
    explicit Buf(unsigned flags) : flags_(flags) {}
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    Buf(Buf &&o) noexcept : p_(o.p_), cap_(o.cap_), flags_(o.flags_), owned_(o.owned_) { o.p_ = nullptr; o.cap_ = 0; o.owned_ = true; }
    Buf &operator=(Buf &&o) noexcept
    {
        if (this != &o) {
            (void)reset();
            p_ = o.p_; cap_ = o.cap_; flags_ = o.flags_; owned_ = o.owned_;
            o.p_ = nullptr; o.cap_ = 0; o.owned_ = true;
        }
        return *this;
    }
    ~Buf() { (void)reset(); }

    T *get() const { return p_; }
    operator T *() const { return p_; }
    size_t cap() const { return cap_; } // elements

    // Room for `need` elements: nothing when need <= cap(); otherwise the old block is freed and `alloc` elements are allocated
    // (contents are not kept).  alloc >= need: for the sites that allocate more than they test for.
    bool grow(size_t need) { return grow(need, need); }
    bool grow(size_t need, size_t alloc)
    {
        if (need <= cap_) return true;
        if (!reset()) return false;
        p_ = static_cast<T *>(Mem::alloc(sizeof(T) * alloc, flags_));
        if (!p_) return false;
        cap_ = alloc;
        return true;
    }
    // Releases the block (an alias only forgets it).  False when the free itself failed; the holder is empty either way.
    bool reset()
    {
        const bool ok = !(p_ && owned_) || Mem::free(p_);
        p_ = nullptr; cap_ = 0; owned_ = true;
        return ok;
    }
    // A non-owning alias of o's block (a view context's rows and graph mirror): never freed here; borrowed again after o grew.
    void borrow(const Buf &o)
    {
        (void)reset();
        p_ = o.p_; cap_ = o.cap_; owned_ = false;
    }

private:
    T *p_ = nullptr;
    size_t cap_ = 0;
    unsigned flags_ = 0;
    bool owned_ = true;
};
template <class T> using DevBuf = Buf<T, DevMem>;
template <class T> using PinBuf = Buf<T, PinMem>;

// Buffers that are replaced together: all released before the first of them is allocated again.
template <class... B>
bool reset_all(B &...b) { return (int(b.reset()) & ...) != 0; }

template <void *(*Create)(bool), void (*Destroy)(void *)>
class Handle {
public:
    Handle() = default;
    Handle(const Handle &) = delete;
    Handle &operator=(const Handle &) = delete;
    Handle(Handle &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Handle &operator=(Handle &&o) noexcept { if (this != &o) { reset(); h_ = o.h_; o.h_ = nullptr; } return *this; }
    ~Handle() { reset(); }
    // created once; `how` is dev_event_create's / dev_stream_create's argument
    bool create(bool how) { if (!h_) h_ = Create(how); return h_ != nullptr; }
    void reset() { if (h_) Destroy(h_); h_ = nullptr; }
    operator void *() const { return h_; }
private:
    void *h_ = nullptr;
};
using DevEvent = Handle<dev_event_create, dev_event_destroy>;
using DevStream = Handle<dev_stream_create, dev_stream_destroy>;

} // namespace hnsw
