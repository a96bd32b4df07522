// ck_buf.h -- the two owning buffer types of libck_hip.so: DevBuf (HBM) and PinBuf (pinned host memory).
// A buffer frees its memory when it goes, so whatever holds one (ck_ctx, CnnWeights, Mog2State, CkTrainer) needs no
// teardown code of its own.  Both are move-only -- a moved-from buffer is empty -- because the models and trainers of a
// context live in vectors that reallocate.  Growth is reserve(): never shrinks, and the contents do not survive it.
//
// No HIP include: the runtime is reached through the four functions below (0 = success, else the runtime's error number),
// which ck_api.hip defines over the HIP allocator and tools/sanitize/buf_stress.cpp over malloc with counters.
#pragma once
#include <stddef.h>

int ck_dev_alloc(void** p, size_t bytes);
int ck_dev_free(void* p);
int ck_pin_alloc(void** p, size_t bytes, unsigned flags);
int ck_pin_free(void* p);
enum { CK_PIN_DEFAULT = 0, CK_PIN_MAPPED = 2 };      // the runtime's flag values for pinned allocations (checked in ck_api.hip)

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;

    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) { (void)release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { (void)release(); }

    int release()
    {
        const int rc = p ? ck_dev_free(p) : 0;
        p = nullptr; cap = 0;
        return rc;
    }
    // nothing when `bytes` fit; else the old block goes and a block of `want` >= bytes comes.  The caller decides how
    // much headroom `want` has, and waits first for whatever may still be reading the old block.
    int reserve(size_t bytes, size_t want)
    {
        if (bytes <= cap) return 0;
        if (int rc = release()) return rc;
        if (int rc = ck_dev_alloc(&p, want)) { p = nullptr; return rc; }
        cap = want;
        return 0;
    }
};

struct PinBuf {
    void* p = nullptr;
    size_t cap = 0;
    unsigned flags = CK_PIN_DEFAULT;

    explicit PinBuf(unsigned f = CK_PIN_DEFAULT) : flags(f) {}
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    PinBuf(PinBuf&& o) noexcept : p(o.p), cap(o.cap), flags(o.flags) { o.p = nullptr; o.cap = 0; }
    PinBuf& operator=(PinBuf&& o) noexcept
    {
        if (this != &o) { (void)release(); p = o.p; cap = o.cap; flags = o.flags; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~PinBuf() { (void)release(); }

    int release()
    {
        const int rc = p ? ck_pin_free(p) : 0;
        p = nullptr; cap = 0;
        return rc;
    }
    int reserve(size_t bytes, size_t want)               // as DevBuf::reserve
    {
        if (bytes <= cap) return 0;
        if (int rc = release()) return rc;
        if (int rc = ck_pin_alloc(&p, want, flags)) { p = nullptr; return rc; }
        cap = want;
        return 0;
    }
};
