// The two ways the engine's host side owns device memory outside lob_create's allocation list: a buffer that only grows, kept
// across calls (GrowBuf), and one that lives for a single call (ScopedBuf).  The allocator is a parameter -- `A::alloc(void**, bytes)`
// returns 0 on success and leaves no error behind on failure, `A::free(void*)` -- so that tests/host_env/devbuf_test.cpp drives
// both over a counting allocator on the CPU; the engine's is HipAlloc (lob_engine_impl.h).  No HIP in this header.
#ifndef LOB_DEVBUF_H
#define LOB_DEVBUF_H

#include <stddef.h>

#include "../../include/lob_engine.h"

namespace lob {

// `cap` counts elements.  reserve() never touches the buffer when it is large enough; when it must grow, the old buffer is gone
// and {p, cap} are {null, 0} BEFORE the allocation is tried, and stay so when it fails: nothing can be launched into, or freed
// twice from, a failed growth, and the next call allocates afresh.
template <class T, class A> struct GrowBuf {
    T* p = nullptr;
    size_t cap = 0;
    int reserve(size_t need) {
        if (need <= cap) return LOB_OK;
        release();
        void* q = nullptr;
        if (A::alloc(&q, need * sizeof(T)) != 0) return LOB_ENOMEM;
        p = (T*)q;
        cap = need;
        return LOB_OK;
    }
    void release() {
        if (p) A::free(p);
        p = nullptr;
        cap = 0;
    }
};

// Freed on every way out of the scope it is declared in.
template <class T, class A> struct ScopedBuf {
    T* p = nullptr;
    ScopedBuf() = default;
    ScopedBuf(const ScopedBuf&) = delete;
    ScopedBuf& operator=(const ScopedBuf&) = delete;
    ~ScopedBuf() { if (p) A::free(p); }
    int alloc(size_t count) {
        void* q = nullptr;
        if (A::alloc(&q, count * sizeof(T)) != 0) return LOB_ENOMEM;
        p = (T*)q;
        return LOB_OK;
    }
};

}  // namespace lob

#endif
