// devbuf.hpp — an owned device array that knows its element count (the scene's buffers, the GPU builder's workspace).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace rtamd {

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
    size_t bytes() const { return n * sizeof(T); }
    // room for `want` elements: a buffer too small is freed and allocated anew (its contents are not kept)
    hipError_t reserve(size_t want) {
        if (n >= want) return hipSuccess;
        release();
        const hipError_t e = hipMalloc(&p, want * sizeof(T));
        if (e == hipSuccess) n = want;
        return e;
    }
    // a fresh array of exactly `count` elements; count == 0 still yields a pointer a kernel may be handed
    hipError_t alloc(size_t count) {
        release();
        const hipError_t e = hipMalloc(&p, (count ? count : 1) * sizeof(T));
        if (e == hipSuccess) n = count;
        return e;
    }
};

}  // namespace rtamd
