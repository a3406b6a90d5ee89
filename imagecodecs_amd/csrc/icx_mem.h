// icx_mem.h -- who owns device and pinned host memory on the host side of libicx.so. Every
// hipFree / hipHostFree of a workspace is here. A failed allocation leaves HIP's error for the
// caller to report (hipGetLastError).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace icx {

// A grow-only block of device memory (pinned host memory with Buf<T> b{true}). reserve() keeps a
// block that is large enough; otherwise it frees it and allocates anew (contents are not kept).
template <class T>
struct Buf {
    T* p = nullptr;
    size_t cap = 0;  // bytes allocated
    bool pinned = false;
    explicit Buf(bool pinned_host = false) : pinned(pinned_host) {}
    Buf(Buf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)), pinned(o.pinned) {}
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            cap = std::exchange(o.cap, 0);
            pinned = o.pinned;
        }
        return *this;
    }
    ~Buf() { release(); }
    // false (and empty) when the allocation fails
    bool reserve(size_t bytes) {
        if (p && bytes <= cap) return true;
        release();
        bytes = std::max<size_t>(bytes, 64);
        void* q = nullptr;
        if ((pinned ? hipHostMalloc(&q, bytes, hipHostMallocDefault) : hipMalloc(&q, bytes)) != hipSuccess) return false;
        p = static_cast<T*>(q);
        cap = bytes;
        return true;
    }
    void release() {
        if (p) (void)(pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }
};

// The blocks of a workspace allocated once (GroupWs, HdrWs): the struct keeps plain pointers for
// the launch code, this frees them -- also after a failure part-way through the allocations.
struct Blocks {
    std::vector<Buf<void>> all;
    template <class T>
    bool alloc(T*& p, size_t bytes, bool pinned_host = false) {
        Buf<void> b(pinned_host);
        if (!b.reserve(bytes)) return false;
        p = static_cast<T*>(b.p);
        all.push_back(std::move(b));
        return true;
    }
    void release() { all.clear(); }
};

}  // namespace icx
