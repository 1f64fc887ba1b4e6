// Host-only RAII wrappers of device and pinned host allocations, shared by every host translation unit.
#pragma once
#include <vector>

#include "common.h"

namespace aur {

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    void ensure(size_t n) {
        if (n <= bytes) return;
        if (p) HIP_CHECK(hipFree(p));
        p = nullptr;
        bytes = 0;
        HIP_CHECK(hipMalloc(&p, n));
        bytes = n;
    }
    // ensure(n) and a blocking copy of n host bytes / of a host vector into the buffer
    void upload(const void* src, size_t n) {
        ensure(n);
        HIP_CHECK(hipMemcpy(p, src, n, hipMemcpyHostToDevice));
    }
    template <class T>
    void upload(const std::vector<T>& v) {
        upload(v.data(), v.size() * sizeof(T));
    }
    // ensure(n) and n zero bytes, in stream order
    void zeros(size_t n, hipStream_t st) {
        ensure(n);
        HIP_CHECK(hipMemsetAsync(p, 0, n, st));
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <class T>
    T* as() const {
        return reinterpret_cast<T*>(p);
    }
};

struct PinBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ~PinBuf() {
        if (p) (void)hipHostFree(p);
    }
    void ensure(size_t n) {
        if (n <= bytes) return;
        if (p) HIP_CHECK(hipHostFree(p));
        p = nullptr;
        HIP_CHECK(hipHostMalloc(&p, n, hipHostMallocDefault));
        bytes = n;
    }
    template <class T>
    T* as() const {
        return reinterpret_cast<T*>(p);
    }
};

}  // namespace aur
