// Host-only RAII wrappers of device and pinned host allocations, the table of loaded weights and the profilers' event pool, shared by every host translation unit.
#pragma once
#include <memory>
#include <string>
#include <unordered_map>
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

// The loaded checkpoint: tensor name -> fp32 device buffer.  The engine fills it (aur_load_weights); the networks look their weights up
// in it when they bind.
struct Tensor {
    std::unique_ptr<DevBuf> buf;
    int64_t numel = 0;
    bool f16_eff = false;   // aur_config.gpt_fp16: the buffer holds the effective weights W'' (a per-layer matrix), or the LayerNorm
                            // gain they were derived with, since the last load of this tensor
    float* d() const { return buf->as<float>(); }
};
struct WeightTable {
    std::unordered_map<std::string, Tensor> map;
    bool has(const std::string& name) const { return map.find(name) != map.end(); }
    Tensor& at(const std::string& name) {
        auto it = map.find(name);
        if (it == map.end()) throw StateError("weight not loaded: " + name);
        return it->second;
    }
    const float* W(const std::string& name, int64_t numel = -1) {
        const Tensor& t = at(name);
        if (numel >= 0 && t.numel != numel)
            throw InvalidArgument("weight " + name + " has " + std::to_string(t.numel) + " elements, expected " + std::to_string(numel));
        return t.d();
    }
};

// A pair of timing events and what the launches between them are booked as: the profiled batches of the decode chain and the
// vocoder's launches.
struct ProfEvent {
    hipEvent_t a, b;
    double flops, bytes;   // of ALL the launches between the two events
    int kind;    // decode profile: 0..4 = GEMM kind (aur_stats.gemm_kind_*), 5 = paged attention; vocoder: aur_stats.conv_class_*, -1 = a whole forward
    int count;   // launches between the two events (decode profile batches)
};
// the next event pair of a pool that grows on demand and is reused from the start once its events have been collected
inline ProfEvent& next_event(std::vector<ProfEvent>& pool, size_t& n_used) {
    if (n_used == pool.size()) {
        ProfEvent e{};
        HIP_CHECK(hipEventCreate(&e.a));
        HIP_CHECK(hipEventCreate(&e.b));
        pool.push_back(e);
    }
    return pool[n_used++];
}

}  // namespace aur
