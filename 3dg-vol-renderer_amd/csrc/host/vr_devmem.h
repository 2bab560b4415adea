// Owners of the HIP objects the host code holds: device allocations (DevBuf), pinned host memory
// (PinnedBuf), events and streams. Each frees its object in its destructor, so a context or a local that
// goes away (an early HIP_TRY return included) leaks nothing. This is the only host file that calls
// hipMalloc / hipFree / hipHostFree / hipEventDestroy / hipStreamDestroy.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <utility>

#include "vr_common.h"

#pragma GCC visibility push(hidden)  // internal to libvr_hip.so: nothing here is an exported symbol
namespace vr {

inline vr_status hip_fail(hipError_t e, const char* what) {
    return fail(VR_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
inline vr_status hip_status(hipError_t e, const char* what) { return e == hipSuccess ? VR_OK : hip_fail(e, what); }
// Return from the calling function with the failure of a vr_status / hipError_t expression.
#define VR_TRY(expr)                \
    do {                            \
        vr_status s_ = (expr);      \
        if (s_ != VR_OK) return s_; \
    } while (0)
#define HIP_TRY(expr, what) VR_TRY(::vr::hip_status(expr, what))

// A hipMalloc allocation of T (move-only). The device that is current when it is allocated must be
// current when it is freed. Carved workspaces are DevBuf<std::byte>: their n counts bytes.
template <class T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {  // (what this held goes with o)
        std::swap(p_, o.p_);
        std::swap(bytes_, o.bytes_);
        return *this;
    }
    ~DevBuf() { reset(); }

    T* get() const { return p_; }
    size_t bytes() const { return bytes_; }
    size_t count() const { return bytes_ / sizeof(T); }
    explicit operator bool() const { return p_ != nullptr; }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        bytes_ = 0;
    }
    // Takes over an allocation of n elements made elsewhere (the device BVH builder's results).
    void adopt(T* p, size_t n) {
        reset();
        p_ = p;
        bytes_ = p ? n * sizeof(T) : 0;
    }
    // Exactly n elements; what it held is freed first. Empty on failure.
    hipError_t try_alloc(size_t n) { return alloc_bytes(n * sizeof(T)); }
    vr_status alloc(size_t n, const char* what) { return hip_status(try_alloc(n), what); }
    // Room for n elements: left alone if it is large enough, else freed and allocated a quarter larger
    // (256 bytes at least). Never shrinks, keeps no contents. Empty on failure.
    vr_status grow(size_t n, const char* what) { return grow_bytes(n * sizeof(T), what); }
    template <class P>
    vr_status grow(size_t n, const char* what, P& out) {  // ... and out = get()
        vr_status st = grow(n, what);
        out = p_;
        return st;
    }
    vr_status grow_bytes(size_t bytes, const char* what) {
        if (bytes <= bytes_ && p_) return VR_OK;
        return hip_status(alloc_bytes(std::max<size_t>(bytes + bytes / 4, 256)), what);
    }

private:
    hipError_t alloc_bytes(size_t bytes) {
        reset();
        hipError_t e = hipMalloc(&p_, bytes);
        if (e != hipSuccess) p_ = nullptr;
        else bytes_ = bytes;
        return e;
    }
    T* p_ = nullptr;
    size_t bytes_ = 0;
};

// n elements of pinned host memory.
template <class T>
class PinnedBuf {
public:
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&&) = delete;
    ~PinnedBuf() { if (p_) (void)hipHostFree(p_); }
    hipError_t alloc(size_t n) { return hipHostMalloc(&p_, n * sizeof(T), hipHostMallocDefault); }
    T* get() const { return p_; }
    T& operator[](size_t i) const { return p_[i]; }

private:
    T* p_ = nullptr;
};

// A HIP event or stream (move-only): created into put(), destroyed with the owner.
template <class H, hipError_t (*Destroy)(H)>
class Handle {
public:
    Handle() = default;
    Handle(Handle&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    ~Handle() { reset(); }
    H* put() { return &h_; }
    operator H() const { return h_; }
    void reset() {
        if (h_) (void)Destroy(h_);
        h_ = nullptr;
    }

private:
    H h_ = nullptr;
};
using Event = Handle<hipEvent_t, hipEventDestroy>;
using Stream = Handle<hipStream_t, hipStreamDestroy>;

}  // namespace vr
#pragma GCC visibility pop
