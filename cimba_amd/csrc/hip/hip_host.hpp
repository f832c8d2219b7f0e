// Host-side HIP plumbing shared by every TU in this directory: the error
// macro, an owning device buffer, a scoped event timer and the integer
// environment knob.  Host only: no kernels, no model headers.  Everything
// that owns a device resource releases it in its destructor, so a HIP_TRY
// that returns from the middle of an entry point leaks nothing
// (scripts/hip_host_selfcheck.cpp drives the no-device error path).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdlib>
#include <optional>

// return a failed call's code (a hipError_t, or the int one of the helpers
// below made of it) as the entry point's int result
#define HIP_TRY(x)                        \
    do {                                  \
        const int err_ = (int)(x);        \
        if (err_ != 0) return err_;       \
    } while (0)
static_assert((int)hipSuccess == 0, "HIP_TRY tests against 0");

namespace cmb_hip {

// One hipMalloc of n elements of T.  Every member returns 0 or the
// hipError_t as int; a failed alloc leaves the buffer null.
template <class T>
class DevBuf {
    T* p_ = nullptr;
    size_t n_ = 0;

public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : n_(o.n_) { p_ = o.release(); }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            n_ = o.n_;
            p_ = o.release();
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    int alloc(size_t n) {
        reset();
        HIP_TRY(hipMalloc(&p_, sizeof(T) * n));
        n_ = n;
        return 0;
    }
    int zero() { return (int)hipMemset(p_, 0, sizeof(T) * n_); }
    int upload(const T* src, size_t n = 1) {
        return (int)hipMemcpy(p_, src, sizeof(T) * n, hipMemcpyHostToDevice);
    }
    int download(T* dst, size_t n = 1) const {
        return (int)hipMemcpy(dst, p_, sizeof(T) * n, hipMemcpyDeviceToHost);
    }
    T* get() const { return p_; }
    // hand the allocation to the caller (a handle that outlives the call)
    T* release() {
        T* p = p_;
        p_ = nullptr;
        n_ = 0;
        return p;
    }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        n_ = 0;
    }
};

// Event pair around a launch on the null stream: start() creates and
// records, stop() records, synchronises and reads the elapsed time.
class EventTimer {
    hipEvent_t t0_ = nullptr, t1_ = nullptr;

public:
    EventTimer() = default;
    EventTimer(const EventTimer&) = delete;
    EventTimer& operator=(const EventTimer&) = delete;
    ~EventTimer() {
        if (t0_) (void)hipEventDestroy(t0_);
        if (t1_) (void)hipEventDestroy(t1_);
    }
    int start() {
        if (!t0_) HIP_TRY(hipEventCreate(&t0_));
        if (!t1_) HIP_TRY(hipEventCreate(&t1_));
        return (int)hipEventRecord(t0_);
    }
    int stop(double* ms) {
        HIP_TRY(hipEventRecord(t1_));
        HIP_TRY(hipEventSynchronize(t1_));
        float f = 0.f;
        HIP_TRY(hipEventElapsedTime(&f, t0_, t1_));
        *ms = (double)f;
        return 0;
    }
};

// integer environment knob, parsed with atoi; nullopt = unset (several
// policies tell "unset" from "0")
inline std::optional<int> env_int(const char* name) {
    const char* e = getenv(name);
    if (!e) return std::nullopt;
    return atoi(e);
}

}  // namespace cmb_hip
