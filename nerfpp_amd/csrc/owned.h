// owned.h -- who frees what: every device / pinned allocation and every scratch block of the library has exactly one owner, and the early-return macros every
// entry point leaves through.  Host code only (no kernels, no HIP library needed to parse it): tests/helpers/owned_check.cpp instantiates it with counting fakes.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <memory>          // handles are built in a std::unique_ptr and released into *out on success

#include "nerfpp_hip.h"

namespace nrf {

void set_error(const char *fmt, ...);
// the library's own stream-ordered scratch (scratch.hip): a buffer for work enqueued on `st`; given back, it serves the next taker ON THAT STREAM.  Drop-in replacements of
// hipMallocAsync / hipFreeAsync (same return type), which proved unsafe inside the LibTorch host.  Taken and given back through Scratch (below) only
hipError_t scratch_take(void **out, size_t bytes, hipStream_t st);
hipError_t scratch_give(void *p, hipStream_t st);
// the ONE count of device bytes the library holds (scratch.hip; nrf_device_bytes_in_use): DeviceMem and the scratch blocks add to it, nothing else allocates
void device_bytes_add(int64_t delta);

#define NRF_CHECK_ARG(cond, ...)                                   \
    do {                                                           \
        if (!(cond)) {                                             \
            ::nrf::set_error(__VA_ARGS__);                         \
            return NRF_ERR_INVALID_ARG;                            \
        }                                                          \
    } while (0)

#define NRF_HIP(call)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            ::nrf::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return NRF_ERR_HIP;                                                                   \
        }                                                                                         \
    } while (0)

#define NRF_LAUNCH_CHECK()                                                                        \
    do {                                                                                          \
        hipError_t e_ = hipGetLastError();                                                        \
        if (e_ != hipSuccess) {                                                                   \
            ::nrf::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), __FILE__, __LINE__); \
            return NRF_ERR_HIP;                                                                   \
        }                                                                                         \
    } while (0)

#define NRF_TRY(expr)                  \
    do {                               \
        int s_ = (expr);               \
        if (s_ != NRF_OK) return s_;   \
    } while (0)

// Mem: where a Buf's bytes come from -- alloc, release, and the name of the call for the error text
struct DeviceMem {
    static constexpr const char *call = "hipMalloc";
    static hipError_t alloc(void **p, size_t bytes) { const hipError_t e = hipMalloc(p, bytes); if (e == hipSuccess) device_bytes_add((int64_t)bytes); return e; }
    static void release(void *p, size_t bytes) { (void)hipFree(p); device_bytes_add(-(int64_t)bytes); }
};
struct PinnedMem {
    static constexpr const char *call = "hipHostMalloc";
    static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void release(void *p, size_t) { (void)hipHostFree(p); }
};

// Move-only owner of one allocation of Mem.  Moving keeps the address (a std::vector of owners may grow under pointers borrowed from them).
template <class Mem> class Buf {
    void *p_ = nullptr;
    size_t n_ = 0;
public:
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    Buf(Buf &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    Buf &operator=(Buf &&o) noexcept { if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; } return *this; }
    ~Buf() { reset(); }
    void reset() { if (p_) Mem::release(p_, n_); p_ = nullptr; n_ = 0; }
    // the same size: the allocation stays (a re-pack of the same shape writes in place); another: freed, then allocated anew; 0 bytes or a failure: left empty
    int resize(size_t bytes)
    {
        if (p_ && n_ == bytes) return NRF_OK;
        reset();
        if (bytes == 0) return NRF_OK;
        const hipError_t e = Mem::alloc(&p_, bytes);
        if (e != hipSuccess) { p_ = nullptr; set_error("%s(%zu) failed: %s", Mem::call, bytes, hipGetErrorString(e)); return NRF_ERR_HIP; }
        n_ = bytes;
        return NRF_OK;
    }
    int upload(const void *host, size_t bytes) { NRF_TRY(resize(bytes)); NRF_HIP(hipMemcpy(p_, host, bytes, hipMemcpyHostToDevice)); return NRF_OK; }          // synchronous
    size_t bytes() const { return n_; }
    explicit operator bool() const { return p_ != nullptr; }
    template <class T> T *as() const { return static_cast<T *>(p_); }
};
using DevBuf = Buf<DeviceMem>;
using PinnedBuf = Buf<PinnedMem>;

// One scratch block for the work a function enqueues on `st`; every return path gives it back on that stream.
class Scratch {
    void *p_ = nullptr;
    hipStream_t st_ = nullptr;
public:
    Scratch() = default;
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    ~Scratch() { if (p_) (void)scratch_give(p_, st_); }
    int take(size_t bytes, hipStream_t st) { if (p_) (void)scratch_give(p_, st_); p_ = nullptr; st_ = st; NRF_HIP(scratch_take(&p_, bytes, st)); return NRF_OK; }
    explicit operator bool() const { return p_ != nullptr; }
    template <class T> T *as() const { return static_cast<T *>(p_); }
};

}  // namespace nrf
