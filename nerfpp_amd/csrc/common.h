// common.h -- internal helpers of libnerfpp_hip (gfx950 only).
#pragma once

#include <atomic>
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "nerfpp_hip.h"
#include "nrf_math.h"
#include "owned.h"          // set_error, the NRF_* early-return macros, DevBuf / PinnedBuf / Scratch

namespace nrf {

// render.hip, for mesh.hip: sigma = raw[..., 3] of nrf_run_network(NRF_PREC_F32) at p explicit points [p, 3], bit for bit, on the exact-fp32 density kernels where the
// renderer has them (1 <= p <= 2^30)
size_t renderer_density_ws_bytes(const nrf_renderer *r, int64_t p);
int renderer_density(const nrf_renderer *r, const float *pts, int64_t p, float *sigma, void *ws, size_t ws_bytes, hipStream_t st);
struct PointSource;
// normals.hip: sigma and d sigma / d x of a hash grid + NeRFSmall (sigma == raw[..., 3] of NRF_PREC_F32 bit for bit); points whose wsel is 0 are skipped (nothing
// written).  NULL from density_grad_unsupported: the pair is in the built family, else the reason it is not
const char *density_grad_unsupported(const nrf_hash *h, const nrf_mlp *m);
int density_grad_launch(const nrf_hash *h, const nrf_mlp *m, const PointSource &ps, int64_t p, const float *wsel, float *sigma, float *grad, hipStream_t st);
//   out[ray] = sum_j w[ray][j] * sign * safe_normalize(v[row][v_col .. v_col + 2]), row = src ? src[ray * s + j] : ray * s + j, ascending j, w == 0 skipped
int normals_composite(int64_t n, int s, const float *v, int v_stride, int v_col, const int32_t *src, float sign, const float *weights, float *out, hipStream_t st);

// One-time kernel attribute setup (the dynamic-LDS window of a kernel) is per DEVICE, not per process: a process that drives several GPUs (the nrf_comm_* C ABI
// allows one communicator per device) must set it on each.  needed() is true until done() has been called for the calling thread's current device; the setup
// itself is idempotent, so two first callers racing on the same device both run it.
struct PerDeviceOnce {
    std::atomic<uint64_t> mask{0};
    static uint64_t bit() { int d = 0; (void)hipGetDevice(&d); return 1ull << (d & 63); }
    bool needed() const { return (mask.load(std::memory_order_acquire) & bit()) == 0; }
    void done() { mask.fetch_or(bit(), std::memory_order_release); }
};

static inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---- profiling (nrf_profile_*): HIP events on the caller's stream around the dominant kernels ----
struct ProfScope {
    int slot;
    hipStream_t stream;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool active;
    ProfScope(int slot, hipStream_t stream);
    ~ProfScope();
};

// ---- small device helpers ----

// Orders LDS traffic between the lanes of ONE wavefront (hardware executes a wave's DS ops in order; the fences
// stop the compiler from moving accesses across, the barrier pins the schedule).  No instruction is emitted beyond
// the waits the compiler derives.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// (the reductions over a wave and a block: reduce.h)
// inclusive prefix sum in lane order (lane = the caller's lane id)
__device__ __forceinline__ double wave_incl_scan(double v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double t = __shfl_up(v, off);
        if (lane >= off) v += t;
    }
    return v;
}

struct Bbox {
    float mn[3];
    float mx[3];
};

struct F3 {
    float x, y, z;
};

// A sample point is either read from an explicit [p,3] array or formed as o + d*z from a packed ray
// batch and a depth table (NeRFRenderer.h:419) -- the fused pipeline never materialises pts.
struct PointSource {
    const float *pts;     // explicit points, or nullptr
    const float *rays;    // [n, ray_stride] packed rays
    const float *z;       // [n, s]
    int ray_stride;
    int s;
};

__device__ __forceinline__ F3 load_point(const PointSource &ps, int64_t i)
{
    F3 r;
    if (ps.pts) {
        r.x = ps.pts[i * 3 + 0];
        r.y = ps.pts[i * 3 + 1];
        r.z = ps.pts[i * 3 + 2];
    } else {
        // 32-bit division when the index fits (always, for a chunk): the 64-bit one is a ~60-instruction sequence
        const int64_t ray = (i >> 31) == 0 ? (int64_t)((uint32_t)i / (uint32_t)ps.s) : i / ps.s;
        const float *rp = ps.rays + ray * ps.ray_stride;
        const float zz = ps.z[i];
        r.x = rp[0] + rp[3] * zz;
        r.y = rp[1] + rp[4] * zz;
        r.z = rp[2] + rp[5] * zz;
    }
    return r;
}

}  // namespace nrf
