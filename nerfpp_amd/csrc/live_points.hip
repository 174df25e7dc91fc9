// live_points.hip -- deterministic stream compaction of the points whose density contributes to a render.
//
// k_raw2outputs (composite.hip) takes relu(sigma) as `sg > 0.0f ? sg : 0.0f`: for every other sigma (negative, +-0, NaN) alpha is exactly 0, the weight is exactly 0
// and w * rgb is +0 for every finite rgb, so the colour of such a point cannot change a bit of RGB, depth, disparity, acc or the weights.  At the coarse depths of a
// hierarchical render sigma is known before the colour net runs (the exact coarse kernel wrote it), so the fine pass's colour-only launch runs over the list made here.
//
//   list[0 .. count)  the point indices with sigma > 0.0f, ascending (part of the contract: the colour kernel's operand gathers stay nearly sequential and the layout
//                     does not depend on scheduling)
//   count             one int32 on the device; nothing is read back
//   rows[p]           (optional) for every DEAD point its raw row (0, 0, 0, sigma), the sigma word copied as it is (a NaN stays a NaN for the non-finite test of
//                     the compositing kernel); rows of live points are left to the colour kernel
//
// Three launches, no atomics: per-block counts, one block scans them, every block scatters its points behind its own offset.  A wave takes LIVE_STEPS x 64
// consecutive points (all loads issued before the first is used); a lane's position in the list is the popcount of the live lanes below it.
#include "live_points.h"
#include "scan.h"

namespace nrf {

constexpr int LIVE_WAVES = 4, LIVE_STEPS = 8;
constexpr int LIVE_BLOCK_PTS = 64 * LIVE_STEPS * LIVE_WAVES;          // 2 048 points per workgroup
constexpr int LIVE_SCAN_B = 1024;

static inline int64_t live_blocks(int64_t p) { return ceil_div(p, LIVE_BLOCK_PTS); }

// the wave's LIVE_STEPS x 64 values from point p0 on; points at or beyond p read as dead (0)
__device__ __forceinline__ void live_load(const float *__restrict__ sigma, uint32_t p0, uint32_t p, int lane, float (&sg)[LIVE_STEPS])
{
#pragma unroll
    for (int k = 0; k < LIVE_STEPS; k++) {
        const uint32_t i = p0 + (uint32_t)(k * 64 + lane);
        sg[k] = i < p ? sigma[i] : 0.0f;
    }
}

__global__ void __launch_bounds__(64 * LIVE_WAVES)
k_live_count(uint32_t p, const float *__restrict__ sigma, int32_t *__restrict__ sums)
{
    __shared__ int32_t wsum[LIVE_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float sg[LIVE_STEPS];
    live_load(sigma, blockIdx.x * (uint32_t)LIVE_BLOCK_PTS + (uint32_t)(wave * 64 * LIVE_STEPS), p, lane, sg);
    int32_t c = 0;
#pragma unroll
    for (int k = 0; k < LIVE_STEPS; k++) c += __popcll(__ballot(sg[k] > 0.0f));
    if (lane == 0) wsum[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t t = 0;
#pragma unroll
        for (int w = 0; w < LIVE_WAVES; w++) t += wsum[w];
        sums[blockIdx.x] = t;
    }
}

// sums[b] <- sum of sums[0 .. b), count <- the total; one workgroup walks the array in LIVE_SCAN_B-wide pieces
__global__ void __launch_bounds__(LIVE_SCAN_B)
k_live_scan(int32_t nb, int32_t *__restrict__ sums, int32_t *__restrict__ count)
{
    __shared__ int32_t sh[LIVE_SCAN_B];
    int32_t carry = 0;
    for (int32_t base = 0; base < nb; base += LIVE_SCAN_B) {
        const int32_t i = base + (int32_t)threadIdx.x;
        const int32_t v = i < nb ? sums[i] : 0;
        int32_t total;
        const int32_t ex = block_exclusive_scan<int32_t, LIVE_SCAN_B>(v, sh, total);
        if (i < nb) sums[i] = carry + ex;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = carry;
}

__global__ void __launch_bounds__(64 * LIVE_WAVES)
k_live_scatter(uint32_t p, const float *__restrict__ sigma, const int32_t *__restrict__ sums, int32_t *__restrict__ list, float4 *__restrict__ rows)
{
    __shared__ int32_t wsum[LIVE_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t p0 = blockIdx.x * (uint32_t)LIVE_BLOCK_PTS + (uint32_t)(wave * 64 * LIVE_STEPS);
    float sg[LIVE_STEPS];
    live_load(sigma, p0, p, lane, sg);
    uint64_t mask[LIVE_STEPS];
    int32_t c = 0;
#pragma unroll
    for (int k = 0; k < LIVE_STEPS; k++) { mask[k] = __ballot(sg[k] > 0.0f); c += __popcll(mask[k]); }
    if (lane == 0) wsum[wave] = c;
    __syncthreads();
    int32_t at = sums[blockIdx.x];
    for (int w = 0; w < wave; w++) at += wsum[w];
    const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
    for (int k = 0; k < LIVE_STEPS; k++) {
        const uint32_t i = p0 + (uint32_t)(k * 64 + lane);
        if ((mask[k] >> lane) & 1ull) list[at + __popcll(mask[k] & below)] = (int32_t)i;          // (a live lane has i < p: points beyond p were read as dead)
        else if (rows && i < p) rows[i] = float4{0.0f, 0.0f, 0.0f, sg[k]};
        at += __popcll(mask[k]);
    }
}

LiveWs live_points_layout(Bump &b, int64_t p)
{
    LiveWs w{};
    w.sums = b.take<int32_t>((size_t)live_blocks(p));
    return w;
}

int live_points_launch(const float *sigma, int64_t p, int32_t *list, int32_t *count, float *rows, const LiveWs &w, hipStream_t st)
{
    if (p <= 0 || p >= ((int64_t)1 << 31)) { set_error("internal: live-point compaction of %lld points (1 .. 2^31 - 1)", (long long)p); return NRF_ERR_INVALID_ARG; }
    const unsigned nb = (unsigned)live_blocks(p);
    hipLaunchKernelGGL(k_live_count, dim3(nb), dim3(64 * LIVE_WAVES), 0, st, (uint32_t)p, sigma, w.sums);
    hipLaunchKernelGGL(k_live_scan, dim3(1), dim3(LIVE_SCAN_B), 0, st, (int32_t)nb, w.sums, count);
    hipLaunchKernelGGL(k_live_scatter, dim3(nb), dim3(64 * LIVE_WAVES), 0, st, (uint32_t)p, sigma, w.sums, list, reinterpret_cast<float4 *>(rows));
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

// ---- the switch: NRF_LIVE_COLOUR=0 / nrf_set_live_colour(0) keeps the colour launch over every coarse depth ----
static std::atomic<int> g_live_colour{-1};          // -1: not decided yet (environment, default on)
int live_colour_on()
{
    int v = g_live_colour.load(std::memory_order_relaxed);
    if (v < 0) {
        const char *e = getenv("NRF_LIVE_COLOUR");
        v = (e && strcmp(e, "0") == 0) ? 0 : 1;
        g_live_colour.store(v, std::memory_order_relaxed);
    }
    return v;
}

}  // namespace nrf

extern "C" {

int nrf_set_live_colour(int on)
{
    NRF_CHECK_ARG(on == 0 || on == 1, "nrf_set_live_colour: 0 (colour at every coarse depth) or 1 (only where sigma > 0)");
    nrf::g_live_colour.store(on, std::memory_order_relaxed);
    return NRF_OK;
}

int nrf_get_live_colour(void) { return nrf::live_colour_on(); }

size_t nrf_live_points_workspace_bytes(int64_t p)
{
    if (p <= 0) return 0;
    return nrf::measure([&](nrf::Bump &b) { nrf::live_points_layout(b, p); });
}

int nrf_live_points(const float *d_sigma, int64_t p, int32_t *d_list, int32_t *d_count, float *d_raw_rows, void *d_workspace, size_t workspace_bytes, void *stream)
{
    NRF_CHECK_ARG(d_sigma && d_list && d_count, "nrf_live_points: null pointer");
    NRF_CHECK_ARG(p >= 1 && p < ((int64_t)1 << 31), "nrf_live_points: 1 <= p < 2^31 points");
    NRF_CHECK_ARG(!d_raw_rows || (reinterpret_cast<uintptr_t>(d_raw_rows) & 15) == 0, "nrf_live_points: d_raw_rows must be 16-byte aligned");
    NRF_CHECK_ARG(d_workspace, "nrf_live_points: null workspace");
    nrf::Bump bump(d_workspace, workspace_bytes);
    const nrf::LiveWs w = nrf::live_points_layout(bump, p);
    NRF_TRY(nrf::ws_check(bump, nrf_live_points_workspace_bytes(p), "nrf_live_points"));
    return nrf::live_points_launch(d_sigma, p, d_list, d_count, d_raw_rows, w, nrf::as_stream(stream));
}

}  // extern "C"
