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
#include "stoch.h"

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

// ---- the same list from per-ray masks ----
// k_resample (composite.hip) had every coarse sigma of a ray in one wave's lanes: it leaves counts[ray] = #{sigma > 0} and the ray's ceil(s / 64) ballot masks in the
// first bytes of the ray's own rows [ray * s .. ray * s + s).  One workgroup turns the n counts into the offsets of the groups of 64 rays (no second pass over sigma, no
// atomics, no read-back; behind the counts, see ray_counts_len); then a wave per ray adds the counts of the rays before it in its group, expands the masks into the
// ascending columns ray * s + i and writes the rows of the ray's dead columns -- after it has read the masks out of them.
constexpr int RAY_SCAN_B = 1024;
constexpr int RAY_GROUP = 64;                                                   // rays per scanned group: one coalesced load and one wave sum
static inline int64_t ray_groups_at(int64_t n) { return (n + 3) / 4 * 4; }     // the group offsets' place in the counts array (16-byte aligned like the counts)

// goffs[g] <- sum of counts[0 .. 64 g).  A thread loads four consecutive counts (a wave 1 KB in a row), sixteen lanes sum a group, and the block scans RAY_SCAN_B group
// sums at a time (scan.h).  The counts array is a multiple of four words long (ray_groups_at): the last load stays inside it, and what lies past n is not added.
__global__ void __launch_bounds__(RAY_SCAN_B)
k_ray_scan(int32_t n, const int32_t *__restrict__ counts, int32_t *__restrict__ goffs)
{
    constexpr int STEPS = RAY_GROUP / 4;          // loads per thread and piece: RAY_SCAN_B groups x 64 rays / (RAY_SCAN_B threads x 4 rays)
    __shared__ int32_t sh[RAY_SCAN_B], gsum[RAY_SCAN_B];
    const int32_t ng = (n + RAY_GROUP - 1) / RAY_GROUP;
    int32_t carry = 0;
    for (int32_t g0 = 0; g0 < ng; g0 += RAY_SCAN_B) {
        int4 v[STEPS];
#pragma unroll
        for (int k = 0; k < STEPS; k++) {          // every load is issued before the first sum
            const int64_t i = ((int64_t)g0 * RAY_GROUP / 4 + k * RAY_SCAN_B + threadIdx.x) * 4;
            v[k] = i < n ? *reinterpret_cast<const int4 *>(counts + i) : int4{0, 0, 0, 0};
        }
#pragma unroll
        for (int k = 0; k < STEPS; k++) {
            const int64_t i = ((int64_t)g0 * RAY_GROUP / 4 + k * RAY_SCAN_B + threadIdx.x) * 4;
            int32_t t = v[k].x + (i + 1 < n ? v[k].y : 0) + (i + 2 < n ? v[k].z : 0) + (i + 3 < n ? v[k].w : 0);
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) t += __shfl_xor(t, off);
            if ((threadIdx.x & 15) == 0) gsum[k * (RAY_SCAN_B / 16) + (threadIdx.x >> 4)] = t;
        }
        __syncthreads();
        int32_t total;
        const int32_t ex = block_exclusive_scan<int32_t, RAY_SCAN_B>(gsum[threadIdx.x], sh, total);
        if (g0 + (int32_t)threadIdx.x < ng) goffs[g0 + threadIdx.x] = carry + ex;
        carry += total;
        __syncthreads();
    }
}

constexpr int MASK_WAVES = 4;         // waves per workgroup
constexpr int MASK_RPW = 4;           // consecutive rays per wave: their masks and counts are requested before the first row is written
constexpr int MASK_WORDS = 4;         // s <= 256

__global__ void __launch_bounds__(64 * MASK_WAVES)
k_mask_scatter(int32_t n, int s, const float *__restrict__ sigma, const int32_t *__restrict__ counts, const int32_t *__restrict__ goffs, int32_t *__restrict__ list,
               int32_t *__restrict__ count, float4 *rows)
{
    const int lane = threadIdx.x & 63;
    const int32_t r0 = ((int32_t)blockIdx.x * MASK_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))) * MASK_RPW;          // (a multiple of 4: one group)
    if (r0 >= n) return;
    const int32_t g = r0 / RAY_GROUP, gr = g * RAY_GROUP;
    // this lane's ray of the group, counted only where it precedes r0; the wave's rays follow from their own counts
    int32_t before = (gr + lane < r0) ? counts[gr + lane] : 0;
    float4 q0[MASK_RPW], q1[MASK_RPW];
    float sgv[MASK_RPW][MASK_WORDS];
    // the masks, read as the rows they lie in (the type the stores below have: none of them can move above these loads), and with them the rays' sigma: one round of
    // loads, then one of stores
#pragma unroll
    for (int q = 0; q < MASK_RPW; q++) {
        const int32_t ray = r0 + q < n ? r0 + q : n - 1;
        q0[q] = rows[(int64_t)ray * s];
        q1[q] = s > 128 ? rows[(int64_t)ray * s + 1] : float4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int b = 0; b < MASK_WORDS; b++) sgv[q][b] = b * 64 + lane < s ? sigma[(int64_t)ray * s + b * 64 + lane] : 0.0f;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off);
    int32_t at = goffs[g] + before;
    const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
    for (int q = 0; q < MASK_RPW; q++) {
        const int32_t ray = r0 + q;
        if (ray >= n) break;
        uint64_t mask[MASK_WORDS];
        mask[0] = (uint64_t)__float_as_uint(q0[q].x) | ((uint64_t)__float_as_uint(q0[q].y) << 32);
        mask[1] = s > 64 ? (uint64_t)__float_as_uint(q0[q].z) | ((uint64_t)__float_as_uint(q0[q].w) << 32) : 0ull;
        mask[2] = (uint64_t)__float_as_uint(q1[q].x) | ((uint64_t)__float_as_uint(q1[q].y) << 32);
        mask[3] = s > 192 ? (uint64_t)__float_as_uint(q1[q].z) | ((uint64_t)__float_as_uint(q1[q].w) << 32) : 0ull;
        float4 *rr = rows + (int64_t)ray * s;
        const int32_t col0 = ray * s;
#pragma unroll
        for (int b = 0; b < MASK_WORDS; b++) {
            if (b * 64 >= s) break;
            const int j = b * 64 + lane;
            if ((mask[b] >> lane) & 1ull) list[at + __popcll(mask[b] & below)] = col0 + j;          // (a live lane has j < s: the ballot was taken over the ray's samples only)
            else if (j < s) rr[j] = float4{0.0f, 0.0f, 0.0f, sgv[q][b]};
            at += __popcll(mask[b]);
        }
        if (ray == n - 1 && lane == 0) *count = at;
    }
}

// the counts array of launch_resample / live_from_masks_launch: n per-ray counts, then (16-byte aligned) the offsets of the groups of 64 rays
int64_t ray_counts_len(int64_t n) { return ray_groups_at(n) + ceil_div(n, RAY_GROUP); }

int live_from_masks_launch(const float *sigma, int64_t n, int s, int32_t *counts, int32_t *list, int32_t *count, float *rows, hipStream_t st)
{
    if (n <= 0 || s < 1 || s > 64 * MASK_WORDS || n * (int64_t)s >= ((int64_t)1 << 31) || !rows || (reinterpret_cast<uintptr_t>(counts) & 15)) {
        set_error("internal: live list from masks of %lld rays x %d samples", (long long)n, s);
        return NRF_ERR_INVALID_ARG;
    }
    int32_t *goffs = counts + ray_groups_at(n);
    hipLaunchKernelGGL(k_ray_scan, dim3(1), dim3(RAY_SCAN_B), 0, st, (int32_t)n, counts, goffs);
    hipLaunchKernelGGL(k_mask_scatter, dim3((unsigned)ceil_div(n, MASK_WAVES * MASK_RPW)), dim3(64 * MASK_WAVES), 0, st, (int32_t)n, s, sigma, counts, goffs, list, count,
                       reinterpret_cast<float4 *>(rows));
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

// ---- the switch: NRF_FUSED_RESAMPLE=0 / nrf_set_fused_resample(0) keeps the stage-wise chain (exact weights, fine depths, count / scan / scatter) ----
static std::atomic<int> g_fused_resample{-1};          // -1: not decided yet (environment, default on)
int fused_resample_on()
{
    int v = g_fused_resample.load(std::memory_order_relaxed);
    if (v < 0) {
        const char *e = getenv("NRF_FUSED_RESAMPLE");
        v = (e && strcmp(e, "0") == 0) ? 0 : 1;
        g_fused_resample.store(v, std::memory_order_relaxed);
    }
    return v;
}

}  // namespace nrf

extern "C" {

int nrf_set_fused_resample(int on)
{
    NRF_CHECK_ARG(on == 0 || on == 1, "nrf_set_fused_resample: 0 (one launch per stage) or 1 (one resampling kernel per chunk)");
    nrf::g_fused_resample.store(on, std::memory_order_relaxed);
    return NRF_OK;
}

int nrf_get_fused_resample(void) { return nrf::fused_resample_on(); }

int nrf_dbg_resample(const float *d_sigma, const float *d_z, const float *d_dirs, int d_stride, int64_t n, int s, const float *d_u, int64_t u_stride, uint64_t seed,
                     int64_t ray_base, int ns, int sum_vec, float *d_z_fine, int32_t *d_src, float *d_z_new, float *d_weights, int32_t *d_counts, int32_t *d_list,
                     int32_t *d_count, float *d_raw_rows, void *stream)
{
    NRF_CHECK_ARG(d_sigma && d_z && d_dirs && d_z_fine && d_src && d_z_new && n >= 0 && d_stride >= 3, "nrf_dbg_resample: bad argument");
    NRF_CHECK_ARG(!d_counts || (d_list && d_count && d_raw_rows && (reinterpret_cast<uintptr_t>(d_counts) & 15) == 0), "nrf_dbg_resample: the live part needs list, count, rows and 16-byte aligned counts");
    NRF_TRY(nrf::launch_resample(d_z, d_sigma, d_dirs, d_stride, n, s, d_u, u_stride, nrf::RngRef{seed, ray_base}, ns, sum_vec, d_z_fine, d_src, d_z_new, d_weights, d_counts,
                                 d_raw_rows, nrf::as_stream(stream)));
    if (!d_counts || n == 0) return NRF_OK;
    return nrf::live_from_masks_launch(d_sigma, n, s, d_counts, d_list, d_count, d_raw_rows, nrf::as_stream(stream));
}

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
