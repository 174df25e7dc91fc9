// reduce.h -- the ordered fp64 sum behind every loss and metric (partials -> totals), in one place.  No atomics anywhere in it: two runs give the same bits.  The order,
// as include/nerfpp_hip.h states it (nrf_mesh_sample_count, step 4) and tests/ordered_sum_ref.py restates it:
//   1. per wave the butterfly v += v[lane ^ o], o = 32 .. 1                                       wave_sum (wave_max: the same tree with fmax)
//   2. per block ((w0 + w1) + w2) + ... over the B / 64 wave sums                                  ordered_block_sum<B, NV> (ordered_block_max<B>)
//   3. over the block partials: thread t of B adds k = t, t + B, ... in ascending order from 0.0  ordered_finish<B, NV, MAX>
//   4. then s[t] += s[t + o] for t < o, o = B / 2 .. 1                                             the same
//   k_finish_loss_pair<B>      kernel: the two fp32 training losses of a [blocks][2] partial array, each divided by its own count
//   block_key_min<B>           the block-wide minimum of a packed 64-bit key (order-free; here because it is the same wave tree + one LDS word per wave)
//   key_pack / key_value / key_index / key_lower, NN_NONE, NO_KEY   that key itself: (float_bits(value) << 32) | index, and its lowering in memory
// A kernel keeps its accumulation into one double per lane and what it does with the total; it writes none of the steps above itself.
#pragma once

#include "common.h"

namespace nrf {

// ---- reductions over the 64 lanes of a wave (every lane gets the result) ----
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}

template <bool MAX> __device__ __forceinline__ double ordered_op(double a, double b) { return MAX ? fmax(a, b) : a + b; }

// ---- steps 1 and 2: v[c] = the block's ordered sum of column c, in every thread.  sh: NV * (B / 64) doubles.  ONE barrier for all NV columns; sh is still being read
// when a thread returns, so a second use of the same words needs a __syncthreads() first ----
template <int B, int NV, bool MAX = false>
__device__ __forceinline__ void ordered_block_sum(double (&v)[NV], double *sh)
{
    constexpr int W = B / 64;
#pragma unroll
    for (int c = 0; c < NV; c++) v[c] = MAX ? wave_max(v[c]) : wave_sum(v[c]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < NV; c++) sh[c * W + (threadIdx.x >> 6)] = v[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NV; c++) {
        double a = sh[c * W];
#pragma unroll
        for (int k = 1; k < W; k++) a = ordered_op<MAX>(a, sh[c * W + k]);
        v[c] = a;
    }
}

// one column (sh: B / 64 doubles), and the block-wide fmax: it does not depend on the order and goes through the same words and barrier
template <int B> __device__ __forceinline__ double ordered_block_sum(double v, double *sh)
{
    double a[1] = {v};
    ordered_block_sum<B, 1>(a, sh);
    return a[0];
}
template <int B> __device__ __forceinline__ double ordered_block_max(double v, double *sh)
{
    double a[1] = {v};
    ordered_block_sum<B, 1, true>(a, sh);
    return a[0];
}

// ---- steps 3 and 4, one workgroup of B threads: out[c] = the sum (MAX: the maximum) over k < count of partials[k * stride + column + c], in every thread.
// sh: NV * B doubles, free again on return ----
template <int B, int NV, bool MAX = false>
__device__ __forceinline__ void ordered_finish(const double *__restrict__ partials, int64_t count, int stride, int column, double (&out)[NV], double *sh)
{
    const int t = threadIdx.x;
    double a[NV];
#pragma unroll
    for (int c = 0; c < NV; c++) a[c] = 0.0;
    for (int64_t k = t; k < count; k += B) {
#pragma unroll
        for (int c = 0; c < NV; c++) a[c] = ordered_op<MAX>(a[c], partials[k * stride + column + c]);
    }
#pragma unroll
    for (int c = 0; c < NV; c++) sh[c * B + t] = a[c];
    __syncthreads();
    for (int off = B / 2; off > 0; off >>= 1) {
        if (t < off) {
#pragma unroll
            for (int c = 0; c < NV; c++) sh[c * B + t] = ordered_op<MAX>(sh[c * B + t], sh[c * B + t + off]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < NV; c++) out[c] = sh[c * B];
    __syncthreads();
}

template <int B, bool MAX = false>
__device__ __forceinline__ double ordered_finish(const double *__restrict__ partials, int64_t count, int stride, int column, double *sh /* B */)
{
    double a[1];
    ordered_finish<B, 1, MAX>(partials, count, stride, column, a, sh);
    return a[0];
}

// one workgroup: losses[v] = (float)((the ordered sum over k < blocks of partials[k][v]) / count_v), v < 2 (nrf_normal_losses, nrf_ray_regularizers)
template <int B>
__global__ void __launch_bounds__(B) k_finish_loss_pair(int64_t blocks, const double *__restrict__ partials, double count0, double count1, float *__restrict__ losses)
{
    __shared__ double sh[2 * B];
    double a[2];
    ordered_finish<B, 2>(partials, blocks, 2, 0, a, sh);
    if (threadIdx.x == 0) { losses[0] = (float)(a[0] / count0); losses[1] = (float)(a[1] / count1); }
}

// ---- the packed 64-bit key of the mesh tools: (float_bits(value) << 32) | index.  value >= 0 (a squared distance, a depth, a ray parameter with -0 made +0), so its
// bit pattern orders as the value does: the minimum is the smallest value, ties to the smallest index, whatever order the keys arrive in ----
constexpr unsigned long long NN_NONE = ((unsigned long long)0x7f800000u << 32) | 0xffffffffu;          // value = +inf, index = -1: above every key with a valid index
constexpr unsigned long long NO_KEY = ~0ull;                                                              // the rasteriser's empty pixel: what a 0xFF memset leaves

__device__ __forceinline__ unsigned long long key_pack(float value, uint32_t index) { return ((unsigned long long)__float_as_uint(value) << 32) | index; }
__device__ __forceinline__ float key_value(unsigned long long k) { return __uint_as_float((uint32_t)(k >> 32)); }
__device__ __forceinline__ int32_t key_index(unsigned long long k) { return (int32_t)(uint32_t)k; }

// *at = min(*at, k) by agent-scope atomic min (coherent across the XCDs; executed at the memory side).  A plain load of the current key filters the atomics: keys
// only ever fall, so a stale load can only be larger than the current one and a skipped atomic would not have lowered the key
__device__ __forceinline__ void key_lower(unsigned long long *at, unsigned long long k) { if (k < *at) __hip_atomic_fetch_min(at, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- the block-wide minimum of a packed 64-bit key, in THREAD 0 (the brute-force fallbacks' one writer): wave tree (two 32-bit shuffles per step), one word per wave.
// sh: B / 64 words, still being read on return like ordered_block_sum's ----
template <int B>
__device__ __forceinline__ unsigned long long block_key_min(unsigned long long key, unsigned long long *sh)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t hi = __shfl_xor((uint32_t)(key >> 32), off, 64), lo = __shfl_xor((uint32_t)key, off, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        key = o < key ? o : key;
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {          // (its own key is wave 0's minimum)
#pragma unroll
        for (int k = 1; k < B / 64; k++) key = sh[k] < key ? sh[k] : key;
    }
    return key;
}

}  // namespace nrf
