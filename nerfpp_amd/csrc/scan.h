// scan.h -- the block-level integer bookkeeping behind every scan-ordered output (counts -> offsets), in one place.  A tool counts per element, totals per block,
// scans the block totals in one workgroup and places every element by a block-local scan; what it needs for that is here and it writes none of it itself:
//   block_count<B>             how many threads of the block set a flag (one ballot, one barrier pair)
//   block_rank<B>              how many set flags come before this thread's, and the block's count
//   block_sum<T, B>            the block's integer total (wave shuffle tree + one LDS word per wave)
//   block_exclusive_scan<T, B> exclusive prefix sum over the block and its total (also the render path's live_points.hip)
//   k_block_sums<C, B>         kernel: bsum[block] = the sum of the block's B counts
//   block_totals_scan / k_totals_scan<T, TOTAL>   one workgroup of SCAN_BLOCK threads, SCAN_ITEMS entries each per round: block totals -> block offsets, *total = the sum
//   wave_append                a wave's flagged lanes onto an unordered list: one returning atomic per wave (the fallback and wide lists of the mesh tools)
// The pass that turns block offsets into element positions does site-specific work besides and stays with its tool.
#pragma once

#include "common.h"

namespace nrf {

constexpr int SCAN_BLOCK = 1024;         // threads of the one-workgroup scan of block totals
constexpr int SCAN_ITEMS = 8;            // entries per thread and round of it

// the count of set flags over the block, in every thread.  sh: B / 64 ints
template <int B>
__device__ __forceinline__ int block_count(bool flag, int *sh)
{
    const unsigned long long bal = __ballot(flag);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = __popcll(bal);
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int w = 0; w < B / 64; w++) total += sh[w];
    __syncthreads();
    return total;
}

// the count of set flags in the block before this thread's; `total` = the block's count.  sh: B / 64 ints
template <int B>
__device__ __forceinline__ int block_rank(bool flag, int *sh, int &total)
{
    const unsigned long long bal = __ballot(flag);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sh[wave] = __popcll(bal);
    __syncthreads();
    int before = __popcll(bal & ((1ull << lane) - 1ull));
    total = 0;
#pragma unroll
    for (int w = 0; w < B / 64; w++) {
        const int c = sh[w];
        if (w < wave) before += c;
        total += c;
    }
    __syncthreads();
    return before;
}

// list[...] = value for the lanes with `take`, in any order; one atomic add per wave.  EVERY lane of the wave must call it: the ballot is the whole wave's
__device__ __forceinline__ void wave_append(bool take, int32_t value, int32_t *__restrict__ list, uint32_t *__restrict__ count)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long m = __ballot(take);
    if (!m) return;          // uniform
    uint32_t at = 0;
    if (lane == 0) at = atomicAdd(count, (uint32_t)__popcll(m));
    at = __shfl(at, 0, 64);
    if (take) list[at + __popcll(m & ((1ull << lane) - 1))] = value;
}

// the sum of v over the block, in every thread (integers: the grouping does not matter).  sh: B / 64 entries
template <class T, int B>
__device__ __forceinline__ T block_sum(T v, T *sh)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    T total = 0;
#pragma unroll
    for (int w = 0; w < B / 64; w++) total += sh[w];
    __syncthreads();
    return total;
}

// exclusive scan over the block (Hillis-Steele in LDS); `total` = the block's sum
template <class T, int B>
__device__ __forceinline__ T block_exclusive_scan(T v, T *sh, T &total)
{
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int off = 1; off < B; off <<= 1) {
        const T t = tid >= off ? sh[tid - off] : T(0);
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
    }
    total = sh[B - 1];
    const T incl = sh[tid];
    __syncthreads();
    return incl - v;
}

// one workgroup of B threads: exclusive scan of bsum[0 .. nb) in place; returns the sum in every thread.  Every thread takes ITEMS consecutive entries per round, so 44 k block totals
// (a mesh of 11 M faces) are six rounds of the block scan at B = 1024, ITEMS = 8, not forty-four.  sh: B entries of LDS
template <class T, int B, int ITEMS>
__device__ __forceinline__ T block_totals_scan(int64_t nb, T *__restrict__ bsum, T *sh)
{
    T carry = 0;
    for (int64_t b0 = 0; b0 < nb; b0 += (int64_t)B * ITEMS) {
        const int64_t first = b0 + (int64_t)threadIdx.x * ITEMS;
        T v[ITEMS], sum = 0;
#pragma unroll
        for (int k = 0; k < ITEMS; k++) {
            v[k] = first + k < nb ? bsum[first + k] : T(0);
            sum += v[k];
        }
        T t;
        T run = carry + block_exclusive_scan<T, B>(sum, sh, t);
#pragma unroll
        for (int k = 0; k < ITEMS; k++) {
            if (first + k < nb) bsum[first + k] = run;
            run += v[k];
        }
        carry += t;
    }
    return carry;
}

// bsum[block] = the sum of the block's B counts (C: int32_t or uint32_t; a block's sum can pass 2^31, the int64 it lands in cannot overflow)
template <class C, int B>
__global__ void __launch_bounds__(B) k_block_sums(int64_t n, const C *__restrict__ count, int64_t *__restrict__ bsum)
{
    __shared__ int64_t sh[B / 64];
    const int64_t i = (int64_t)blockIdx.x * B + threadIdx.x;
    const int64_t total = block_sum<int64_t, B>(i < n ? (int64_t)count[i] : 0, sh);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one workgroup of SCAN_BLOCK threads: exclusive scan of bsum[0 .. nb) in place; *total = the sum, in the type of the header word it goes to
template <class T, class TOTAL>
__global__ void __launch_bounds__(SCAN_BLOCK) k_totals_scan(int64_t nb, T *__restrict__ bsum, TOTAL *__restrict__ total)
{
    __shared__ T sh[SCAN_BLOCK];
    const T sum = block_totals_scan<T, SCAN_BLOCK, SCAN_ITEMS>(nb, bsum, sh);
    if (threadIdx.x == 0) *total = (TOTAL)sum;
}

}  // namespace nrf
