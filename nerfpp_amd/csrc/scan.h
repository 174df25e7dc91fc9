// scan.h -- the block-wide prefix sum of the scan-ordered outputs (mesh.hip's vertex / face positions, components.hip's dense component ids) and the one-workgroup scan
// of per-block totals (simplify.hip, smooth.hip).
#pragma once

#include "common.h"

namespace nrf {

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

// one workgroup of B threads: exclusive scan of bsum[0 .. nb) in place; *total = the sum.  Every thread takes ITEMS consecutive entries per round, so 44 k block totals
// (a mesh of 11 M faces) are six rounds of the block scan at B = 1024, ITEMS = 8, not forty-four.  sh: B entries of LDS
template <class T, int B, int ITEMS>
__device__ __forceinline__ void block_totals_scan(int64_t nb, T *__restrict__ bsum, T *__restrict__ total, T *sh)
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
    if (threadIdx.x == 0) *total = carry;
}

}  // namespace nrf
