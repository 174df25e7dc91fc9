// scan.h -- the block-wide prefix sum of the scan-ordered outputs (mesh.hip's vertex / face positions, components.hip's dense component ids).
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

}  // namespace nrf
