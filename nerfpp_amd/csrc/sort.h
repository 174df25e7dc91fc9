// sort.h -- a stable least-significant-digit radix sort of (uint32 key, int32 payload) pairs on scan.h's building blocks: nrf_sort_pairs_u32 (bvh.hip holds the C entry).
// Bits [begin_bit, end_bit) of the key in 8-bit digits, lowest digit first; equal keys keep their input order, so the result is np.argsort(masked keys, kind="stable").
// One pass over a digit:
//   k_sort_hist      a block takes SORT_TILE consecutive elements and counts its digits in LDS (integer atomics); count[digit * blocks + block], digit-major
//   k_block_sums, k_totals_scan (scan.h), k_sort_offsets      the exclusive scan of those 256 * blocks counts, in place: where the block's elements of a digit begin
//   k_sort_scatter   the block walks its tile in rounds of SORT_BLOCK elements in input order; an element's place is the block's offset of its digit, plus the
//                    block's elements of that digit in earlier rounds, plus its rank among the equal digits of its round (the block-local split: eight ballots give
//                    the lanes of the wave with the same digit, one LDS word per wave and digit orders the waves)
// Digit-major counts with ascending blocks, rounds in order and lanes in order make every pass stable.  The passes ping-pong between the output arrays and a pair of
// arrays in the caller-owned workspace so that the last pass lands in the outputs; the input is only read.  No synchronisation, no atomics on global memory: two runs
// give the same bytes.  0 <= n <= 2^31 - 1; n == 0 launches nothing.
#pragma once

#include "common.h"
#include "scan.h"
#include "workspace.h"

#include <climits>

namespace nrf {

constexpr int SORT_BLOCK = 256;                          // threads of a block
constexpr int SORT_ROUNDS = 8;                           // rounds of SORT_BLOCK elements a block takes
constexpr int SORT_TILE = SORT_BLOCK * SORT_ROUNDS;      // elements of a block
constexpr int SORT_DIGITS = 256;

struct SortWs {
    uint32_t *keys;          // [n] the other side of the ping-pong
    int32_t *values;         // [n]
    uint32_t *count;         // [256 * blocks] digit-major counts, then offsets
    int64_t *bsum;           // [ceil(256 * blocks / SORT_BLOCK)]
    int64_t *total;          // [1] n again: the scan's total has to go somewhere
};

inline int64_t sort_blocks(int64_t n) { return ceil_div(n, SORT_TILE); }

inline SortWs sort_layout(Bump &b, int64_t n)
{
    SortWs s;
    const int64_t counts = (int64_t)SORT_DIGITS * sort_blocks(n);
    s.keys = b.take<uint32_t>((size_t)n);
    s.values = b.take<int32_t>((size_t)n);
    s.count = b.take<uint32_t>((size_t)counts);
    s.bsum = b.take<int64_t>((size_t)ceil_div(counts, SORT_BLOCK));
    s.total = b.take<int64_t>(1);
    return s;
}

inline size_t sort_workspace_bytes(int64_t n)
{
    if (n < 0 || n > INT32_MAX) return 0;
    return measure([&](Bump &b) { sort_layout(b, n); });
}

__global__ void __launch_bounds__(SORT_BLOCK) k_sort_hist(const uint32_t *__restrict__ keys, int64_t n, int shift, uint32_t mask, int64_t blocks, uint32_t *__restrict__ count)
{
    __shared__ uint32_t hist[SORT_DIGITS];
    hist[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t first = (int64_t)blockIdx.x * SORT_TILE;
#pragma unroll
    for (int r = 0; r < SORT_ROUNDS; r++) {
        const int64_t i = first + r * SORT_BLOCK + threadIdx.x;
        if (i < n) atomicAdd(&hist[(keys[i] >> shift) & mask], 1u);
    }
    __syncthreads();
    count[(int64_t)threadIdx.x * blocks + blockIdx.x] = hist[threadIdx.x];
}

// counts -> offsets in place: one block per SORT_BLOCK counts, the block's offset from the scan of the block totals
__global__ void __launch_bounds__(SORT_BLOCK) k_sort_offsets(int64_t counts, uint32_t *__restrict__ count, const int64_t *__restrict__ bsum)
{
    __shared__ uint32_t sh[SORT_BLOCK];
    const int64_t c = (int64_t)blockIdx.x * SORT_BLOCK + threadIdx.x;
    const uint32_t v = c < counts ? count[c] : 0u;
    uint32_t total;
    const uint32_t e = block_exclusive_scan<uint32_t, SORT_BLOCK>(v, sh, total);
    if (c < counts) count[c] = (uint32_t)(bsum[blockIdx.x] + e);          // below n <= 2^31 - 1
}

// values_in == NULL: the payload is the element's index
__global__ void __launch_bounds__(SORT_BLOCK) k_sort_scatter(const uint32_t *__restrict__ keys_in, const int32_t *__restrict__ values_in, int64_t n, int shift, uint32_t mask,
                                                             int64_t blocks, const uint32_t *__restrict__ offset, uint32_t *__restrict__ keys_out,
                                                             int32_t *__restrict__ values_out)
{
    __shared__ uint32_t running[SORT_DIGITS];                          // where the block's next element of a digit goes
    __shared__ uint32_t in_wave[SORT_BLOCK / 64][SORT_DIGITS];         // this round's elements of a digit, per wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    running[threadIdx.x] = offset[(int64_t)threadIdx.x * blocks + blockIdx.x];
#pragma unroll
    for (int w = 0; w < SORT_BLOCK / 64; w++) in_wave[w][threadIdx.x] = 0u;
    __syncthreads();
    const int64_t first = (int64_t)blockIdx.x * SORT_TILE;
    for (int r = 0; r < SORT_ROUNDS; r++) {          // uniform over the block
        const int64_t i = first + r * SORT_BLOCK + threadIdx.x;
        const bool live = i < n;
        const uint32_t key = live ? keys_in[i] : 0u;
        const uint32_t digit = (key >> shift) & mask;
        // the lanes of this wave that are live and hold the same digit
        unsigned long long peers = __ballot(live);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const bool bit = (digit >> b) & 1u;
            const unsigned long long bal = __ballot(bit);
            peers &= bit ? bal : ~bal;
        }
        const int before = __popcll(peers & ((1ull << lane) - 1ull));
        if (live && before == 0) in_wave[wave][digit] = (uint32_t)__popcll(peers);          // the first of the peers writes their number
        __syncthreads();
        if (live) {
            uint32_t at = running[digit] + (uint32_t)before;
#pragma unroll
            for (int w = 0; w < SORT_BLOCK / 64; w++) at += w < wave ? in_wave[w][digit] : 0u;
            keys_out[at] = key;
            values_out[at] = values_in ? values_in[i] : (int32_t)i;
        }
        __syncthreads();
        uint32_t sum = 0u;          // thread d closes digit d's round
#pragma unroll
        for (int w = 0; w < SORT_BLOCK / 64; w++) {
            sum += in_wave[w][threadIdx.x];
            in_wave[w][threadIdx.x] = 0u;
        }
        running[threadIdx.x] += sum;
        __syncthreads();
    }
}

// begin_bit == end_bit: nothing to order, the pairs are copied
__global__ void __launch_bounds__(SORT_BLOCK) k_sort_copy(const uint32_t *__restrict__ keys_in, const int32_t *__restrict__ values_in, int64_t n, uint32_t *__restrict__ keys_out,
                                                          int32_t *__restrict__ values_out)
{
    const int64_t i = (int64_t)blockIdx.x * SORT_BLOCK + threadIdx.x;
    if (i >= n) return;
    keys_out[i] = keys_in[i];
    values_out[i] = values_in ? values_in[i] : (int32_t)i;
}

// the passes of one sort; every argument has been checked by the caller (0 < n <= 2^31 - 1, 0 <= begin_bit <= end_bit <= 32, ws laid out by sort_layout(n))
inline int sort_pairs_launch(const uint32_t *keys, const int32_t *values, int64_t n, int begin_bit, int end_bit, uint32_t *keys_out, int32_t *values_out, const SortWs &ws,
                             hipStream_t st)
{
    const int passes = (end_bit - begin_bit + 7) / 8;
    if (passes == 0) {
        hipLaunchKernelGGL(k_sort_copy, dim3((unsigned)ceil_div(n, SORT_BLOCK)), dim3(SORT_BLOCK), 0, st, keys, values, n, keys_out, values_out);
        NRF_LAUNCH_CHECK();
        return NRF_OK;
    }
    const int64_t blocks = sort_blocks(n), counts = (int64_t)SORT_DIGITS * blocks, cb = ceil_div(counts, SORT_BLOCK);
    const uint32_t *src_k = keys;
    const int32_t *src_v = values;
    for (int p = 0; p < passes; p++) {
        const int shift = begin_bit + 8 * p, width = end_bit - shift < 8 ? end_bit - shift : 8;
        const uint32_t mask = (1u << width) - 1u;
        const bool to_out = ((passes - 1 - p) & 1) == 0;          // the last pass lands in the outputs
        uint32_t *dst_k = to_out ? keys_out : ws.keys;
        int32_t *dst_v = to_out ? values_out : ws.values;
        hipLaunchKernelGGL(k_sort_hist, dim3((unsigned)blocks), dim3(SORT_BLOCK), 0, st, src_k, n, shift, mask, blocks, ws.count);
        NRF_LAUNCH_CHECK();
        hipLaunchKernelGGL((k_block_sums<uint32_t, SORT_BLOCK>), dim3((unsigned)cb), dim3(SORT_BLOCK), 0, st, counts, (const uint32_t *)ws.count, ws.bsum);
        NRF_LAUNCH_CHECK();
        hipLaunchKernelGGL((k_totals_scan<int64_t, int64_t>), dim3(1), dim3(SCAN_BLOCK), 0, st, cb, ws.bsum, ws.total);
        NRF_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_sort_offsets, dim3((unsigned)cb), dim3(SORT_BLOCK), 0, st, counts, ws.count, (const int64_t *)ws.bsum);
        NRF_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_sort_scatter, dim3((unsigned)blocks), dim3(SORT_BLOCK), 0, st, src_k, src_v, n, shift, mask, blocks, (const uint32_t *)ws.count, dst_k, dst_v);
        NRF_LAUNCH_CHECK();
        src_k = dst_k;
        src_v = dst_v;
    }
    return NRF_OK;
}

}  // namespace nrf
