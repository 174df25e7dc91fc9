// mfma_frag.h -- the one copy of what every matrix-core kernel needs (mlp_small_*, sigma_*_f32, mlp_nerf_*, mlp_lerf_*):
//   * the vector types of an operand fragment and of a D tile (half8, f32x16, f32x4, u32x4);
//   * where the rows of a 32x32 D tile sit in a lane's registers (perm_row, row_neuron) -- host packers use the same functions;
//   * the (hi, lo) fp16 split of fp32 values (split_pair) and the conversion of a finished tile into the next layer's operand fragments
//     (tile_to_frag, tile_to_frag2);
//   * the LDS-DMA weight stream of the kernels whose weights do not fit in LDS (stage_dma, stage_piece, stage_all).
// Every function is __forceinline__: a kernel's machine code does not depend on which file states it.  Nothing here assumes -fno-honor-nans; the files that
// want a ReLU to be a single v_max_f32 are built with it (Makefile).
#pragma once

#include "common.h"

#include <utility>

namespace nrf {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));       // one lane's share of a 32x32x16 operand fragment
typedef float f32x16 __attribute__((ext_vector_type(16)));        // one lane's share of a 32x32 D tile
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));       // a half8 as four packed words

// neuron (row of a 32x32 D tile / k of the next layer) held by element j of lane-half h in k-step s of a 32-row tile: register 8s + j of lane half h
__host__ __device__ inline int perm_row(int s, int h, int j) { return 16 * s + 8 * (j >> 2) + 4 * h + (j & 3); }

// exact-fp32 kernels (sigma_*_f32.hip, 32x32x2 tiles): the neuron carried by row i of an m-tile, 2(4(i/8) + i%4) + (i/4)%2 -- register q of lane half hh of the D tile
// is then neuron 2q + hh, the B operand of k-step q of the next layer in natural ascending k (sigma_small_f32.hip has the formulation)
__host__ __device__ inline int row_neuron(int i) { return 2 * (4 * (i >> 3) + (i & 3)) + ((i >> 2) & 1); }

// D tile registers 8s..8s+7 -> fp16 B fragment of k-step s (round to nearest even), optional ReLU
template <bool RELU>
__device__ __forceinline__ half8 tile_to_frag(const f32x16 &acc, int s)
{
    half8 r;
#pragma unroll
    for (int j = 0; j < 8; j++) r[j] = (_Float16)acc[8 * s + j];
    // ReLU after the (monotonic) rounding: max(round(x), 0) == round(max(x, 0)); packed, 4 v_pk_max_f16 instead of 8 v_max_f32
    if (RELU) r = __builtin_elementwise_max(r, half8{0, 0, 0, 0, 0, 0, 0, 0});
    return r;
}

// Two fp32 values -> packed (hi, lo) fp16 pairs: v = hi + lo to 22 bits.
// VALU cost matters here (a split kernel converts as many values as it multiplies tiles): half a v_cvt_pk_f16_f32 (RNE) per value, and lo = f16(v - hi) as ONE
// mixed-precision FMA that reads hi as a half and writes a half (v_fma_mixlo/mixhi_f16: fma(f32(hi), -1, v), exact difference, rounded once) -- which the
// compiler does not select by itself (it emits cvt + sub + cvt).  The asm only ever reads compiler-produced VALU results, never an MFMA result directly,
// so the MFMA -> VALU hazard handling stays with the compiler (it does not look into asm): a caller passes the result of a max / a multiply / a copy, not a
// matrix instruction's destination.
__device__ __forceinline__ void split_pair(float v0, float v1, uint32_t &hi, uint32_t &lo)
{
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(hi) : "v"(v0), "v"(v1));
    asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(lo) : "v"(hi), "v"(v0));
    asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(lo) : "v"(hi), "v"(v1));
}

// D tile registers 8s..8s+7 -> the (hi, lo) pair of B fragments of k-step s, each value through `pre` first: the vector instruction whose result split_pair's asm reads
template <class Pre>
__device__ __forceinline__ void tile_to_frag2_of(const f32x16 &acc, int s, Pre pre, half8 &hi, half8 &lo)
{
    union { half8 v; uint32_t u[4]; } h, l;
#pragma unroll
    for (int j = 0; j < 4; j++) split_pair(pre(acc[8 * s + 2 * j]), pre(acc[8 * s + 2 * j + 1]), h.u[j], l.u[j]);
    hi = h.v; lo = l.v;
}

// ... with the ReLU as that instruction, max(v, 0) (2.5 instructions per value: the max is one v_max_f32 where the file is built with -fno-honor-nans, otherwise
// fmaxf first canonicalises the MFMA result); without a ReLU a max with -FLT_MAX, the cheapest instruction that is the identity on every finite value
template <bool RELU>
__device__ __forceinline__ void tile_to_frag2(const f32x16 &acc, int s, half8 &hi, half8 &lo)
{
    tile_to_frag2_of(acc, s, [](float v) { return fmaxf(v, RELU ? 0.0f : -3.402823466e38f); }, hi, lo);
}

// ---- the weight stream: chunks of a weight image -> LDS by LDS-DMA (global_load_lds_dwordx4) ----
// One wave-instruction moves one 1-KB fragment (64 lanes x 16 B, lane-linear on both sides -- exactly the fragment layout); wave w of NW takes fragments w, w + NW, ...
// No staging registers (the register-staged version carried 20 VGPRs per thread in a kernel at the 256-VGPR cap) and no ds_write pass; the data is in flight while
// the running chunk's MFMAs execute and is retired by the counted vmcnt at the end of a chunk.  N is the net's chunk table (NerfNet, lerf::Net, NerfNetS, lerf::NetS).
//
// The address.  A fragment's address is an SGPR base + lane * 16, the saddr form of the DMA.  The base starts at the image pointer + the wave's share, is made opaque
// (asm volatile "+s") so that the addresses derived from it cannot be hoisted out of the persistent loop -- left to itself the compiler hoists every chunk's lane
// addresses as 64-bit VGPR pairs, or 533 SGPR pairs that spill -- then gets the fragment's constant offset added on the scalar side (s_add_u32 / s_addc_u32) and is
// made opaque again.  With the offset added BEHIND the second opaque point the compiler forms a 64-bit per-lane address instead: two v_lshl_add_u64 per DMA,
// ~1 070 per iteration of the classic split kernel.
//
// Callers pass `dst` (and the buffer they read, and their bias table) down as __restrict__ PARAMETERS of their chunk body on purpose: inlining turns that into
// alias-scope metadata on the LDS reads and on the DMA's LDS write, which is what lets the compiler see that the running chunk's reads do not touch the look-ahead's
// destination.  Without it every LDS read issued while an LDS-DMA is pending is preceded by s_waitcnt vmcnt(0) and the look-ahead is drained at the top of the chunk.

// fp16 kernels: the whole chunk CI in one burst
template <class N, int NW, int CI>
__device__ __forceinline__ void stage_dma(half8 *__restrict__ dst, const half8 *__restrict__ packed, int wave, int lane)
{
    constexpr int ci = CI % N::total_chunks();
    constexpr int nf = N::chunk_frags(ci);
    constexpr int base = N::chunk_off(ci);
#pragma unroll
    for (int q = 0; q < (nf + NW - 1) / NW; q++) {
        const half8 *pk = packed + (size_t)wave * 64;
        asm volatile("" : "+s"(pk));                     // not hoistable out of the persistent loop ...
        pk += (size_t)(base + q * NW) * 64;
        asm volatile("" : "+s"(pk));                     // ... and the offset added here, on the scalar side
        if (q * NW + wave < nf)                          // wave-uniform
            __builtin_amdgcn_global_load_lds(pk + lane, (__attribute__((address_space(3))) void *)(dst + (q * NW + wave) * 64), 16, 0, 0);
    }
}

// split kernels: piece Q (0 .. pieces per wave) of chunk CI, issued between the running chunk's matrix instructions.  N::dma_frags(ci) of the chunk's fragments
// travel (a multiple of NW), starting at k-step N::k0_dma(ci); N::hi_only(ci): every second fragment of the image (the hi ones), each into its usual slot.
template <class N, int NW, int CI, int Q>
__device__ __forceinline__ void stage_piece(half8 *__restrict__ dst, const half8 *__restrict__ packed, int wave, int lane)
{
    constexpr int ci = CI % N::total_chunks();
    constexpr int nf = N::dma_frags(ci);
    constexpr int STEP = N::hi_only(ci) ? 2 : 1;
    static_assert(nf % NW == 0, "fragments per chunk must divide by the wave count");
    if constexpr (Q * NW < nf) {
        constexpr int base = N::chunk_off(ci);
        const half8 *pk = packed + (size_t)wave * (64 * STEP);
        asm volatile("" : "+s"(pk));                          // opaque: not hoistable out of the persistent loop
        constexpr int F0 = 2 * N::k0_dma(ci);                 // first fragment of the chunk that travels
        pk += (size_t)(base + F0 + STEP * Q * NW) * 64;
        asm volatile("" : "+s"(pk));                          // the offset is added HERE, on the scalar side
        __builtin_amdgcn_global_load_lds(pk + lane, (__attribute__((address_space(3))) void *)(dst + (F0 + STEP * (Q * NW + wave)) * 64), 16, 0, 0);
    }
}

template <class N, int NW, int CI, int... Qs>
__device__ __forceinline__ void stage_all(half8 *__restrict__ dst, const half8 *__restrict__ packed, int wave, int lane, std::integer_sequence<int, Qs...>)
{
    (stage_piece<N, NW, CI, Qs>(dst, packed, wave, lane), ...);
}

}  // namespace nrf
