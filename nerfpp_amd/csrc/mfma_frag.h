// mfma_frag.h -- device helpers the matrix-core kernels share: where the rows of a 32x32 D tile sit in a lane's registers, and the (hi, lo) fp16 split of
// fp32 values into operand fragments.  mlp_small_mfma.hip (and the other files profiles/pmc_latest.json stamps by their bytes: sigma_small_f32.hip, mlp_nerf_*)
// still carry copies of their own: they move here when the counter passes are next taken (tools/gpu_pmc_round.sh), which is what re-stamps the summary.
#pragma once

#include "common.h"

namespace nrf {

// neuron (row of a 32x32 D tile / k of the next layer) held by element j of lane-half h in k-step s of a 32-row tile: register 8s + j of lane half h
__host__ __device__ inline int perm_row(int s, int h, int j) { return 16 * s + 8 * (j >> 2) + 4 * h + (j & 3); }

// exact-fp32 kernels (sigma_*_f32.hip, 32x32x2 tiles): the neuron carried by row i of an m-tile, 2(4(i/8) + i%4) + (i/4)%2 -- register q of lane half hh of the D tile
// is then neuron 2q + hh, the B operand of k-step q of the next layer in natural ascending k (sigma_small_f32.hip has the formulation)
__host__ __device__ inline int row_neuron(int i) { return 2 * (4 * (i >> 3) + (i & 3)) + ((i >> 2) & 1); }

// Two fp32 values -> packed (hi, lo) fp16 pairs: v = hi + lo to 22 bits.
// VALU cost matters here (a split kernel converts as many values as it multiplies tiles): half a v_cvt_pk_f16_f32 (RNE) per value, and lo = f16(v - hi) as ONE
// mixed-precision FMA that reads hi as a half and writes a half (v_fma_mixlo/mixhi_f16: fma(f32(hi), -1, v), exact difference, rounded once) -- which the
// compiler does not select by itself (it emits cvt + sub + cvt).  The asm only ever reads compiler-produced VALU results, never an MFMA result directly,
// so the MFMA -> VALU hazard handling stays with the compiler: a caller passes the result of a max / an add / a copy, not a matrix instruction's destination.
__device__ __forceinline__ void split_pair(float v0, float v1, uint32_t &hi, uint32_t &lo)
{
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(hi) : "v"(v0), "v"(v1));
    asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(lo) : "v"(hi), "v"(v0));
    asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(lo) : "v"(hi), "v"(v1));
}

}  // namespace nrf
