// edge_fn.h -- the exact coverage test, the barycentrics and the pixel box that the rasteriser (raster.hip: pixels) and the voxeliser (voxel.hip: lattice columns)
// share, so that "the voxeliser's coverage is the rasteriser's" is one function.  Each tool keeps its own set-up of the edge functions (tri_setup, vx_setup).
#pragma once

#include "common.h"

namespace nrf {

// the pixel centres a face with snapped extremes [xmin, xmax] x [ymin, ymax] can cover: columns i0 .. i1 and rows j0 .. j1 (empty where i1 < i0 or j1 < j0).
// >> of a negative int is arithmetic: floor
__device__ __forceinline__ void edge_box(int xmin, int xmax, int ymin, int ymax, int n_cols, int n_rows, int &i0, int &i1, int &j0, int &j1)
{
    i0 = max((xmin + (NRF_RASTER_SUBPIXEL - 1)) >> 8, 0); i1 = min(xmax >> 8, n_cols - 1);
    j0 = max((ymin + (NRF_RASTER_SUBPIXEL - 1)) >> 8, 0); j1 = min(ymax >> 8, n_rows - 1);
}

// is the centre of pixel (column i, row j) covered?  e00 / sx / sy: the three edge functions at (0, 0) and their steps, times s = sign(A); tl: the top-left rule.
// Decided in int64 (exact): se[k] = e(0, 0) + i * step_x + j * step_y is the header's E_ab(p) whatever the visiting order
__device__ __forceinline__ bool edge_cover(const int64_t e00[3], const int64_t sx[3], const int64_t sy[3], const bool tl[3], int i, int j, int64_t se[3])
{
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        se[k] = e00[k] + (int64_t)i * sx[k] + (int64_t)j * sy[k];
        in = in && (se[k] > 0 || (se[k] == 0 && tl[k]));
    }
    return in;
}

// b[k] = (float)((double)se[k] / (double)sA): one fp64 division per barycentric
__device__ __forceinline__ void edge_bary(const int64_t se[3], int64_t sA, float b[3])
{
    const double den = (double)sA;
#pragma unroll
    for (int k = 0; k < 3; k++) b[k] = (float)((double)se[k] / den);
}

}  // namespace nrf
