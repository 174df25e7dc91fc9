// live_points.h -- compaction of the points with sigma > 0 (live_points.hip), for render.hip and the nrf_live_points entry.
#pragma once

#include "workspace.h"

namespace nrf {

struct LiveWs {
    int32_t *sums;          // per-workgroup live counts, scanned in place
};
LiveWs live_points_layout(Bump &b, int64_t p);
// list [p] int32 (the first *count entries are written, ascending), count [1] int32, rows [p, 4] or NULL: see live_points.hip.  1 <= p < 2^31, no host synchronisation
int live_points_launch(const float *sigma, int64_t p, int32_t *list, int32_t *count, float *rows, const LiveWs &w, hipStream_t st);
int live_colour_on();          // nrf_get_live_colour

// The renderer's resampling as one kernel (composite.hip: k_resample) and the same list from what it leaves behind.  launch_resample: sigma [n, s] -> z_fine, src, z_new
// as launch_raw2outputs(exact, weights only) + launch_fine_depths give them, bit for bit; w_out (the coarse weights) and counts are optional.  With counts [n] (16-byte
// aligned) it also leaves every ray's number of sigma > 0 there and the ray's ballot masks in the first bytes of the ray's rows [n * s, 4]; live_from_masks_launch then
// makes list / count / dead rows exactly as live_points_launch does.  counts holds ray_counts_len(n) int32: the n counts, then the list offsets of the groups of 64 rays
// (the scan's output).  2 <= s <= 256, 1 <= ns <= 256, n (s + ns) < 2^31.
int64_t ray_counts_len(int64_t n);
struct RngRef;
int launch_resample(const float *z, const float *sigma, const float *dirs, int d_stride, int64_t n, int s, const float *u, int64_t u_stride, const RngRef &g, int ns,
                    int sum_vec, float *zf, int32_t *src, float *z_new, float *w_out, int32_t *counts, float *rows, hipStream_t st);
int live_from_masks_launch(const float *sigma, int64_t n, int s, int32_t *counts, int32_t *list, int32_t *count, float *rows, hipStream_t st);
int fused_resample_on();       // nrf_get_fused_resample

}  // namespace nrf
