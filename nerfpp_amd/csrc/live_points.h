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

}  // namespace nrf
