// geometry.hip -- comparing surfaces in space: an area-weighted sampling of a triangle list (nrf_mesh_sample_count / _emit), the nearest neighbour of every point of
// one set in another (nrf_nearest_points) and the sums a Chamfer distance or an F-score is made of (nrf_distance_stats).  The reference has none of it; the contract is
// stated in include/nerfpp_hip.h and restated in numpy by tests/geometry_ref.py, which the GPU tests compare with bit for bit.
//
// Sampling.  k_sample_faces: one lane per face -- indices checked before anything is read, the fp32 area, the face's point count n_f (floor of area * density plus
//   one Bernoulli draw of the fraction), the block's total of n_f and its ordered fp64 sum of the areas (reduce.h).  k_totals_scan (scan.h, one workgroup) turns the block totals into block
//   offsets, k_geo_finish adds the area partials in reduce.h's finish pass, k_sample_offsets writes every face's first point.  The emit kernel runs one lane per
//   POINT and finds its face by a binary search in the offsets: a face clamped to NRF_SAMPLE_MAX_PER_FACE points costs its lanes nothing extra.  Every position comes
//   from an integer prefix sum and every draw is a pure function of (seed, stream, index): two runs give the same arrays.
// Nearest points.  A uniform grid over the caller's box: k_nn_bin<0> (one non-returning atomic add per finite target), the scan of the cell counts (scan.h's k_block_sums
//   and k_totals_scan, then k_nn_cell_starts), k_nn_bin<1> (16-byte records {x, y, z, index} in cell order; the order INSIDE a cell is whatever the atomics gave).  k_nn_query:
//   one lane per query scans rings of cells outward, every ring as contiguous runs of records (the x-neighbours of a row are one range of the start array), keeps the
//   minimum of reduce.h's packed key (d2, index) and stops by the rule the header proves.  A query still open after NRF_NN_MAX_RINGS
//   rings is appended to a list (scan.h's wave_append); k_nn_far, a fixed grid of workgroups, brute-forces all records for each listed query with a block-wide minimum.
//   Both form d2 in nn_d2: one copy of the arithmetic.  The result depends on neither the grid, the scheduling nor the order of the targets (beyond the key's tie-break).
// Statistics.  k_dist_stats: 4096 entries per block, lane t takes t, t + 256, ... in ascending order; reduce.h's ordered block sum (block maximum) per column, one row of
//   eight fp64 partials per block; k_geo_finish is reduce.h's ordered finish pass per column.  No atomics.
// Closest point on a mesh.  The same grid holds FACES: k_fg_bin<0> counts one reference per cell of a face's cell box (a box of more than NRF_FG_MAX_FACE_CELLS cells:
//   the large list), the scan, k_fg_starts (starts into the caller's grid buffer, with what it was built for at its head), k_fg_bin<1> scatters face indices.
//   k_cm_query: one lane per query, the large list, then k_nn_query's ring walk over references, the same stop; k_cm_far brute-forces all faces for the listed
//   queries.  cm_take / cm_closest are the one copy of the candidate: Ericson's regions in a fixed order, P clamped to the face's coordinate box (the stop's proof
//   needs it), d2 through nn_d2.  tests/closest_ref.py restates it.  What a reader of the grid buffer needs (the grid, the buffer's layout and head, cm_face, the
//   clamp) lives in face_grid.h, which raycast.hip shares; so do cm_closest, CmHit and nn_d2, which voxel.hip scatters over a lattice.
// Every loop is bounded by a clamped range or a count; no kernel waits on another workgroup.
#include "reduce.h"
#include "scan.h"
#include "workspace.h"
#include "face_grid.h"
#include "nrf_rng.h"

#include <climits>
#include <cmath>

namespace nrf {

namespace {

// GEO_BLOCK, FAR_GRID, the grid and everything a reader of the face-grid buffer needs: face_grid.h (shared with raycast.hip)
constexpr int STATS_TILE = 4096;         // entries per block of k_dist_stats
constexpr int STATS_VALUES = 8;          // count, sum d, sum d2, max d, four tau counts

// out[v] = the ordered sum over k of partials[k * nv + v] (v == max_at: the maximum), v < n_out: one block, reduce.h's finish pass per column
__global__ void __launch_bounds__(GEO_BLOCK) k_geo_finish(int64_t count, int nv, int max_at, const double *__restrict__ partials, double *__restrict__ out, int n_out)
{
    __shared__ double s_a[GEO_BLOCK];
    for (int v = 0; v < n_out; v++) {
        const double a = v == max_at ? ordered_finish<GEO_BLOCK, true>(partials, count, nv, v, s_a) : ordered_finish<GEO_BLOCK>(partials, count, nv, v, s_a);
        if (threadIdx.x == 0) out[v] = a;
    }
}

// ---------------------------------------------------------------------------------------------- 1. surface sampling
struct SampleWs {
    int64_t *header;         // [0] the number of points; [1] the bits of the fp64 total area
    int32_t *count;          // [F] n_f
    int32_t *offset;         // [F] the face's first point
    int64_t *bsum;           // [blocks] n_f per block of 256 faces, scanned in place
    double *area;            // [blocks] the area partials
};

SampleWs sample_layout(Bump &b, int64_t n_faces)
{
    SampleWs s;
    const size_t nb = (size_t)ceil_div(n_faces > 0 ? n_faces : 1, GEO_BLOCK);
    s.header = b.take<int64_t>(4);
    s.count = b.take<int32_t>((size_t)n_faces);
    s.offset = b.take<int32_t>((size_t)n_faces);
    s.bsum = b.take<int64_t>(nb);
    s.area = b.take<double>(nb);
    return s;
}

// the corners of face f; false (nothing dereferenced) where an index lies outside [0, V)
__device__ __forceinline__ bool face_corners(const float *__restrict__ verts, int32_t n_verts, const int32_t *__restrict__ faces, int64_t f, float v0[3], float e1[3], float e2[3],
                                             bool &finite)
{
    const int32_t i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    if (i0 < 0 || i0 >= n_verts || i1 < 0 || i1 >= n_verts || i2 < 0 || i2 >= n_verts) return false;
    float v1[3], v2[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        v0[a] = verts[(int64_t)i0 * 3 + a];
        v1[a] = verts[(int64_t)i1 * 3 + a];
        v2[a] = verts[(int64_t)i2 * 3 + a];
        e1[a] = v1[a] - v0[a];
        e2[a] = v2[a] - v0[a];
    }
    finite = finite3(v0) && finite3(v1) && finite3(v2);
    return true;
}

__global__ void __launch_bounds__(GEO_BLOCK) k_sample_faces(const float *__restrict__ verts, int32_t n_verts, const int32_t *__restrict__ faces, int64_t n_faces, float density,
                                                            uint64_t seed, int32_t *__restrict__ count, int64_t *__restrict__ bsum, double *__restrict__ area_part,
                                                            uint32_t *__restrict__ stats)
{
    __shared__ int sh[GEO_BLOCK / 64];
    __shared__ double s_wave[GEO_BLOCK / 64];
    const int64_t f = (int64_t)blockIdx.x * GEO_BLOCK + threadIdx.x;
    int n = 0, cls = -1;          // class 0 bad index, 1 non-finite, 2 clamped
    double area64 = 0.0;
    if (f < n_faces) {
        float v0[3], e1[3], e2[3];
        bool finite = false;
        if (!face_corners(verts, n_verts, faces, f, v0, e1, e2, finite)) {
            cls = 0;
        } else {
            const float cx = e1[1] * e2[2] - e1[2] * e2[1];
            const float cy = e1[2] * e2[0] - e1[0] * e2[2];
            const float cz = e1[0] * e2[1] - e1[1] * e2[0];
            const float s = (cx * cx + cy * cy) + cz * cz;
            const float area = 0.5f * sqrtf(s);
            if (!finite || !isfinite(area)) {
                cls = 1;
            } else {
                area64 = (double)area;
                const float a = area * density;
                const float fa = floorf(a);
                if (fa > (float)NRF_SAMPLE_MAX_PER_FACE) {          // also a == +inf; the conversion below is defined
                    n = NRF_SAMPLE_MAX_PER_FACE;
                    cls = 2;
                } else {
                    n = (int)fa + (nrf_rng_uniform(seed, NRF_RNG_SURFACE_COUNT, (uint64_t)f) < a - fa ? 1 : 0);
                    if (n > NRF_SAMPLE_MAX_PER_FACE) { n = NRF_SAMPLE_MAX_PER_FACE; cls = 2; }
                }
            }
        }
        count[f] = n;
    }
    const int total = block_sum<int, GEO_BLOCK>(n, sh);
    const double part = ordered_block_sum<GEO_BLOCK>(area64, s_wave);
    if (threadIdx.x == 0) {
        bsum[blockIdx.x] = total;
        area_part[blockIdx.x] = part;
    }
    if (!stats) return;          // uniform
    const int t0 = block_count<GEO_BLOCK>(cls == 0, sh), t1 = block_count<GEO_BLOCK>(cls == 1, sh), t2 = block_count<GEO_BLOCK>(cls == 2, sh);
    if (threadIdx.x == 0) {          // counts: their values do not depend on the order of the additions
        if (t0) atomicAdd(stats + 0, (uint32_t)t0);
        if (t1) atomicAdd(stats + 1, (uint32_t)t1);
        if (t2) atomicAdd(stats + 2, (uint32_t)t2);
    }
}

__global__ void __launch_bounds__(GEO_BLOCK) k_sample_offsets(int64_t n_faces, const int32_t *__restrict__ count, const int64_t *__restrict__ bsum,
                                                              int32_t *__restrict__ offset)
{
    __shared__ int sh[GEO_BLOCK];
    const int64_t f = (int64_t)blockIdx.x * GEO_BLOCK + threadIdx.x;
    int total;
    const int e = block_exclusive_scan<int, GEO_BLOCK>(f < n_faces ? count[f] : 0, sh, total);
    const int64_t at = bsum[blockIdx.x] + e;
    if (f < n_faces) offset[f] = at > INT32_MAX ? INT32_MAX : (int32_t)at;          // a total beyond int32 is refused by the count call: nothing is emitted from it
}

__global__ void __launch_bounds__(GEO_BLOCK) k_sample_points(const float *__restrict__ verts, int32_t n_verts, const int32_t *__restrict__ faces, int64_t n_faces, uint64_t seed,
                                                             int64_t n_points, const int64_t *__restrict__ header, const int32_t *__restrict__ offset,
                                                             float *__restrict__ points, int32_t *__restrict__ out_face, float *__restrict__ out_uv)
{
    const int64_t p = (int64_t)blockIdx.x * GEO_BLOCK + threadIdx.x;
    if (p >= n_points || p >= header[0]) return;          // never beyond the caller's buffers, never beyond what the count call laid out
    // the last face whose first point is <= p: faces without points share their successor's offset, so this is the face that owns p
    int64_t lo = 0, hi = n_faces;                         // offset[lo] <= p < offset[hi] (offset[n_faces] = the total)
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)offset[mid] <= p) lo = mid;
        else hi = mid;
    }
    const int64_t f = lo;
    float u = nrf_rng_uniform(seed, NRF_RNG_SURFACE_UV, 2 * (uint64_t)p);
    float v = nrf_rng_uniform(seed, NRF_RNG_SURFACE_UV, 2 * (uint64_t)p + 1);
    if (u + v > 1.0f) { u = 1.0f - u; v = 1.0f - v; }
    float v0[3] = {0.0f, 0.0f, 0.0f}, e1[3] = {0.0f, 0.0f, 0.0f}, e2[3] = {0.0f, 0.0f, 0.0f};
    bool finite;
    (void)face_corners(verts, n_verts, faces, f, v0, e1, e2, finite);          // true: the count call gave points to valid faces only
#pragma unroll
    for (int a = 0; a < 3; a++) points[p * 3 + a] = (v0[a] + u * e1[a]) + v * e2[a];
    if (out_face) out_face[p] = (int32_t)f;
    if (out_uv) { out_uv[p * 2 + 0] = u; out_uv[p * 2 + 1] = v; }
}

#ifdef NRF_SAMPLE_EMIT_BY_FACE
// the alternative the header leaves open, for tuning builds (make EXTRA=-DNRF_SAMPLE_EMIT_BY_FACE): one lane per FACE writes its n_f points; same bits
__global__ void __launch_bounds__(GEO_BLOCK) k_sample_points_by_face(const float *__restrict__ verts, int32_t n_verts, const int32_t *__restrict__ faces, int64_t n_faces,
                                                                     uint64_t seed, int64_t n_points, const int64_t *__restrict__ header, const int32_t *__restrict__ count,
                                                                     const int32_t *__restrict__ offset, float *__restrict__ points, int32_t *__restrict__ out_face,
                                                                     float *__restrict__ out_uv)
{
    const int64_t f = (int64_t)blockIdx.x * GEO_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    const int n = count[f];
    if (n <= 0) return;
    const int64_t first = offset[f], limit = n_points < header[0] ? n_points : header[0];
    if (first < 0) return;          // not a workspace of the count call
    float v0[3], e1[3], e2[3];
    bool finite;
    if (!face_corners(verts, n_verts, faces, f, v0, e1, e2, finite)) return;
    for (int64_t p = first; p < first + n && p < limit; p++) {
        float u = nrf_rng_uniform(seed, NRF_RNG_SURFACE_UV, 2 * (uint64_t)p);
        float v = nrf_rng_uniform(seed, NRF_RNG_SURFACE_UV, 2 * (uint64_t)p + 1);
        if (u + v > 1.0f) { u = 1.0f - u; v = 1.0f - v; }
#pragma unroll
        for (int a = 0; a < 3; a++) points[p * 3 + a] = (v0[a] + u * e1[a]) + v * e2[a];
        if (out_face) out_face[p] = (int32_t)f;
        if (out_uv) { out_uv[p * 2 + 0] = u; out_uv[p * 2 + 1] = v; }
    }
}
#endif

// ---------------------------------------------------------------------------------------------- 2. nearest points
struct NnWs {
    uint32_t *start;         // [cells + 1] counts, then the exclusive scan: the records of cell c are start[c] .. start[c + 1]
    uint32_t *cursor;        // [cells] where the next record of a cell goes
    int64_t *bsum;           // [cell blocks]
    int64_t *total;          // [1]
    float4 *rec;             // [nt] {x, y, z, index bits} in cell order
    FarList far;             // [nq] the queries of the brute-force kernel
};

NnWs nn_layout(Bump &b, int64_t nq, int64_t nt, int64_t cells)
{
    NnWs s;
    s.start = b.take<uint32_t>((size_t)cells + 1);
    s.cursor = b.take<uint32_t>((size_t)cells);
    s.bsum = b.take<int64_t>((size_t)ceil_div(cells, GEO_BLOCK));
    s.total = b.take<int64_t>(1);
    s.rec = b.take<float4>((size_t)nt);
    s.far = far_layout(b, nq);
    return s;
}

__device__ __forceinline__ int64_t nn_cell_of(const NnGrid &g, float x, float y, float z)
{
    const int cx = nn_cell(x, g.bmin[0], g.inv_h[0], g.n[0]), cy = nn_cell(y, g.bmin[1], g.inv_h[1], g.n[1]), cz = nn_cell(z, g.bmin[2], g.inv_h[2], g.n[2]);
    return ((int64_t)cz * g.n[1] + cy) * g.n[0] + cx;
}

__device__ __forceinline__ void nn_take(float qx, float qy, float qz, const float4 &t, float md2, unsigned long long &best)
{
    const float d2 = nn_d2(qx, qy, qz, t);
    const unsigned long long k = key_pack(d2, __float_as_uint(t.w));
    if (d2 <= md2 && k < best) best = k;
}

// pass 0: count[cell]++ per finite target; pass 1: the record goes to cursor[cell]++
template <int PASS>
__global__ void __launch_bounds__(GEO_BLOCK) k_nn_bin(const float *__restrict__ target, int64_t nt, NnGrid g, uint32_t *__restrict__ cell_word, float4 *__restrict__ rec,
                                                      uint32_t *__restrict__ stats)
{
    __shared__ int sh[GEO_BLOCK / 64];
    const int64_t j = (int64_t)blockIdx.x * GEO_BLOCK + threadIdx.x;
    bool bad = false;
    if (j < nt) {
        const float x = target[j * 3 + 0], y = target[j * 3 + 1], z = target[j * 3 + 2];
        if (isfinite(x) && isfinite(y) && isfinite(z)) {
            const int64_t c = nn_cell_of(g, x, y, z);
            if (PASS == 0) {
                (void)__hip_atomic_fetch_add(cell_word + c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);          // the result is unused: no return trip
            } else {
                const uint32_t at = atomicAdd(cell_word + c, 1u);          // < the finite targets <= nt: every target is counted once and placed once
                rec[at] = make_float4(x, y, z, __uint_as_float((uint32_t)j));
            }
        } else {
            bad = true;
        }
    }
    if (PASS != 0 || !stats) return;          // uniform
    const int total = block_count<GEO_BLOCK>(bad, sh);
    if (threadIdx.x == 0 && total) atomicAdd(stats + 1, (uint32_t)total);
}

// counts -> starts in place (start[cells] = the number of records), and the scatter's cursors
__global__ void __launch_bounds__(GEO_BLOCK) k_nn_cell_starts(int64_t cells, uint32_t *__restrict__ start, const int64_t *__restrict__ bsum, uint32_t *__restrict__ cursor)
{
    __shared__ int sh[GEO_BLOCK];
    const int64_t c = (int64_t)blockIdx.x * GEO_BLOCK + threadIdx.x;
    const int n = c < cells ? (int)start[c] : 0;
    int total;
    const int e = block_exclusive_scan<int, GEO_BLOCK>(n, sh, total);
    if (c >= cells) return;
    const uint32_t at = (uint32_t)(bsum[blockIdx.x] + e);
    start[c] = at;
    cursor[c] = at;
    if (c == cells - 1) start[cells] = at + (uint32_t)n;
}

__global__ void __launch_bounds__(GEO_BLOCK) k_nn_query(const float *__restrict__ query, int64_t nq, NnGrid g, float md2, const uint32_t *__restrict__ start,
                                                        const float4 *__restrict__ rec, float *__restrict__ dist2, int32_t *__restrict__ index, int32_t *__restrict__ far,
                                                        uint32_t *__restrict__ n_far, uint32_t *__restrict__ stats)
{
    __shared__ int sh[GEO_BLOCK / 64];
    const int64_t q = (int64_t)blockIdx.x * GEO_BLOCK + threadIdx.x;
    const bool live = q < nq;
    float qx = 0.0f, qy = 0.0f, qz = 0.0f;
    if (live) { qx = query[q * 3 + 0]; qy = query[q * 3 + 1]; qz = query[q * 3 + 2]; }
    const bool finite = live && isfinite(qx) && isfinite(qy) && isfinite(qz);
    unsigned long long best = NN_NONE;
    bool open = false;          // rings exhausted without a stop: the brute-force kernel's
    if (finite && start[g.cells] != 0) {
        const int cx = nn_cell(qx, g.bmin[0], g.inv_h[0], g.n[0]), cy = nn_cell(qy, g.bmin[1], g.inv_h[1], g.n[1]), cz = nn_cell(qz, g.bmin[2], g.inv_h[2], g.n[2]);
        // the ring that completes the grid as seen from this cell
        const int r_all = max(max(max(cx, g.n[0] - 1 - cx), max(cy, g.n[1] - 1 - cy)), max(cz, g.n[2] - 1 - cz));
        open = true;
        for (int r = 0; r <= NRF_NN_MAX_RINGS; r++) {
            const int z0 = max(cz - r, 0), z1 = min(cz + r, g.n[2] - 1), y0 = max(cy - r, 0), y1 = min(cy + r, g.n[1] - 1);
            const int x0 = max(cx - r, 0), x1 = min(cx + r, g.n[0] - 1);
            for (int z = z0; z <= z1; z++) {
                for (int y = y0; y <= y1; y++) {
                    const int64_t row = ((int64_t)z * g.n[1] + y) * g.n[0];
                    const bool shell = z == cz - r || z == cz + r || y == cy - r || y == cy + r;          // the whole row belongs to ring r
                    if (shell) {
                        const uint32_t a = start[row + x0], b = start[row + x1 + 1];
                        for (uint32_t i = a; i < b; i++) nn_take(qx, qy, qz, rec[i], md2, best);
                    } else {                                                                                 // r >= 1: the two end cells, where the grid has them
                        if (cx - r >= 0) {
                            const uint32_t a = start[row + cx - r], b = start[row + cx - r + 1];
                            for (uint32_t i = a; i < b; i++) nn_take(qx, qy, qz, rec[i], md2, best);
                        }
                        if (cx + r <= g.n[0] - 1) {
                            const uint32_t a = start[row + cx + r], b = start[row + cx + r + 1];
                            for (uint32_t i = a; i < b; i++) nn_take(qx, qy, qz, rec[i], md2, best);
                        }
                    }
                }
            }
            if (r >= r_all) { open = false; break; }          // every cell has been scanned
            const float B = ((float)r * g.h_min) * 0.999f;
            const float B2 = B * B;
            // every unscanned target has d2 >= B2 (header): a strictly smaller best cannot be beaten or tied, and beyond max_dist nothing counts
            if (fminf(key_value(best), md2) < B2) { open = false; break; }
        }
    }
    wave_append(open, (int32_t)q, far, n_far);          // the walk has rejoined: every lane of the wave arrives here.  Every query is appended at most once
    if (live && !open) {
        dist2[q] = key_value(best);
        index[q] = key_index(best);
    }
    if (!stats) return;          // uniform
    const int total = block_count<GEO_BLOCK>(live && !finite, sh);
    if (threadIdx.x == 0 && total) atomicAdd(stats + 0, (uint32_t)total);
}

__global__ void __launch_bounds__(GEO_BLOCK) k_nn_far(const float *__restrict__ query, float md2, const uint32_t *__restrict__ start, int64_t cells,
                                                      const float4 *__restrict__ rec, float *__restrict__ dist2, int32_t *__restrict__ index, const int32_t *__restrict__ far,
                                                      const uint32_t *__restrict__ n_far, uint32_t *__restrict__ stats)
{
    __shared__ unsigned long long s_best[GEO_BLOCK / 64];
    const uint32_t n = *n_far, n_rec = start[cells];
    if (stats && blockIdx.x == 0 && threadIdx.x == 0 && n) atomicAdd(stats + 2, n);
    for (uint32_t i = blockIdx.x; i < n; i += FAR_GRID) {          // uniform over the workgroup
        const int64_t q = far[i];
        const float qx = query[q * 3 + 0], qy = query[q * 3 + 1], qz = query[q * 3 + 2];
        unsigned long long best = NN_NONE;
        for (uint32_t t = threadIdx.x; t < n_rec; t += GEO_BLOCK) nn_take(qx, qy, qz, rec[t], md2, best);
        best = block_key_min<GEO_BLOCK>(best, s_best);
        if (threadIdx.x == 0) {
            dist2[q] = key_value(best);
            index[q] = key_index(best);
        }
        __syncthreads();          // the next query goes through the same words
    }
}

// ---------------------------------------------------------------------------------------------- 3. distance statistics
struct Taus {
    float t[NRF_STATS_MAX_TAU];
    int n;
};

struct StatsWs {
    double *partials;          // [blocks][8]
};

int64_t stats_blocks(int64_t n) { return n > 0 ? ceil_div(n, STATS_TILE) : 1; }

void stats_layout(Bump &b, int64_t n, StatsWs &ws) { ws.partials = b.take<double>((size_t)stats_blocks(n) * STATS_VALUES); }

__global__ void __launch_bounds__(GEO_BLOCK) k_dist_stats(const float *__restrict__ d2, int64_t n, Taus taus, double *__restrict__ partials)
{
    __shared__ double s_wave[GEO_BLOCK / 64];
    const int t = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * STATS_TILE;
    const int64_t left = n - first;
    const int cnt = left < STATS_TILE ? (int)(left > 0 ? left : 0) : STATS_TILE;
    double acc[STATS_VALUES] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int e = t; e < cnt; e += GEO_BLOCK) {
        const float v = d2[first + e];
        if (!isfinite(v)) continue;
        const float d = sqrtf(v);
        acc[0] += 1.0;
        acc[1] += (double)d;
        acc[2] += (double)v;
        acc[3] = fmax(acc[3], (double)d);
#pragma unroll
        for (int k = 0; k < NRF_STATS_MAX_TAU; k++)
            if (k < taus.n && d <= taus.t[k]) acc[4 + k] += 1.0;
    }
#pragma unroll
    for (int v = 0; v < STATS_VALUES; v++) {
        const double a = v == 3 ? ordered_block_max<GEO_BLOCK>(acc[3], s_wave) : ordered_block_sum<GEO_BLOCK>(acc[v], s_wave);
        if (t == 0) partials[(int64_t)blockIdx.x * STATS_VALUES + v] = a;
        __syncthreads();          // the next column goes through the same words
    }
}

// ---------------------------------------------------------------------------------------------- 4. closest point on a mesh
// FgKey, FgGrid and their makers, cm_face, cm_dot and the clamp: face_grid.h
struct FgWs {                // count and build
    uint32_t *count;         // [cells] references per cell
    uint32_t *cursor;        // [cells] where the next reference of a cell goes
    int64_t *bsum;           // [cell blocks]
    int64_t *total;          // [1] n_refs
    uint32_t *counters;      // [0] n_large (count), [1] the large list's cursor (build)
};

struct CmWs {
    FarList far;             // [nq] the queries of the brute-force kernel
};

FgWs fg_ws_layout(Bump &b, int64_t cells)
{
    FgWs s;
    s.count = b.take<uint32_t>((size_t)cells);
    s.cursor = b.take<uint32_t>((size_t)cells);
    s.bsum = b.take<int64_t>((size_t)ceil_div(cells, GEO_BLOCK));
    s.total = b.take<int64_t>(1);
    s.counters = b.take<uint32_t>(2);
    return s;
}

CmWs cm_layout(Bump &b, int64_t nq)
{
    CmWs s;
    s.far = far_layout(b, nq);
    return s;
}

// the cell box of a face: per axis nn_cell(min of the three) .. nn_cell(max of the three); its cell count (<= 2^30)
__device__ __forceinline__ int64_t fg_box(const NnGrid &g, const float a[3], const float b[3], const float c[3], int lo[3], int hi[3])
{
    int64_t n = 1;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        lo[k] = nn_cell(fminf(fminf(a[k], b[k]), c[k]), g.bmin[k], g.inv_h[k], g.n[k]);
        hi[k] = nn_cell(fmaxf(fmaxf(a[k], b[k]), c[k]), g.bmin[k], g.inv_h[k], g.n[k]);
        n *= hi[k] - lo[k] + 1;
    }
    return n;
}

// cm_take and cm_write, a face as the candidate of a query (cm_closest(q, a, b, c, h) folded into the key) and the outputs of a query from its key: face_grid.h;
// bvh.hip forms both through the same two functions

// pass 0: count[cell]++ for every cell of a binned face's box, n_large++ for a large one; pass 1: the face's index goes to cursor[cell]++ resp. to the large list
template <int PASS>
__global__ void __launch_bounds__(GEO_BLOCK) k_fg_bin(const float *__restrict__ verts, int32_t n_verts, const int32_t *__restrict__ faces, int64_t n_faces, NnGrid g,
                                                      uint32_t *__restrict__ cell_word, uint32_t *__restrict__ counters, int32_t *__restrict__ refs, uint32_t n_refs,
                                                      int32_t *__restrict__ large, uint32_t n_large, uint32_t *__restrict__ stats)
{
    __shared__ int sh[GEO_BLOCK / 64];
    const int64_t f = (int64_t)blockIdx.x * GEO_BLOCK + threadIdx.x;
    int cls = -1;
    bool is_large = false;
    if (f < n_faces) {
        float a[3], b[3], c[3];
        cls = cm_face(verts, n_verts, faces, n_faces, f, a, b, c);
        if (cls == 0) {
            int lo[3], hi[3];
            is_large = fg_box(g, a, b, c, lo, hi) > NRF_FG_MAX_FACE_CELLS;
            if (!is_large) {
                for (int z = lo[2]; z <= hi[2]; z++)
                    for (int y = lo[1]; y <= hi[1]; y++)
                        for (int x = lo[0]; x <= hi[0]; x++) {          // at most NRF_FG_MAX_FACE_CELLS cells
                            const int64_t cell = ((int64_t)z * g.n[1] + y) * g.n[0] + x;
                            if (PASS == 0) {
                                (void)__hip_atomic_fetch_add(cell_word + cell, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            } else {
                                const uint32_t at = atomicAdd(cell_word + cell, 1u);
                                if (at < n_refs) refs[at] = (int32_t)f;          // always, for the workspace of the count call over this mesh
                            }
                        }
            } else if (PASS == 1) {
                const uint32_t at = atomicAdd(counters + 1, 1u);
                if (at < n_large) large[at] = (int32_t)f;
            }
        }
    }
    if (PASS != 0) return;          // uniform
    const int nl = block_count<GEO_BLOCK>(is_large, sh);
    if (threadIdx.x == 0 && nl) atomicAdd(counters + 0, (uint32_t)nl);
    if (!stats) return;             // uniform
    const int t1 = block_count<GEO_BLOCK>(cls == 1, sh), t2 = block_count<GEO_BLOCK>(cls == 2, sh);
    if (threadIdx.x == 0) {
        if (t1) atomicAdd(stats + 1, (uint32_t)t1);
        if (t2) atomicAdd(stats + 2, (uint32_t)t2);
    }
}

// counts -> the grid buffer's starts (start[cells] = n_refs) and the scatter's cursors; block 0 writes what the buffer is built for
__global__ void __launch_bounds__(GEO_BLOCK) k_fg_starts(int64_t cells, const uint32_t *__restrict__ count, const int64_t *__restrict__ bsum, uint32_t *__restrict__ start,
                                                         uint32_t *__restrict__ cursor, FgKey key, long long *__restrict__ out_key)
{
    __shared__ uint32_t sh[GEO_BLOCK];
    const int64_t c = (int64_t)blockIdx.x * GEO_BLOCK + threadIdx.x;
    const uint32_t n = c < cells ? count[c] : 0u;
    uint32_t total;
    const uint32_t e = block_exclusive_scan<uint32_t, GEO_BLOCK>(n, sh, total);
    if (blockIdx.x == 0 && threadIdx.x < 8) out_key[threadIdx.x] = key.w[threadIdx.x];
    if (c >= cells) return;
    const uint32_t at = (uint32_t)(bsum[blockIdx.x] + e);
    start[c] = at;
    cursor[c] = at;
    if (c == cells - 1) start[cells] = at + n;
}

__global__ void __launch_bounds__(GEO_BLOCK) k_cm_query(const float *__restrict__ query, int64_t nq, const float *__restrict__ verts, int32_t n_verts,
                                                        const int32_t *__restrict__ faces, int64_t n_faces, NnGrid g, FgKey key, float md2,
                                                        const long long *__restrict__ grid_key, const uint32_t *__restrict__ start, const int32_t *__restrict__ refs,
                                                        const int32_t *__restrict__ large, float *__restrict__ dist2, int32_t *__restrict__ face, float *__restrict__ uv,
                                                        float *__restrict__ point, int32_t *__restrict__ far, uint32_t *__restrict__ n_far, uint32_t *__restrict__ stats)
{
    __shared__ int sh[GEO_BLOCK / 64];
    if (!fg_key_matches(grid_key, key)) return;          // uniform: not the buffer nrf_face_grid_build made for these arguments; nothing of it is read, nothing written
    const int64_t qi = (int64_t)blockIdx.x * GEO_BLOCK + threadIdx.x;
    const bool live = qi < nq;
    const uint32_t n_refs = (uint32_t)key.w[3], n_large = (uint32_t)key.w[4];
    float q[3] = {0.0f, 0.0f, 0.0f};
    if (live) { q[0] = query[qi * 3 + 0]; q[1] = query[qi * 3 + 1]; q[2] = query[qi * 3 + 2]; }
    const bool finite = live && finite3(q);
    unsigned long long best = NN_NONE;
    bool open = false;          // rings exhausted without a stop: the brute-force kernel's
    if (finite) {
        for (uint32_t i = 0; i < n_large; i++) cm_take(q, verts, n_verts, faces, n_faces, large[i], md2, best);
        auto run = [&](uint32_t a, uint32_t b) {          // the references of a run of cells; never beyond the list
            b = b < n_refs ? b : n_refs;
            for (uint32_t i = a; i < b; i++) cm_take(q, verts, n_verts, faces, n_faces, refs[i], md2, best);
        };
        if (n_refs != 0) {
            const int cx = nn_cell(q[0], g.bmin[0], g.inv_h[0], g.n[0]), cy = nn_cell(q[1], g.bmin[1], g.inv_h[1], g.n[1]), cz = nn_cell(q[2], g.bmin[2], g.inv_h[2], g.n[2]);
            const int r_all = max(max(max(cx, g.n[0] - 1 - cx), max(cy, g.n[1] - 1 - cy)), max(cz, g.n[2] - 1 - cz));
            open = true;
            for (int r = 0; r <= NRF_NN_MAX_RINGS; r++) {          // k_nn_query's walk, cell for cell
                const int z0 = max(cz - r, 0), z1 = min(cz + r, g.n[2] - 1), y0 = max(cy - r, 0), y1 = min(cy + r, g.n[1] - 1);
                const int x0 = max(cx - r, 0), x1 = min(cx + r, g.n[0] - 1);
                for (int z = z0; z <= z1; z++) {
                    for (int y = y0; y <= y1; y++) {
                        const int64_t row = ((int64_t)z * g.n[1] + y) * g.n[0];
                        const bool shell = z == cz - r || z == cz + r || y == cy - r || y == cy + r;
                        if (shell) {
                            run(start[row + x0], start[row + x1 + 1]);
                        } else {
                            if (cx - r >= 0) run(start[row + cx - r], start[row + cx - r + 1]);
                            if (cx + r <= g.n[0] - 1) run(start[row + cx + r], start[row + cx + r + 1]);
                        }
                    }
                }
                if (r >= r_all) { open = false; break; }
                const float B = ((float)r * g.h_min) * 0.999f;
                const float B2 = B * B;
                // the closest point of every face without a reference in the cube lies in a cell at least r + 1 away on some axis (the clamp): d2 >= B2 (header)
                if (fminf(key_value(best), md2) < B2) { open = false; break; }
            }
        }
    }
    wave_append(open, (int32_t)qi, far, n_far);          // the walk has rejoined: every lane of the wave arrives here.  Every query is appended at most once
    if (live && !open) cm_write(q, qi, best, verts, n_verts, faces, n_faces, dist2, face, uv, point);
    if (!stats) return;          // uniform
    const int total = block_count<GEO_BLOCK>(live && !finite, sh);
    if (threadIdx.x == 0 && total) atomicAdd(stats + 0, (uint32_t)total);
}

__global__ void __launch_bounds__(GEO_BLOCK) k_cm_far(const float *__restrict__ query, const float *__restrict__ verts, int32_t n_verts, const int32_t *__restrict__ faces,
                                                      int64_t n_faces, FgKey key, float md2, const long long *__restrict__ grid_key, float *__restrict__ dist2,
                                                      int32_t *__restrict__ face, float *__restrict__ uv, float *__restrict__ point, const int32_t *__restrict__ far,
                                                      const uint32_t *__restrict__ n_far, uint32_t *__restrict__ stats)
{
    __shared__ unsigned long long s_best[GEO_BLOCK / 64];
    if (!fg_key_matches(grid_key, key)) return;          // uniform, as in k_cm_query
    const uint32_t n = *n_far;
    if (stats && blockIdx.x == 0 && threadIdx.x == 0 && n) atomicAdd(stats + 3, n);
    for (uint32_t i = blockIdx.x; i < n; i += FAR_GRID) {          // uniform over the workgroup
        const int64_t qi = far[i];
        const float q[3] = {query[qi * 3 + 0], query[qi * 3 + 1], query[qi * 3 + 2]};
        unsigned long long best = NN_NONE;
        for (int64_t f = threadIdx.x; f < n_faces; f += GEO_BLOCK) cm_take(q, verts, n_verts, faces, n_faces, f, md2, best);
        best = block_key_min<GEO_BLOCK>(best, s_best);
        if (threadIdx.x == 0) cm_write(q, qi, best, verts, n_verts, faces, n_faces, dist2, face, uv, point);
        __syncthreads();          // the next query goes through the same words
    }
}

}  // namespace

}  // namespace nrf

using namespace nrf;

extern "C" {

size_t nrf_mesh_sample_workspace_bytes(int64_t n_verts, int64_t n_faces)
{
    if (!sample_shape_ok(n_verts, n_faces)) return 0;
    return measure([&](Bump &b) { sample_layout(b, n_faces); });
}

int nrf_mesh_sample_count(const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, float density, uint64_t seed, int64_t *n_points,
                          double *total_area, uint32_t *d_stats, void *d_workspace, size_t workspace_bytes, void *stream)
{
    NRF_CHECK_ARG(sample_shape_ok(n_verts, n_faces), "nrf_mesh_sample_count: %lld vertices, %lld faces (both 0 .. 2^31 - 1)", (long long)n_verts, (long long)n_faces);
    NRF_CHECK_ARG(n_points && total_area, "nrf_mesh_sample_count: null n_points or total_area");
    NRF_CHECK_ARG(n_faces == 0 || d_faces, "nrf_mesh_sample_count: null d_faces");
    NRF_CHECK_ARG(d_verts || n_verts == 0 || n_faces == 0, "nrf_mesh_sample_count: null d_verts");
    NRF_CHECK_ARG(std::isfinite(density) && density >= 0.0f, "nrf_mesh_sample_count: the density must be finite and >= 0 (got %g)", (double)density);
    NRF_CHECK_ARG(d_workspace && (reinterpret_cast<uintptr_t>(d_workspace) & 7) == 0, "nrf_mesh_sample_count: the workspace must be non-null and 8-byte aligned");
    Bump bump(d_workspace, workspace_bytes);
    const SampleWs ws = sample_layout(bump, n_faces);
    NRF_TRY(ws_check(bump, nrf_mesh_sample_workspace_bytes(n_verts, n_faces), "nrf_mesh_sample_count"));
    hipStream_t st = as_stream(stream);
    const int64_t nb = ceil_div(n_faces, GEO_BLOCK);
    NRF_HIP(hipMemsetAsync(ws.header, 0, 4 * sizeof(int64_t), st));
    if (n_faces > 0) {
        hipLaunchKernelGGL(k_sample_faces, dim3((unsigned)nb), dim3(GEO_BLOCK), 0, st, d_verts, (int32_t)n_verts, d_faces, n_faces, density, seed, ws.count, ws.bsum, ws.area,
                           d_stats);
        NRF_LAUNCH_CHECK();
        hipLaunchKernelGGL((k_totals_scan<int64_t, int64_t>), dim3(1), dim3(SCAN_BLOCK), 0, st, nb, ws.bsum, ws.header);
        NRF_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_geo_finish, dim3(1), dim3(GEO_BLOCK), 0, st, nb, 1, -1, (const double *)ws.area, reinterpret_cast<double *>(ws.header + 1), 1);
        NRF_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_sample_offsets, dim3((unsigned)nb), dim3(GEO_BLOCK), 0, st, n_faces, (const int32_t *)ws.count, (const int64_t *)ws.bsum, ws.offset);
        NRF_LAUNCH_CHECK();
    }
    int64_t h[2] = {0, 0};
    NRF_HIP(hipMemcpyAsync(h, ws.header, sizeof(h), hipMemcpyDeviceToHost, st));
    NRF_HIP(hipStreamSynchronize(st));
    *n_points = h[0];
    std::memcpy(total_area, &h[1], sizeof(double));
    NRF_CHECK_ARG(h[0] <= INT32_MAX, "nrf_mesh_sample_count: %lld points exceed the int32 range of the offsets (lower the density)", (long long)h[0]);
    return NRF_OK;
}

int nrf_mesh_sample_emit(const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, uint64_t seed, int64_t n_points, float *d_points,
                         int32_t *d_face, float *d_uv, void *d_workspace, size_t workspace_bytes, void *stream)
{
    NRF_CHECK_ARG(sample_shape_ok(n_verts, n_faces), "nrf_mesh_sample_emit: %lld vertices, %lld faces (both 0 .. 2^31 - 1)", (long long)n_verts, (long long)n_faces);
    NRF_CHECK_ARG(n_points >= 0 && n_points <= INT32_MAX, "nrf_mesh_sample_emit: %lld points (0 .. 2^31 - 1)", (long long)n_points);
    NRF_CHECK_ARG(n_points == 0 || (d_points && d_faces && d_verts && n_faces > 0 && n_verts > 0), "nrf_mesh_sample_emit: %lld points with a null d_points, d_faces or d_verts, or of an empty mesh",
                  (long long)n_points);
    NRF_CHECK_ARG(d_workspace && (reinterpret_cast<uintptr_t>(d_workspace) & 7) == 0, "nrf_mesh_sample_emit: the workspace must be non-null and 8-byte aligned");
    Bump bump(d_workspace, workspace_bytes);
    const SampleWs ws = sample_layout(bump, n_faces);
    NRF_TRY(ws_check(bump, nrf_mesh_sample_workspace_bytes(n_verts, n_faces), "nrf_mesh_sample_emit"));
    if (n_points == 0) return NRF_OK;
#ifdef NRF_SAMPLE_EMIT_BY_FACE
    hipLaunchKernelGGL(k_sample_points_by_face, dim3((unsigned)ceil_div(n_faces, GEO_BLOCK)), dim3(GEO_BLOCK), 0, as_stream(stream), d_verts, (int32_t)n_verts, d_faces, n_faces,
                       seed, n_points, (const int64_t *)ws.header, (const int32_t *)ws.count, (const int32_t *)ws.offset, d_points, d_face, d_uv);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
#endif
    hipLaunchKernelGGL(k_sample_points, dim3((unsigned)ceil_div(n_points, GEO_BLOCK)), dim3(GEO_BLOCK), 0, as_stream(stream), d_verts, (int32_t)n_verts, d_faces, n_faces, seed,
                       n_points, (const int64_t *)ws.header, (const int32_t *)ws.offset, d_points, d_face, d_uv);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

size_t nrf_nearest_points_workspace_bytes(int64_t nq, int64_t nt, int nx, int ny, int nz)
{
    if (!nn_shape_ok(nq, nt, nx, ny, nz)) return 0;
    return measure([&](Bump &b) { nn_layout(b, nq, nt, (int64_t)nx * ny * nz); });
}

int nrf_nearest_points(const float *d_query, int64_t nq, const float *d_target, int64_t nt, const float *bbox, int nx, int ny, int nz, float max_dist, float *d_dist2,
                       int32_t *d_index, uint32_t *d_stats, void *d_workspace, size_t workspace_bytes, void *stream)
{
    NRF_CHECK_ARG(nn_shape_ok(nq, nt, nx, ny, nz), "nrf_nearest_points: %lld queries, %lld targets (0 .. 2^31 - 1), grid %d x %d x %d (each 1 .. %d, product <= %d)",
                  (long long)nq, (long long)nt, nx, ny, nz, NRF_NN_MAX_DIM, NRF_NN_MAX_CELLS);
    NRF_CHECK_ARG(nq == 0 || (d_query && d_dist2 && d_index), "nrf_nearest_points: null d_query, d_dist2 or d_index");
    NRF_CHECK_ARG(nt == 0 || d_target, "nrf_nearest_points: null d_target");
    NRF_CHECK_ARG(bbox, "nrf_nearest_points: null bbox");
    NRF_CHECK_ARG(max_dist >= 0.0f, "nrf_nearest_points: max_dist must be >= 0 or +inf (got %g)", (double)max_dist);          // NaN fails
    NnGrid g;
    int axis = 0;
    NRF_CHECK_ARG(nn_grid_make(bbox, nx, ny, nz, g, axis), "nrf_nearest_points: empty, inverted or non-finite box on axis %d ([%g, %g])", axis, (double)bbox[axis],
                  (double)bbox[3 + axis]);
    NRF_CHECK_ARG(d_workspace && (reinterpret_cast<uintptr_t>(d_workspace) & 15) == 0, "nrf_nearest_points: the workspace must be non-null and 16-byte aligned");
    Bump bump(d_workspace, workspace_bytes);
    const NnWs ws = nn_layout(bump, nq, nt, g.cells);
    NRF_TRY(ws_check(bump, nrf_nearest_points_workspace_bytes(nq, nt, nx, ny, nz), "nrf_nearest_points"));
    if (nq == 0) return NRF_OK;
    hipStream_t st = as_stream(stream);
    const float md2 = max_dist * max_dist;
    const int64_t cb = ceil_div(g.cells, GEO_BLOCK);
    NRF_HIP(hipMemsetAsync(ws.start, 0, ((size_t)g.cells + 1) * sizeof(uint32_t), st));
    NRF_HIP(hipMemsetAsync(ws.far.n, 0, sizeof(uint32_t), st));
    if (nt > 0) {
        const unsigned tb = (unsigned)ceil_div(nt, GEO_BLOCK);
        hipLaunchKernelGGL(k_nn_bin<0>, dim3(tb), dim3(GEO_BLOCK), 0, st, d_target, nt, g, ws.start, ws.rec, d_stats);
        NRF_LAUNCH_CHECK();
        hipLaunchKernelGGL((k_block_sums<uint32_t, GEO_BLOCK>), dim3((unsigned)cb), dim3(GEO_BLOCK), 0, st, g.cells, (const uint32_t *)ws.start, ws.bsum);
        NRF_LAUNCH_CHECK();
        hipLaunchKernelGGL((k_totals_scan<int64_t, int64_t>), dim3(1), dim3(SCAN_BLOCK), 0, st, cb, ws.bsum, ws.total);
        NRF_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_nn_cell_starts, dim3((unsigned)cb), dim3(GEO_BLOCK), 0, st, g.cells, ws.start, (const int64_t *)ws.bsum, ws.cursor);
        NRF_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_nn_bin<1>, dim3(tb), dim3(GEO_BLOCK), 0, st, d_target, nt, g, ws.cursor, ws.rec, d_stats);
        NRF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_nn_query, dim3((unsigned)ceil_div(nq, GEO_BLOCK)), dim3(GEO_BLOCK), 0, st, d_query, nq, g, md2, (const uint32_t *)ws.start, (const float4 *)ws.rec,
                       d_dist2, d_index, ws.far.list, ws.far.n, d_stats);
    NRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_nn_far, dim3(FAR_GRID), dim3(GEO_BLOCK), 0, st, d_query, md2, (const uint32_t *)ws.start, g.cells, (const float4 *)ws.rec, d_dist2, d_index,
                       (const int32_t *)ws.far.list, (const uint32_t *)ws.far.n, d_stats);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

size_t nrf_distance_stats_workspace_bytes(int64_t n)
{
    if (n < 0 || n >= ((int64_t)1 << 40)) return 0;
    return measure([&](Bump &b) { StatsWs ws; stats_layout(b, n, ws); });
}

int nrf_distance_stats(const float *d_dist2, int64_t n, const float *taus, int n_tau, double *d_out, void *d_workspace, size_t workspace_bytes, void *stream)
{
    NRF_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 40), "nrf_distance_stats: %lld entries (0 .. 2^40 - 1)", (long long)n);
    NRF_CHECK_ARG(n_tau >= 0 && n_tau <= NRF_STATS_MAX_TAU, "nrf_distance_stats: %d thresholds (0 .. %d)", n_tau, NRF_STATS_MAX_TAU);
    NRF_CHECK_ARG(d_out && (d_dist2 || n == 0) && (taus || n_tau == 0), "nrf_distance_stats: null d_out, d_dist2 or taus");
    Taus t{};
    t.n = n_tau;
    for (int k = 0; k < n_tau; k++) {
        NRF_CHECK_ARG(std::isfinite(taus[k]) && taus[k] >= 0.0f, "nrf_distance_stats: threshold %d must be finite and >= 0 (got %g)", k, (double)taus[k]);
        t.t[k] = taus[k];
    }
    NRF_CHECK_ARG(d_workspace && (reinterpret_cast<uintptr_t>(d_workspace) & 7) == 0, "nrf_distance_stats: the workspace must be non-null and 8-byte aligned");
    Bump bump(d_workspace, workspace_bytes);
    StatsWs ws;
    stats_layout(bump, n, ws);
    NRF_TRY(ws_check(bump, nrf_distance_stats_workspace_bytes(n), "nrf_distance_stats"));
    hipStream_t st = as_stream(stream);
    const int64_t nb = stats_blocks(n);
    hipLaunchKernelGGL(k_dist_stats, dim3((unsigned)nb), dim3(GEO_BLOCK), 0, st, d_dist2, n, t, ws.partials);
    NRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_geo_finish, dim3(1), dim3(GEO_BLOCK), 0, st, nb, STATS_VALUES, 3, (const double *)ws.partials, d_out, 4 + n_tau);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

size_t nrf_face_grid_workspace_bytes(int64_t n_faces, int nx, int ny, int nz)
{
    if (!fg_shape_ok(0, n_faces, nx, ny, nz)) return 0;
    return measure([&](Bump &b) { fg_ws_layout(b, (int64_t)nx * ny * nz); });
}

size_t nrf_face_grid_bytes(int64_t n_faces, int nx, int ny, int nz, int64_t n_refs, int64_t n_large)
{
    if (!fg_shape_ok(0, n_faces, nx, ny, nz) || !fg_counts_ok(n_faces, n_refs, n_large)) return 0;
    return measure([&](Bump &b) { fg_grid_layout(b, (int64_t)nx * ny * nz, n_refs, n_large); });
}

// NRF_FG_CHECK_MESH, the argument checks the face-grid entries share: face_grid.h

int nrf_face_grid_count(const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, const float *bbox, int nx, int ny, int nz, int64_t *n_refs,
                        int64_t *n_large, uint32_t *d_stats, void *d_workspace, size_t workspace_bytes, void *stream)
{
    NRF_FG_CHECK_MESH("nrf_face_grid_count");
    NRF_CHECK_ARG(n_refs && n_large, "nrf_face_grid_count: null n_refs or n_large");
    NRF_CHECK_ARG(d_workspace && (reinterpret_cast<uintptr_t>(d_workspace) & 7) == 0, "nrf_face_grid_count: the workspace must be non-null and 8-byte aligned");
    Bump bump(d_workspace, workspace_bytes);
    const FgWs ws = fg_ws_layout(bump, g.cells);
    NRF_TRY(ws_check(bump, nrf_face_grid_workspace_bytes(n_faces, nx, ny, nz), "nrf_face_grid_count"));
    hipStream_t st = as_stream(stream);
    const int64_t cb = ceil_div(g.cells, GEO_BLOCK);
    NRF_HIP(hipMemsetAsync(ws.count, 0, (size_t)g.cells * sizeof(uint32_t), st));
    NRF_HIP(hipMemsetAsync(ws.total, 0, sizeof(int64_t), st));
    NRF_HIP(hipMemsetAsync(ws.counters, 0, 2 * sizeof(uint32_t), st));
    if (n_faces > 0) {
        hipLaunchKernelGGL(k_fg_bin<0>, dim3((unsigned)ceil_div(n_faces, GEO_BLOCK)), dim3(GEO_BLOCK), 0, st, d_verts, (int32_t)n_verts, d_faces, n_faces, g, ws.count,
                           ws.counters, (int32_t *)nullptr, 0u, (int32_t *)nullptr, 0u, d_stats);
        NRF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL((k_block_sums<uint32_t, GEO_BLOCK>), dim3((unsigned)cb), dim3(GEO_BLOCK), 0, st, g.cells, (const uint32_t *)ws.count, ws.bsum);
    NRF_LAUNCH_CHECK();
    hipLaunchKernelGGL((k_totals_scan<int64_t, int64_t>), dim3(1), dim3(SCAN_BLOCK), 0, st, cb, ws.bsum, ws.total);
    NRF_LAUNCH_CHECK();
    int64_t total = 0;
    uint32_t counters[2] = {0, 0};
    NRF_HIP(hipMemcpyAsync(&total, ws.total, sizeof(total), hipMemcpyDeviceToHost, st));
    NRF_HIP(hipMemcpyAsync(counters, ws.counters, sizeof(counters), hipMemcpyDeviceToHost, st));
    NRF_HIP(hipStreamSynchronize(st));
    *n_refs = total;
    *n_large = (int64_t)counters[0];
    NRF_CHECK_ARG(total < ((int64_t)1 << 32), "nrf_face_grid_count: %lld references are 2^32 or more, beyond the uint32 range of the cell starts (use a coarser grid)",
                  (long long)total);
    return NRF_OK;
}

int nrf_face_grid_build(const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, const float *bbox, int nx, int ny, int nz, int64_t n_refs,
                        int64_t n_large, void *d_grid, size_t grid_bytes, void *d_workspace, size_t workspace_bytes, void *stream)
{
    NRF_FG_CHECK_MESH("nrf_face_grid_build");
    NRF_CHECK_ARG(fg_counts_ok(n_faces, n_refs, n_large), "nrf_face_grid_build: %lld references (0 .. 2^32 - 1), %lld large faces (0 .. %lld): not the count call's",
                  (long long)n_refs, (long long)n_large, (long long)n_faces);
    NRF_CHECK_ARG(d_grid && (reinterpret_cast<uintptr_t>(d_grid) & 7) == 0, "nrf_face_grid_build: the grid buffer must be non-null and 8-byte aligned");
    NRF_CHECK_ARG(grid_bytes == nrf_face_grid_bytes(n_faces, nx, ny, nz, n_refs, n_large), "nrf_face_grid_build: a grid buffer of %zu bytes, nrf_face_grid_bytes gives %zu",
                  grid_bytes, nrf_face_grid_bytes(n_faces, nx, ny, nz, n_refs, n_large));
    NRF_CHECK_ARG(d_workspace && (reinterpret_cast<uintptr_t>(d_workspace) & 7) == 0, "nrf_face_grid_build: the workspace must be non-null and 8-byte aligned");
    Bump bump(d_workspace, workspace_bytes);
    const FgWs ws = fg_ws_layout(bump, g.cells);
    NRF_TRY(ws_check(bump, nrf_face_grid_workspace_bytes(n_faces, nx, ny, nz), "nrf_face_grid_build"));
    Bump gb(d_grid, grid_bytes);
    const FgGrid grid = fg_grid_layout(gb, g.cells, n_refs, n_large);
    hipStream_t st = as_stream(stream);
    const int64_t cb = ceil_div(g.cells, GEO_BLOCK);
    hipLaunchKernelGGL(k_fg_starts, dim3((unsigned)cb), dim3(GEO_BLOCK), 0, st, g.cells, (const uint32_t *)ws.count, (const int64_t *)ws.bsum, grid.start, ws.cursor,
                       fg_key(n_faces, nx, ny, nz, n_refs, n_large, bbox), grid.key);
    NRF_LAUNCH_CHECK();
    if (n_faces > 0) {
        hipLaunchKernelGGL(k_fg_bin<1>, dim3((unsigned)ceil_div(n_faces, GEO_BLOCK)), dim3(GEO_BLOCK), 0, st, d_verts, (int32_t)n_verts, d_faces, n_faces, g, ws.cursor,
                           ws.counters, grid.refs, (uint32_t)n_refs, grid.large, (uint32_t)n_large, (uint32_t *)nullptr);
        NRF_LAUNCH_CHECK();
    }
    return NRF_OK;
}

size_t nrf_closest_on_mesh_workspace_bytes(int64_t nq)
{
    if (nq < 0 || nq > INT32_MAX) return 0;
    return measure([&](Bump &b) { cm_layout(b, nq); });
}

int nrf_closest_on_mesh(const float *d_query, int64_t nq, const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, const float *bbox, int nx, int ny,
                        int nz, int64_t n_refs, int64_t n_large, const void *d_grid, size_t grid_bytes, float max_dist, float *d_dist2, int32_t *d_face, float *d_uv,
                        float *d_point, uint32_t *d_stats, void *d_workspace, size_t workspace_bytes, void *stream)
{
    NRF_CHECK_ARG(nq >= 0 && nq <= INT32_MAX, "nrf_closest_on_mesh: %lld queries (0 .. 2^31 - 1)", (long long)nq);
    NRF_FG_CHECK_MESH("nrf_closest_on_mesh");
    NRF_CHECK_ARG(nq == 0 || (d_query && d_dist2 && d_face), "nrf_closest_on_mesh: null d_query, d_dist2 or d_face");
    NRF_CHECK_ARG(max_dist >= 0.0f, "nrf_closest_on_mesh: max_dist must be >= 0 or +inf (got %g)", (double)max_dist);          // NaN fails
    NRF_CHECK_ARG(fg_counts_ok(n_faces, n_refs, n_large), "nrf_closest_on_mesh: %lld references (0 .. 2^32 - 1), %lld large faces (0 .. %lld): not the count call's",
                  (long long)n_refs, (long long)n_large, (long long)n_faces);
    NRF_CHECK_ARG(d_grid && (reinterpret_cast<uintptr_t>(d_grid) & 7) == 0, "nrf_closest_on_mesh: the grid buffer must be non-null and 8-byte aligned");
    NRF_CHECK_ARG(grid_bytes == nrf_face_grid_bytes(n_faces, nx, ny, nz, n_refs, n_large),
                  "nrf_closest_on_mesh: a grid buffer of %zu bytes was not built for these faces, dims and counts (nrf_face_grid_bytes gives %zu)", grid_bytes,
                  nrf_face_grid_bytes(n_faces, nx, ny, nz, n_refs, n_large));
    NRF_CHECK_ARG(d_workspace && (reinterpret_cast<uintptr_t>(d_workspace) & 7) == 0, "nrf_closest_on_mesh: the workspace must be non-null and 8-byte aligned");
    Bump bump(d_workspace, workspace_bytes);
    const CmWs ws = cm_layout(bump, nq);
    NRF_TRY(ws_check(bump, nrf_closest_on_mesh_workspace_bytes(nq), "nrf_closest_on_mesh"));
    if (nq == 0) return NRF_OK;
    Bump gb(const_cast<void *>(d_grid), grid_bytes);
    const FgGrid grid = fg_grid_layout(gb, g.cells, n_refs, n_large);
    hipStream_t st = as_stream(stream);
    const float md2 = max_dist * max_dist;
    const FgKey key = fg_key(n_faces, nx, ny, nz, n_refs, n_large, bbox);
    NRF_HIP(hipMemsetAsync(ws.far.n, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_cm_query, dim3((unsigned)ceil_div(nq, GEO_BLOCK)), dim3(GEO_BLOCK), 0, st, d_query, nq, d_verts, (int32_t)n_verts, d_faces, n_faces, g, key, md2,
                       (const long long *)grid.key, (const uint32_t *)grid.start, (const int32_t *)grid.refs, (const int32_t *)grid.large, d_dist2, d_face, d_uv, d_point, ws.far.list,
                       ws.far.n, d_stats);
    NRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cm_far, dim3(FAR_GRID), dim3(GEO_BLOCK), 0, st, d_query, d_verts, (const int32_t)n_verts, d_faces, n_faces, key, md2, (const long long *)grid.key,
                       d_dist2, d_face, d_uv, d_point, (const int32_t *)ws.far.list, (const uint32_t *)ws.far.n, d_stats);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

}  // extern "C"
