// raycast.hip -- what a ray hits on a mesh: nrf_ray_cast_mesh (first hit / any hit over the face grid of geometry.hip), nrf_hemisphere_dirs (cosine-weighted
// directions around normals) and nrf_mesh_ambient_occlusion (the two fused: no ray or direction is written).  The reference has none of it; the contract and the
// argument why the walk cannot miss are stated in include/nerfpp_hip.h ("Ray casting on a mesh") and restated by brute force in tests/raycast_ref.py, which the
// GPU tests compare with bit for bit.
//
// Candidate.  rc_candidate is the one place a (ray, face) pair is judged: Moeller-Trumbore in the header's operation order, t + 0.0f, the acceptance tests, P clamped
//   to the face's box by face_grid.h's cm_clamp_to_face, and the consistency of t with P.  Walk, large list and fallback all come through rc_take.
// Premise.  k_rc_premise: one lane per face, a flag in the workspace where a valid face has a coordinate outside the grid's box.  The walk's clipping is only
//   complete when all faces lie inside; with the flag set every valid ray goes to the fallback.
// Walk.  rc_walk, one lane per ray: the far-origin test, the slab clip against the widened box, the large list, then uniform steps in t; every step looks up the
//   cells between its two end points widened by 2 tau_k, skipping those the previous step looked up, and stops by the header's rule.  It returns open where it
//   gives the ray up (far origin, a step that does not advance, NRF_RC_MAX_STEPS); k_rc_query appends such rays to a list (scan.h's wave_append) and k_rc_far,
//   a fixed grid of workgroups, brute-forces all faces for each listed ray with reduce.h's block-wide minimum of the packed key (t, face).
// Directions.  rc_hemisphere_dir: Marsaglia's disc rejection, no trigonometry; every draw a pure function of (seed, index, j, attempt).
// Ambient occlusion.  k_rc_ao: one lane per ray of the flattened [n, k] rays, the same rc_hemisphere_dir and rc_walk in any mode, a point's hits in a wave by
//   ballot and popcount into its integer counter; a ray the walk gives up is brute-forced by its whole wave on the spot, lanes over faces.  k_rc_ao_finish: d_ao.
// Every loop is bounded by a clamped range or a count; no kernel waits on another workgroup.
#include "reduce.h"
#include "scan.h"
#include "workspace.h"
#include "face_grid.h"
#include "raycast.h"
#include "nrf_rng.h"

#include <climits>
#include <cmath>

namespace nrf {

namespace {

constexpr float RC_SLACK = 1.0f / 1024.0f;         // the widening of the clip box and of the slab parameters

struct RcWs {
    FarList far;             // [n] the rays of the brute-force kernel
    uint32_t *outside;       // [1] != 0: some valid face has a coordinate outside the grid's box
};

RcWs rc_layout(Bump &b, int64_t n)
{
    RcWs s;
    s.far = far_layout(b, n, 2);          // two words: a single memset clears the length and the flag
    s.outside = s.far.n + 1;
    return s;
}

struct RcBox {
    float lo[3], hi[3];          // the grid's box, or the clip box: the grid's box widened by the header's margin on every side
};

// RcRay, RcHit, rc_candidate, rc_take: raycast.h

struct RcMesh {
    const float *verts;
    const int32_t *faces;
    const uint32_t *start;
    const int32_t *refs, *large;
    int32_t n_verts;
    int64_t n_faces;
    uint32_t n_refs, n_large;
};

// The walk of one ray (the header's WALK).  ANY: stop at the first accepted candidate.  Returns true where the ray is given up (the caller brute-forces it);
// otherwise best holds the answer (NN_NONE: a miss).
template <bool ANY>
__device__ __forceinline__ bool rc_walk(const RcRay &r, const RcMesh &m, const NnGrid &g, const RcBox &box, int cull, unsigned long long &best)
{
    best = NN_NONE;
    if (!(r.lo <= r.hi)) return false;                                   // an empty range
    if (4.0f * (RC_TAU * r.o_inf) > g.h_min) return true;                // a far origin: tau alone is a quarter of a cell
    float t0 = r.lo, t1 = r.hi;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        if (r.d[a] == 0.0f) {
            if (r.o[a] < box.lo[a] || r.o[a] > box.hi[a]) return false;
        } else {
            float ta = (box.lo[a] - r.o[a]) / r.d[a], tb = (box.hi[a] - r.o[a]) / r.d[a];
            if (ta > tb) { const float s = ta; ta = tb; tb = s; }
            if (ta > 0.0f) ta = ta * (1.0f - RC_SLACK);
            tb = tb * (1.0f + RC_SLACK);
            t0 = ta > t0 ? ta : t0;
            t1 = tb < t1 ? tb : t1;
        }
    }
    if (!(t0 <= t1)) return false;
    for (uint32_t i = 0; i < m.n_large; i++) {
        rc_take(r, m.verts, m.n_verts, m.faces, m.n_faces, m.large[i], cull, best);
        if (ANY && best != NN_NONE) return false;
    }
    if (m.n_refs == 0) return false;
    const float d_inf = fmaxf(fmaxf(fabsf(r.d[0]), fabsf(r.d[1])), fabsf(r.d[2]));
    const float dt = g.h_min / d_inf;
    float tk = t0;
    float pa[3];
#pragma unroll
    for (int a = 0; a < 3; a++) pa[a] = r.o[a] + tk * r.d[a];
    int plo[3] = {1, 1, 1}, phi[3] = {0, 0, 0};          // the previous lookup's cell range: empty
    for (int k = 1; k <= NRF_RC_MAX_STEPS; k++) {
        float tn = t0 + (float)k * dt;
        if (!(tn > tk)) return true;                                     // a step that does not advance (or a NaN)
        if (tn > t1 && t1 > tk) tn = t1;
        float pb[3], am = r.o_inf;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            pb[a] = r.o[a] + tn * r.d[a];
            am = fmaxf(am, fmaxf(fabsf(pa[a]), fabsf(pb[a])));
        }
        const float tau = RC_TAU * am;
        if (!(4.0f * tau <= g.h_min)) return true;                       // also a non-finite end point
        const float two = 2.0f * tau;
        int lo[3], hi[3];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            lo[a] = nn_cell(fminf(pa[a], pb[a]) - two, g.bmin[a], g.inv_h[a], g.n[a]);
            hi[a] = nn_cell(fmaxf(pa[a], pb[a]) + two, g.bmin[a], g.inv_h[a], g.n[a]);
        }
        const bool same = lo[0] == plo[0] && lo[1] == plo[1] && lo[2] == plo[2] && hi[0] == phi[0] && hi[1] == phi[1] && hi[2] == phi[2];
        if (!same) {
            for (int z = lo[2]; z <= hi[2]; z++) {
                for (int y = lo[1]; y <= hi[1]; y++) {
                    const int64_t row = ((int64_t)z * g.n[1] + y) * g.n[0];
                    const bool seen = z >= plo[2] && z <= phi[2] && y >= plo[1] && y <= phi[1];          // cells [plo[0], phi[0]] of this row: the previous lookup's
                    // the row's cells as at most two runs of references around the part already looked up
                    const int x1a = seen ? min(hi[0], plo[0] - 1) : hi[0];
                    const int x0b = seen ? max(lo[0], phi[0] + 1) : hi[0] + 1;
                    if (lo[0] <= x1a) {
                        uint32_t e = m.start[row + x1a + 1];
                        e = e < m.n_refs ? e : m.n_refs;
                        for (uint32_t i = m.start[row + lo[0]]; i < e; i++) rc_take(r, m.verts, m.n_verts, m.faces, m.n_faces, m.refs[i], cull, best);
                    }
                    if (x0b <= hi[0]) {
                        uint32_t e = m.start[row + hi[0] + 1];
                        e = e < m.n_refs ? e : m.n_refs;
                        for (uint32_t i = m.start[row + x0b]; i < e; i++) rc_take(r, m.verts, m.n_verts, m.faces, m.n_faces, m.refs[i], cull, best);
                    }
                }
            }
#pragma unroll
            for (int a = 0; a < 3; a++) { plo[a] = lo[a]; phi[a] = hi[a]; }
        }
        if (ANY ? best != NN_NONE : key_value(best) <= tn) return false;          // every accepted candidate with t <= tn has been seen
        if (tn >= t1) return false;                                              // the clipped range is exhausted
        tk = tn;
#pragma unroll
        for (int a = 0; a < 3; a++) pa[a] = pb[a];
    }
    return true;                                                                 // still open after NRF_RC_MAX_STEPS steps
}

// rc_write, rc_load_ray: raycast.h

// flag != 0 where a valid face has a coordinate outside [bmin, bmax] (the premise of the walk's clipping)
__global__ void __launch_bounds__(GEO_BLOCK) k_rc_premise(const float *__restrict__ verts, int32_t n_verts, const int32_t *__restrict__ faces, int64_t n_faces, RcBox grid_box,
                                                          uint32_t *__restrict__ flag)
{
    const int64_t f = (int64_t)blockIdx.x * GEO_BLOCK + threadIdx.x;
    bool out = false;
    float a[3], b[3], c[3];
    if (f < n_faces && cm_face(verts, n_verts, faces, n_faces, f, a, b, c) == 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float lo = fminf(fminf(a[k], b[k]), c[k]), hi = fmaxf(fmaxf(a[k], b[k]), c[k]);
            out = out || lo < grid_box.lo[k] || hi > grid_box.hi[k];
        }
    }
    if (__ballot(out) != 0ull && (threadIdx.x & 63) == 0) *flag = 1u;          // a plain vector store of the same value from every such wave
}

template <bool ANY>
__global__ void __launch_bounds__(GEO_BLOCK) k_rc_query(const float *__restrict__ rays, int64_t n, int stride, RcMesh m, NnGrid g, RcBox box, FgKey key, int cull,
                                                        const long long *__restrict__ grid_key, float *__restrict__ out_t, int32_t *__restrict__ face,
                                                        float *__restrict__ uv, float *__restrict__ point, uint8_t *__restrict__ hit, int32_t *__restrict__ far,
                                                        uint32_t *__restrict__ n_far, const uint32_t *__restrict__ outside, uint32_t *__restrict__ stats)
{
    __shared__ int sh[GEO_BLOCK / 64];
    if (!fg_key_matches(grid_key, key)) return;          // uniform: not the buffer nrf_face_grid_build made for these arguments; nothing of it is read, nothing written
    const int64_t i = (int64_t)blockIdx.x * GEO_BLOCK + threadIdx.x;
    const bool live = i < n;
    RcRay r;
    bool valid = false;
    if (live) valid = rc_load_ray(rays, i, stride, r);
    unsigned long long best = NN_NONE;
    bool open = false;
    if (valid) open = *outside != 0u ? r.lo <= r.hi : rc_walk<ANY>(r, m, g, box, cull, best);
    wave_append(open, (int32_t)i, far, n_far);          // the walk has rejoined: every lane of the wave arrives here.  Every ray is appended at most once
    if (live && !open) rc_write(r, i, best, m.verts, m.n_verts, m.faces, m.n_faces, cull, out_t, face, uv, point, hit);
    if (!stats) return;          // uniform
    const int total = block_count<GEO_BLOCK>(live && !valid, sh);
    if (threadIdx.x == 0 && total) atomicAdd(stats + 0, (uint32_t)total);
}

__global__ void __launch_bounds__(GEO_BLOCK) k_rc_far(const float *__restrict__ rays, int stride, RcMesh m, FgKey key, int cull, const long long *__restrict__ grid_key,
                                                      float *__restrict__ out_t, int32_t *__restrict__ face, float *__restrict__ uv, float *__restrict__ point,
                                                      uint8_t *__restrict__ hit, const int32_t *__restrict__ far, const uint32_t *__restrict__ n_far,
                                                      uint32_t *__restrict__ stats)
{
    __shared__ unsigned long long s_best[GEO_BLOCK / 64];
    if (!fg_key_matches(grid_key, key)) return;          // uniform, as in k_rc_query
    const uint32_t n = *n_far;
    if (stats && blockIdx.x == 0 && threadIdx.x == 0 && n) atomicAdd(stats + 3, n);
    for (uint32_t j = blockIdx.x; j < n; j += FAR_GRID) {          // uniform over the workgroup
        const int64_t i = far[j];
        RcRay r;
        (void)rc_load_ray(rays, i, stride, r);
        unsigned long long best = NN_NONE;
        for (int64_t f = threadIdx.x; f < m.n_faces; f += GEO_BLOCK) rc_take(r, m.verts, m.n_verts, m.faces, m.n_faces, f, cull, best);
        best = block_key_min<GEO_BLOCK>(best, s_best);
        if (threadIdx.x == 0) rc_write(r, i, best, m.verts, m.n_verts, m.faces, m.n_faces, cull, out_t, face, uv, point, hit);
        __syncthreads();          // the next ray goes through the same words
    }
}

// ---------------------------------------------------------------------------------------------- hemisphere directions
// n-hat of a normal, the header's form; false (zeros) for a zero or non-finite normal or a squared length that is 0 or not finite
__device__ __forceinline__ bool rc_unit_normal(const float n[3], float out[3])
{
    out[0] = out[1] = out[2] = 0.0f;
    if (!finite3(n)) return false;
    const float l2 = cm_dot(n, n);
    if (!(l2 > 0.0f) || !(l2 < INFINITY)) return false;
    const float len = __builtin_sqrtf(l2);
#pragma unroll
    for (int k = 0; k < 3; k++) out[k] = n[k] / len;
    return true;
}

// direction j of point `index` around the unit normal nh (the header's steps)
__device__ __forceinline__ void rc_hemisphere_dir(const float nh[3], uint64_t seed, uint64_t index, uint32_t j, float dir[3])
{
    float q[3] = {0.0f, 0.0f, 1.0f};
    const uint64_t base = (index << 20) | ((uint64_t)j << 4);
    for (uint32_t a = 0; a < NRF_HEMI_ATTEMPTS; a++) {
        const float x1 = 2.0f * nrf_rng_uniform(seed, NRF_RNG_HEMI_DIR, base | (2 * a)) - 1.0f;
        const float x2 = 2.0f * nrf_rng_uniform(seed, NRF_RNG_HEMI_DIR, base | (2 * a + 1)) - 1.0f;
        const float s = x1 * x1 + x2 * x2;
        if (s < 1.0f) {
            const float rr = __builtin_sqrtf(1.0f - s);
            q[0] = (2.0f * x1) * rr;
            q[1] = (2.0f * x2) * rr;
            q[2] = 1.0f - 2.0f * s;
            break;
        }
    }
    float v[3];
#pragma unroll
    for (int k = 0; k < 3; k++) v[k] = nh[k] + q[k];
    const float l2 = cm_dot(v, v);
    if (l2 < NRF_HEMI_MIN_LEN2) {
#pragma unroll
        for (int k = 0; k < 3; k++) dir[k] = nh[k];
    } else {
        const float len = __builtin_sqrtf(l2);
#pragma unroll
        for (int k = 0; k < 3; k++) dir[k] = v[k] / len;
    }
}

__global__ void __launch_bounds__(GEO_BLOCK) k_rc_dirs(const float *__restrict__ normals, int64_t n, int k, uint64_t seed, int64_t index0, float *__restrict__ dirs,
                                                       uint32_t *__restrict__ stats)
{
    __shared__ int sh[GEO_BLOCK / 64];
    const int64_t e = (int64_t)blockIdx.x * GEO_BLOCK + threadIdx.x;          // one lane per direction
    const bool live = e < n * k;
    bool bad = false;
    if (live) {
        const int64_t i = e / k;
        const uint32_t j = (uint32_t)(e - i * k);
        const float nrm[3] = {normals[i * 3 + 0], normals[i * 3 + 1], normals[i * 3 + 2]};
        float nh[3], dir[3] = {0.0f, 0.0f, 0.0f};
        if (rc_unit_normal(nrm, nh)) rc_hemisphere_dir(nh, seed, (uint64_t)(index0 + i), j, dir);
        else bad = j == 0;
        dirs[e * 3 + 0] = dir[0];
        dirs[e * 3 + 1] = dir[1];
        dirs[e * 3 + 2] = dir[2];
    }
    if (!stats) return;          // uniform
    const int total = block_count<GEO_BLOCK>(bad, sh);
    if (threadIdx.x == 0 && total) atomicAdd(stats + 0, (uint32_t)total);
}

// ---------------------------------------------------------------------------------------------- ambient occlusion
// One lane per ray over the flattened [n, k] rays (ray e = i * k + j), as the composition through nrf_ray_cast_mesh runs them: a wave holds the rays of 64 / k points
// where k is small and a part of a point's where it is large, and no lane idles for a k that is no multiple of 64.  (A wave per point with lanes over the k rays,
// the first form tried, ran BEHIND the composition at k = 16, where it leaves 48 of 64 lanes idle; tools/raycast_bench.py)  The hits of a point's rays
// in a wave are one ballot and a popcount under the point's lane mask, added to the point's integer counter in the workspace by its first lane; k_rc_ao_finish turns
// the counters into d_ao.  A ray the walk gives up is brute-forced by the whole wave on the spot, lanes over faces.
__global__ void __launch_bounds__(GEO_BLOCK) k_rc_ao(const float *__restrict__ points, const float *__restrict__ normals, int64_t n, int k, float offset, float max_dist,
                                                     uint64_t seed, int64_t index0, RcMesh m, NnGrid g, RcBox box, FgKey key, const long long *__restrict__ grid_key,
                                                     const uint32_t *__restrict__ outside, uint32_t *__restrict__ hits, uint32_t *__restrict__ stats)
{
    if (!fg_key_matches(grid_key, key)) return;          // uniform
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * GEO_BLOCK + threadIdx.x;
    const bool live = e < n * k;
    const int64_t i = live ? e / k : n;
    const int j = live ? (int)(e - i * k) : 0;
    RcRay r;
    bool valid = false, open = false;
    unsigned long long best = NN_NONE;
#pragma unroll
    for (int a = 0; a < 3; a++) r.o[a] = r.d[a] = 0.0f;
    if (live) {
        const float nrm[3] = {normals[i * 3 + 0], normals[i * 3 + 1], normals[i * 3 + 2]};
        float nh[3];
        const bool has_normal = rc_unit_normal(nrm, nh);
#pragma unroll
        for (int a = 0; a < 3; a++) r.o[a] = points[i * 3 + a] + offset * nh[a];
        if (has_normal) rc_hemisphere_dir(nh, seed, (uint64_t)(index0 + i), (uint32_t)j, r.d);
        rc_ray_finish(r, 0.0f, max_dist);
        valid = rc_ray_valid(r, 0.0f, max_dist);
        if (valid) open = *outside != 0u ? r.lo <= r.hi : rc_walk<true>(r, m, g, box, 0, best);
    }
    bool hit = best != NN_NONE;
    unsigned long long todo = __ballot(open);          // every lane of the wave arrives here
    const uint32_t fallback = (uint32_t)__popcll(todo);
    while (todo) {          // at most 64 rounds; uniform over the wave
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        RcRay s;
#pragma unroll
        for (int a = 0; a < 3; a++) { s.o[a] = __shfl(r.o[a], src, 64); s.d[a] = __shfl(r.d[a], src, 64); }
        rc_ray_finish(s, 0.0f, max_dist);
        unsigned long long b = NN_NONE;
        for (int64_t f0 = 0; f0 < m.n_faces; f0 += 64) {          // uniform; stops at the first slab of faces with a hit
            const int64_t f = f0 + lane;
            if (f < m.n_faces) rc_take(s, m.verts, m.n_verts, m.faces, m.n_faces, f, 0, b);
            if (__ballot(b != NN_NONE) != 0ull) break;
        }
        const bool found = __ballot(b != NN_NONE) != 0ull;
        if (lane == src) hit = found;
    }
    const unsigned long long hit_mask = __ballot(hit);
    const uint32_t invalid = (uint32_t)__popcll(__ballot(live && !valid));
    if (live && (lane == 0 || j == 0)) {          // the first lane of the point's rays in this wave: rays j .. j + len - 1 sit in lanes lane .. lane + len - 1
        const int len = min(k - j, 64 - lane);
        const unsigned long long mine = (len == 64 ? ~0ull : ((1ull << len) - 1ull)) << lane;
        const uint32_t c = (uint32_t)__popcll(hit_mask & mine);
        if (c) atomicAdd(hits + i, c);          // integer: the sum does not depend on the order
    }
    if (lane == 0 && stats) {
        if (invalid) atomicAdd(stats + 0, invalid);
        if (fallback) atomicAdd(stats + 3, fallback);
    }
}

__global__ void __launch_bounds__(GEO_BLOCK) k_rc_ao_finish(int64_t n, int k, FgKey key, const long long *__restrict__ grid_key, const uint32_t *__restrict__ hits,
                                                            float *__restrict__ ao)
{
    if (!fg_key_matches(grid_key, key)) return;          // uniform: as k_rc_ao, nothing written
    const int64_t i = (int64_t)blockIdx.x * GEO_BLOCK + threadIdx.x;
    if (i < n) ao[i] = (float)((uint32_t)k - hits[i]) / (float)k;
}

bool rc_box_make(const float *bbox, const NnGrid &g, RcBox &grid_box, RcBox &clip)
{
    float b_inf = 0.0f;
    for (int a = 0; a < 6; a++) b_inf = std::fabs(bbox[a]) > b_inf ? std::fabs(bbox[a]) : b_inf;
    const float margin = g.h_min + RC_SLACK * b_inf;
    for (int a = 0; a < 3; a++) {
        grid_box.lo[a] = bbox[a];
        grid_box.hi[a] = bbox[3 + a];
        clip.lo[a] = bbox[a] - margin;
        clip.hi[a] = bbox[3 + a] + margin;
    }
    return std::isfinite(clip.lo[0]) && std::isfinite(clip.lo[1]) && std::isfinite(clip.lo[2]) && std::isfinite(clip.hi[0]) && std::isfinite(clip.hi[1]) &&
           std::isfinite(clip.hi[2]);
}

}  // namespace

}  // namespace nrf

using namespace nrf;

extern "C" {

size_t nrf_ray_cast_workspace_bytes(int64_t n_rays)
{
    if (n_rays < 0 || n_rays > INT32_MAX) return 0;
    return measure([&](Bump &b) { rc_layout(b, n_rays); });
}

// what nrf_ray_cast_mesh and nrf_mesh_ambient_occlusion do alike after their own checks: the grid's layout, the clip box, the premise pass
#define NRF_RC_PREPARE(who, n_items)                                                                                                                                       \
    NRF_FG_CHECK_GRID(who);                                                                                                                                               \
    NRF_CHECK_ARG(d_workspace && (reinterpret_cast<uintptr_t>(d_workspace) & 7) == 0, who ": the workspace must be non-null and 8-byte aligned");                         \
    Bump bump(d_workspace, workspace_bytes);                                                                                                                              \
    const RcWs ws = rc_layout(bump, n_items);                                                                                                                             \
    NRF_TRY(ws_check(bump, nrf_ray_cast_workspace_bytes(n_items), who));                                                                                                  \
    RcBox grid_box, clip;                                                                                                                                                 \
    NRF_CHECK_ARG(rc_box_make(bbox, g, grid_box, clip), who ": the box widened by a cell is not finite")

#define NRF_RC_LAUNCH_PREMISE()                                                                                                                                           \
    Bump gb(const_cast<void *>(d_grid), grid_bytes);                                                                                                                      \
    const FgGrid grid = fg_grid_layout(gb, g.cells, n_refs, n_large);                                                                                                     \
    hipStream_t st = as_stream(stream);                                                                                                                                   \
    const FgKey key = fg_key(n_faces, nx, ny, nz, n_refs, n_large, bbox);                                                                                                 \
    const RcMesh m = {d_verts, d_faces, grid.start, grid.refs, grid.large, (int32_t)n_verts, n_faces, (uint32_t)n_refs, (uint32_t)n_large};                               \
    NRF_HIP(hipMemsetAsync(ws.far.n, 0, 2 * sizeof(uint32_t), st));          /* the length and outside lie side by side */                                               \
    if (n_faces > 0) {                                                                                                                                                    \
        hipLaunchKernelGGL(k_rc_premise, dim3((unsigned)ceil_div(n_faces, GEO_BLOCK)), dim3(GEO_BLOCK), 0, st, d_verts, (int32_t)n_verts, d_faces, n_faces, grid_box,     \
                           ws.outside);                                                                                                                                   \
        NRF_LAUNCH_CHECK();                                                                                                                                               \
    }

int nrf_ray_cast_mesh(const float *d_rays, int64_t n_rays, int stride, const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, const float *bbox,
                      int nx, int ny, int nz, int64_t n_refs, int64_t n_large, const void *d_grid, size_t grid_bytes, int cull, int mode, float *d_t, int32_t *d_face,
                      float *d_uv, float *d_point, uint8_t *d_hit, uint32_t *d_stats, void *d_workspace, size_t workspace_bytes, void *stream)
{
    NRF_CHECK_ARG(n_rays >= 0 && n_rays <= INT32_MAX, "nrf_ray_cast_mesh: %lld rays (0 .. 2^31 - 1)", (long long)n_rays);
    NRF_CHECK_ARG(stride >= 8 && stride <= NRF_RC_MAX_STRIDE, "nrf_ray_cast_mesh: a ray stride of %d floats (8 .. %d)", stride, NRF_RC_MAX_STRIDE);
    NRF_FG_CHECK_MESH("nrf_ray_cast_mesh");
    NRF_CHECK_ARG(cull >= NRF_RC_CULL_NONE && cull <= NRF_RC_CULL_FRONT, "nrf_ray_cast_mesh: cull %d is none of NRF_RC_CULL_NONE / _BACK / _FRONT", cull);
    NRF_CHECK_ARG(mode == NRF_RC_CLOSEST || mode == NRF_RC_ANY, "nrf_ray_cast_mesh: mode %d is neither NRF_RC_CLOSEST nor NRF_RC_ANY", mode);
    NRF_CHECK_ARG(n_rays == 0 || d_rays, "nrf_ray_cast_mesh: null d_rays");
    NRF_CHECK_ARG(n_rays == 0 || mode != NRF_RC_CLOSEST || (d_t && d_face), "nrf_ray_cast_mesh: null d_t or d_face in closest mode");
    NRF_CHECK_ARG(n_rays == 0 || mode != NRF_RC_ANY || (d_hit && !d_t && !d_face && !d_uv && !d_point),
                  "nrf_ray_cast_mesh: any mode writes d_hit alone (null d_hit, or a d_t, d_face, d_uv or d_point that is not null)");
    NRF_RC_PREPARE("nrf_ray_cast_mesh", n_rays);
    if (n_rays == 0) return NRF_OK;
    NRF_RC_LAUNCH_PREMISE();
    const dim3 blocks((unsigned)ceil_div(n_rays, GEO_BLOCK));
    if (mode == NRF_RC_ANY)
        hipLaunchKernelGGL(k_rc_query<true>, blocks, dim3(GEO_BLOCK), 0, st, d_rays, n_rays, stride, m, g, clip, key, cull, (const long long *)grid.key, d_t, d_face, d_uv,
                           d_point, d_hit, ws.far.list, ws.far.n, (const uint32_t *)ws.outside, d_stats);
    else
        hipLaunchKernelGGL(k_rc_query<false>, blocks, dim3(GEO_BLOCK), 0, st, d_rays, n_rays, stride, m, g, clip, key, cull, (const long long *)grid.key, d_t, d_face, d_uv,
                           d_point, d_hit, ws.far.list, ws.far.n, (const uint32_t *)ws.outside, d_stats);
    NRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_rc_far, dim3(FAR_GRID), dim3(GEO_BLOCK), 0, st, d_rays, stride, m, key, cull, (const long long *)grid.key, d_t, d_face, d_uv, d_point, d_hit,
                       (const int32_t *)ws.far.list, (const uint32_t *)ws.far.n, d_stats);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

int nrf_hemisphere_dirs(const float *d_normals, int64_t n, int k, uint64_t seed, int64_t index0, float *d_dirs, uint32_t *d_stats, void *stream)
{
    NRF_CHECK_ARG(n >= 0 && n <= INT32_MAX, "nrf_hemisphere_dirs: %lld normals (0 .. 2^31 - 1)", (long long)n);
    NRF_CHECK_ARG(k >= 1 && k <= NRF_HEMI_MAX_K, "nrf_hemisphere_dirs: %d directions per normal (1 .. %d)", k, NRF_HEMI_MAX_K);
    NRF_CHECK_ARG(index0 >= 0 && index0 <= NRF_HEMI_MAX_INDEX - n, "nrf_hemisphere_dirs: index0 %lld with %lld normals leaves [0, 2^40]", (long long)index0, (long long)n);
    NRF_CHECK_ARG(n * k <= INT32_MAX, "nrf_hemisphere_dirs: %lld directions in one call (at most 2^31 - 1)", (long long)(n * k));
    NRF_CHECK_ARG(n == 0 || (d_normals && d_dirs), "nrf_hemisphere_dirs: null d_normals or d_dirs");
    if (n == 0) return NRF_OK;
    hipLaunchKernelGGL(k_rc_dirs, dim3((unsigned)ceil_div(n * k, GEO_BLOCK)), dim3(GEO_BLOCK), 0, as_stream(stream), d_normals, n, k, seed, index0, d_dirs, d_stats);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

int nrf_mesh_ambient_occlusion(const float *d_points, const float *d_normals, int64_t n, int k, float offset, float max_dist, uint64_t seed, int64_t index0,
                               const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, const float *bbox, int nx, int ny, int nz, int64_t n_refs,
                               int64_t n_large, const void *d_grid, size_t grid_bytes, float *d_ao, uint32_t *d_stats, void *d_workspace, size_t workspace_bytes,
                               void *stream)
{
    NRF_CHECK_ARG(n >= 0 && n <= INT32_MAX, "nrf_mesh_ambient_occlusion: %lld points (0 .. 2^31 - 1)", (long long)n);
    NRF_CHECK_ARG(k >= 1 && k <= NRF_HEMI_MAX_K, "nrf_mesh_ambient_occlusion: %d rays per point (1 .. %d)", k, NRF_HEMI_MAX_K);
    NRF_CHECK_ARG(index0 >= 0 && index0 <= NRF_HEMI_MAX_INDEX - n, "nrf_mesh_ambient_occlusion: index0 %lld with %lld points leaves [0, 2^40]", (long long)index0,
                  (long long)n);
    NRF_CHECK_ARG(std::isfinite(offset), "nrf_mesh_ambient_occlusion: offset must be finite (got %g)", (double)offset);
    NRF_CHECK_ARG(max_dist >= 0.0f, "nrf_mesh_ambient_occlusion: max_dist must be >= 0 or +inf (got %g)", (double)max_dist);          // NaN fails
    NRF_FG_CHECK_MESH("nrf_mesh_ambient_occlusion");
    NRF_CHECK_ARG(n == 0 || (d_points && d_normals && d_ao), "nrf_mesh_ambient_occlusion: null d_points, d_normals or d_ao");
    NRF_CHECK_ARG(n * k <= NRF_AO_MAX_RAYS, "nrf_mesh_ambient_occlusion: %lld rays in one call (at most 2^38; call it slab by slab with index0)", (long long)(n * k));
    NRF_RC_PREPARE("nrf_mesh_ambient_occlusion", n);
    if (n == 0) return NRF_OK;
    NRF_RC_LAUNCH_PREMISE();
    uint32_t *hits = reinterpret_cast<uint32_t *>(ws.far.list);          // the list of the ray-cast entry serves as the points' hit counters here
    NRF_HIP(hipMemsetAsync(hits, 0, (size_t)n * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_rc_ao, dim3((unsigned)ceil_div(n * k, GEO_BLOCK)), dim3(GEO_BLOCK), 0, st, d_points, d_normals, n, k, offset, max_dist, seed, index0, m, g, clip,
                       key, (const long long *)grid.key, (const uint32_t *)ws.outside, hits, d_stats);
    NRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_rc_ao_finish, dim3((unsigned)ceil_div(n, GEO_BLOCK)), dim3(GEO_BLOCK), 0, st, n, k, key, (const long long *)grid.key, (const uint32_t *)hits, d_ao);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

}  // extern "C"
