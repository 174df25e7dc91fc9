// face_grid.h -- what the tools that read a face grid share (geometry.hip: nrf_face_grid_* and nrf_closest_on_mesh; raycast.hip: nrf_ray_cast_mesh and
// nrf_mesh_ambient_occlusion): the uniform grid of nrf_nearest_points (NnGrid, nn_cell, nn_grid_make), the layout and the head of the caller-owned grid buffer
// (FgGrid, FgKey, fg_key_matches), the classes of a face (cm_face), the dot product in the header's order and the clamp of a surface point to its face's own
// coordinate box.  One copy of each: a query of either kind reads exactly the buffer the build wrote, and both proofs of completeness lean on the same clamp.
// Also the closest point of a triangle itself (nn_d2, CmHit, cm_closest): nrf_closest_on_mesh gathers it per query, voxel.hip (nrf_mesh_voxelize) scatters it per
// face over the lattice, and the two agree bit for bit because it is one function.  And the list of the queries a walk gives up (FarList, far_layout), and a face as a candidate of a query and the outputs of a
// query from its key (cm_take, cm_write): the grid's rings, its fallback and the BVH of bvh.hip go through them.
#pragma once

#include "common.h"
#include "reduce.h"
#include "workspace.h"

#include <climits>
#include <cmath>
#include <cstring>

namespace nrf {

constexpr int GEO_BLOCK = 256;
constexpr int FAR_GRID = 1024;           // workgroups of the brute-force kernels: 4 per CU

// the queries (rays) a walk gives up, for the brute-force kernel of its tool: scan.h's wave_append fills it
struct FarList {
    int32_t *list;           // [n] in any order
    uint32_t *n;             // [words] n[0] the length; the ray caster keeps its flag in a second word of the same 256-byte piece, so one memset clears both
};

inline FarList far_layout(Bump &b, int64_t n, int words = 1) { return FarList{b.take<int32_t>((size_t)n), b.take<uint32_t>((size_t)words)}; }

struct NnGrid {
    int n[3];
    int64_t cells;
    float bmin[3], inv_h[3];
    float h_min;             // the smallest cell edge, fl(1 / inv_h)
};

inline bool sample_shape_ok(int64_t n_verts, int64_t n_faces) { return n_verts >= 0 && n_verts <= INT32_MAX && n_faces >= 0 && n_faces <= INT32_MAX; }

inline bool nn_shape_ok(int64_t nq, int64_t nt, int nx, int ny, int nz)
{
    return nq >= 0 && nq <= INT32_MAX && nt >= 0 && nt <= INT32_MAX && nx >= 1 && nx <= NRF_NN_MAX_DIM && ny >= 1 && ny <= NRF_NN_MAX_DIM && nz >= 1 &&
           nz <= NRF_NN_MAX_DIM && (int64_t)nx * ny * nz <= NRF_NN_MAX_CELLS;
}

__device__ __forceinline__ bool finite3(const float p[3]) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

// the header's cell coordinate: clamp((int)floorf((x - bmin) * inv_h), 0, n - 1), clamped as a float so that the conversion is defined for every finite x
__device__ __forceinline__ int nn_cell(float x, float bmin, float inv_h, int n)
{
    const float t = floorf((x - bmin) * inv_h);
    return (int)fminf(fmaxf(t, 0.0f), (float)(n - 1));
}

// the grid of a box and dims, as nrf_nearest_points states it; false with the offending axis where the box is refused
inline bool nn_grid_make(const float *bbox, int nx, int ny, int nz, NnGrid &g, int &axis)
{
    g.n[0] = nx; g.n[1] = ny; g.n[2] = nz;
    g.cells = (int64_t)nx * ny * nz;
    g.h_min = INFINITY;
    for (int a = 0; a < 3; a++) {
        const float extent = bbox[3 + a] - bbox[a];
        const float inv_h = (float)g.n[a] / extent;
        const float h = 1.0f / inv_h;
        if (!(std::isfinite(bbox[a]) && std::isfinite(bbox[3 + a]) && extent > 0.0f && std::isfinite(extent) && std::isfinite(inv_h) && inv_h > 0.0f && std::isfinite(h) &&
              h > 0.0f)) {
            axis = a;
            return false;
        }
        g.bmin[a] = bbox[a];
        g.inv_h[a] = inv_h;
        g.h_min = h < g.h_min ? h : g.h_min;
    }
    return true;
}

// ---------------------------------------------------------------------------------------------- the face grid
constexpr long long FG_MAGIC = 0x4e52464647524431ll;          // "NRFFGRD1": the first word of a built grid buffer

// what a grid buffer was built for, as the header states it: the query kernels compare it with their own arguments before they read anything else of the buffer
struct FgKey {
    long long w[8];          // magic, F, dims packed, n_refs, n_large, the bits of the box two floats to a word
};

struct FgGrid {              // the caller-owned buffer the queries read
    long long *key;          // [8]
    uint32_t *start;         // [cells + 1] the references of cell c are refs[start[c] .. start[c + 1])
    int32_t *refs;           // [n_refs] face indices in cell order
    int32_t *large;          // [n_large] the faces every query tests
};

inline FgGrid fg_grid_layout(Bump &b, int64_t cells, int64_t n_refs, int64_t n_large)
{
    FgGrid s;
    s.key = b.take<long long>(8);
    s.start = b.take<uint32_t>((size_t)cells + 1);
    s.refs = b.take<int32_t>((size_t)n_refs);
    s.large = b.take<int32_t>((size_t)n_large);
    return s;
}

inline bool fg_shape_ok(int64_t n_verts, int64_t n_faces, int nx, int ny, int nz) { return sample_shape_ok(n_verts, n_faces) && nn_shape_ok(0, 0, nx, ny, nz); }

inline bool fg_counts_ok(int64_t n_faces, int64_t n_refs, int64_t n_large) { return n_refs >= 0 && n_refs < ((int64_t)1 << 32) && n_large >= 0 && n_large <= n_faces; }

inline FgKey fg_key(int64_t n_faces, int nx, int ny, int nz, int64_t n_refs, int64_t n_large, const float *bbox)
{
    FgKey k;
    uint32_t bits[6];
    std::memcpy(bits, bbox, sizeof(bits));
    k.w[0] = FG_MAGIC;
    k.w[1] = n_faces;
    k.w[2] = ((long long)nz << 40) | ((long long)ny << 20) | nx;
    k.w[3] = n_refs;
    k.w[4] = n_large;
    for (int a = 0; a < 3; a++) k.w[5 + a] = (long long)(((unsigned long long)bits[3 + a] << 32) | bits[a]);
    return k;
}

__device__ __forceinline__ bool fg_key_matches(const long long *__restrict__ grid_key, const FgKey &key)
{
    bool same = true;
#pragma unroll
    for (int k = 0; k < 8; k++) same = same && grid_key[k] == key.w[k];
    return same;
}

// the corners of face f -> 0: a face; 1: a corner outside [0, V) (nothing dereferenced) or f outside [0, F); 2: a non-finite coordinate
__device__ __forceinline__ int cm_face(const float *__restrict__ verts, int32_t n_verts, const int32_t *__restrict__ faces, int64_t n_faces, int64_t f, float a[3], float b[3],
                                       float c[3])
{
    if (f < 0 || f >= n_faces) return 1;
    const int32_t i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    if (i0 < 0 || i0 >= n_verts || i1 < 0 || i1 >= n_verts || i2 < 0 || i2 >= n_verts) return 1;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        a[k] = verts[(int64_t)i0 * 3 + k];
        b[k] = verts[(int64_t)i1 * 3 + k];
        c[k] = verts[(int64_t)i2 * 3 + k];
    }
    return finite3(a) && finite3(b) && finite3(c) ? 0 : 2;
}

__device__ __forceinline__ float cm_dot(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// a surface point stays inside its face's coordinate box (the proofs of both queries need it): out = p < lo ? lo : (p > hi ? hi : p) per component, lo / hi the
// smallest / largest of the three corners; the comparisons keep a NaN a NaN
__device__ __forceinline__ void cm_clamp_to_face(const float p[3], const float a[3], const float b[3], const float c[3], float out[3])
{
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float lo = fminf(fminf(a[k], b[k]), c[k]), hi = fmaxf(fmaxf(a[k], b[k]), c[k]);
        out[k] = p[k] < lo ? lo : (p[k] > hi ? hi : p[k]);
    }
}

// the one place d2 is formed
__device__ __forceinline__ float nn_d2(float qx, float qy, float qz, const float4 &t)
{
    const float dx = qx - t.x, dy = qy - t.y, dz = qz - t.z;
    return (dx * dx + dy * dy) + dz * dz;
}

struct CmHit {
    float d2, v, w, p[3];
};

// the one place the closest point of a triangle is formed (the header's steps, Ericson 5.1.5): region, (v, w), P, the clamp to the face's own box, d2
__device__ __forceinline__ void cm_closest(const float q[3], const float a[3], const float b[3], const float c[3], CmHit &h)
{
    float ab[3], ac[3], ap[3], bp[3], cp[3], p[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        ab[k] = b[k] - a[k];
        ac[k] = c[k] - a[k];
        ap[k] = q[k] - a[k];
        bp[k] = q[k] - b[k];
        cp[k] = q[k] - c[k];
    }
    const float d1 = cm_dot(ab, ap), d2 = cm_dot(ac, ap), d3 = cm_dot(ab, bp), d4 = cm_dot(ac, bp), d5 = cm_dot(ab, cp), d6 = cm_dot(ac, cp);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    float v, w;
    if (d1 <= 0.0f && d2 <= 0.0f) {                                                  // A
        v = 0.0f; w = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; k++) p[k] = a[k];
    } else if (d3 >= 0.0f && d4 <= d3) {                                             // B
        v = 1.0f; w = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; k++) p[k] = b[k];
    } else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {                             // edge AB
        v = d1 / (d1 - d3); w = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; k++) p[k] = a[k] + v * ab[k];
    } else if (d6 >= 0.0f && d5 <= d6) {                                             // C
        v = 0.0f; w = 1.0f;
#pragma unroll
        for (int k = 0; k < 3; k++) p[k] = c[k];
    } else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {                             // edge AC
        v = 0.0f; w = d2 / (d2 - d6);
#pragma unroll
        for (int k = 0; k < 3; k++) p[k] = a[k] + w * ac[k];
    } else if (va <= 0.0f && (d4 - d3) >= 0.0f && (d5 - d6) >= 0.0f) {               // edge BC
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6)); v = 1.0f - w;
#pragma unroll
        for (int k = 0; k < 3; k++) p[k] = b[k] + w * (c[k] - b[k]);
    } else {                                                                         // interior
        const float denom = 1.0f / ((va + vb) + vc);
        v = vb * denom; w = vc * denom;
#pragma unroll
        for (int k = 0; k < 3; k++) p[k] = (a[k] + ab[k] * v) + ac[k] * w;
    }
    cm_clamp_to_face(p, a, b, c, h.p);          // P stays inside the face's coordinate box (the stop rule's proof needs it); the comparisons keep a NaN a NaN
    h.v = v;
    h.w = w;
    h.d2 = nn_d2(q[0], q[1], q[2], make_float4(h.p[0], h.p[1], h.p[2], 0.0f));
}

// face f as a candidate of query q: rings, large list and fallback all come through here
__device__ __forceinline__ void cm_take(const float q[3], const float *__restrict__ verts, int32_t n_verts, const int32_t *__restrict__ faces, int64_t n_faces, int64_t f,
                                        float md2, unsigned long long &best)
{
    float a[3], b[3], c[3];
    if (cm_face(verts, n_verts, faces, n_faces, f, a, b, c) != 0) return;
    CmHit h;
    cm_closest(q, a, b, c, h);
    const unsigned long long k = key_pack(h.d2, (uint32_t)f);
    if (h.d2 <= md2 && k < best) best = k;          // a NaN d2 fails the comparison
}

// the outputs of query qi from its key: (v, w) and P are those of the winning face, formed once more by the same function
__device__ __forceinline__ void cm_write(const float q[3], int64_t qi, unsigned long long best, const float *__restrict__ verts, int32_t n_verts,
                                         const int32_t *__restrict__ faces, int64_t n_faces, float *__restrict__ dist2, int32_t *__restrict__ face, float *__restrict__ uv,
                                         float *__restrict__ point)
{
    const int32_t f = key_index(best);
    dist2[qi] = key_value(best);
    face[qi] = f;
    if (!uv && !point) return;
    CmHit h;
    h.v = h.w = h.p[0] = h.p[1] = h.p[2] = 0.0f;
    float a[3], b[3], c[3];
    if (f >= 0 && cm_face(verts, n_verts, faces, n_faces, f, a, b, c) == 0) cm_closest(q, a, b, c, h);
    if (uv) { uv[qi * 2 + 0] = h.v; uv[qi * 2 + 1] = h.w; }
    if (point) { point[qi * 3 + 0] = h.p[0]; point[qi * 3 + 1] = h.p[1]; point[qi * 3 + 2] = h.p[2]; }
}

// the argument checks the entries over a face grid share: shapes, pointers of the mesh, the box
#define NRF_FG_CHECK_MESH(who)                                                                                                                                            \
    NRF_CHECK_ARG(fg_shape_ok(n_verts, n_faces, nx, ny, nz), who ": %lld vertices, %lld faces (both 0 .. 2^31 - 1), grid %d x %d x %d (each 1 .. %d, product <= %d)",    \
                  (long long)n_verts, (long long)n_faces, nx, ny, nz, NRF_NN_MAX_DIM, NRF_NN_MAX_CELLS);                                                                   \
    NRF_CHECK_ARG(n_faces == 0 || d_faces, who ": null d_faces");                                                                                                         \
    NRF_CHECK_ARG(d_verts || n_verts == 0 || n_faces == 0, who ": null d_verts");                                                                                         \
    NRF_CHECK_ARG(bbox, who ": null bbox");                                                                                                                               \
    NnGrid g;                                                                                                                                                             \
    int axis = 0;                                                                                                                                                         \
    NRF_CHECK_ARG(nn_grid_make(bbox, nx, ny, nz, g, axis), who ": empty, inverted or non-finite box on axis %d ([%g, %g])", axis, (double)bbox[axis], (double)bbox[3 + axis])

// the checks of the grid buffer and the counts that every query over a built grid makes
#define NRF_FG_CHECK_GRID(who)                                                                                                                                            \
    NRF_CHECK_ARG(fg_counts_ok(n_faces, n_refs, n_large), who ": %lld references (0 .. 2^32 - 1), %lld large faces (0 .. %lld): not the count call's",                   \
                  (long long)n_refs, (long long)n_large, (long long)n_faces);                                                                                              \
    NRF_CHECK_ARG(d_grid && (reinterpret_cast<uintptr_t>(d_grid) & 7) == 0, who ": the grid buffer must be non-null and 8-byte aligned");                                 \
    NRF_CHECK_ARG(grid_bytes == nrf_face_grid_bytes(n_faces, nx, ny, nz, n_refs, n_large),                                                                                \
                  who ": a grid buffer of %zu bytes was not built for these faces, dims and counts (nrf_face_grid_bytes gives %zu)", grid_bytes,                          \
                  nrf_face_grid_bytes(n_faces, nx, ny, nz, n_refs, n_large))

}  // namespace nrf
