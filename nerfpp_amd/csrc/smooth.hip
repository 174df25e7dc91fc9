// smooth.hip -- the inverted index of a triangle list (nrf_mesh_adjacency_count / _emit) and the two gathers that read it: the Taubin / Laplacian filter
// (nrf_mesh_smooth) and face-derived vertex normals (nrf_mesh_vertex_normals).  The reference has no mesh code; the contract is stated in include/nerfpp_hip.h and
// restated in numpy by tests/smooth_ref.py, which the GPU tests compare with bit for bit.
//
// Count call.
//   k_adj_classify   one lane per face: BAD / REPEATED / valid; a valid face adds 1 to the degree of its three corners (integer atomics); the block's two skip counts
//   k_block_sums / k_totals_scan (scan.h) / k_adj_starts   exclusive scan of the degrees -> the row starts [V+1] (int64); run twice, for the face rows and the neighbour rows
//   k_adj_fill       one lane per valid face: each corner takes the next free place of its row (an integer cursor): the row holds the right faces in ARRIVAL order
//   k_adj_rows<1>    one lane per vertex with a row of at most NRF_ADJ_SHORT_ROW faces; a longer row is appended to a list (its order does not matter) for
//   k_adj_rows<256>  one workgroup per listed row.  Both run the same four steps over one row:
//                      1. rank sort of the row's faces (distinct integers: the rank of a face is the number of smaller ones) -> ascending face index;
//                      2. per face of the sorted row the two corners that are not the vertex, in the face's winding -> 2 * len half-edge ends;
//                      3. rank sort of those (ties by position) -> ascending neighbour, a neighbour once per face on the edge;
//                      4. the number of distinct values = the length of the neighbour row.
// Emit call.  Copies the starts and the face rows out; k_adj_emit, one lane per vertex, walks the sorted half-edge ends: each run is one neighbour, its length the
// number of faces on the edge; flags and the statistics (integer sums and maxima) follow.
// Only integers decide anything here, and nothing that reaches an output depends on which lane won a cursor.  No kernel waits on another workgroup.
//
// nrf_mesh_smooth: one launch per step, one lane per vertex, a gather over the neighbour row in its stored order; d_tmp and d_out alternate so that the last step
// writes d_out.  nrf_mesh_vertex_normals: one lane per vertex over its face row.  No atomics in either.
#include "common.h"
#include "scan.h"
#include "workspace.h"

#include <climits>
#include <cmath>

namespace nrf {

namespace {

constexpr int ADJ_BLOCK = 256;
constexpr int ADJ_LONG_GRID = 1024;          // workgroups that share the long rows

struct AdjWs {
    unsigned long long *header;          // [0] long rows, [1] faces with a bad index, [2] faces with a repeated corner
    int32_t *deg;                        // [V] valid faces per vertex
    int32_t *cursor;                     // [V] places of the row taken so far
    int32_t *ndeg;                       // [V] distinct neighbours
    int32_t *longv;                      // [V] the vertices whose row is longer than NRF_ADJ_SHORT_ROW
    int64_t *fstart, *nstart;            // [V+1] row starts; [V] = the totals the count call returns
    int64_t *bsum;                       // [vertex blocks]
    int32_t *raw;                        // [3F] face rows in arrival order
    int32_t *flist;                      // [3F] face rows, ascending
    int32_t *he_raw;                     // [6F] half-edge ends in face order
    int32_t *he_sorted;                  // [6F] ascending, with repeats
};

AdjWs adj_layout(Bump &b, int64_t n_verts, int64_t n_faces)
{
    AdjWs w;
    w.header = b.take<unsigned long long>(4);
    w.deg = b.take<int32_t>((size_t)n_verts);
    w.cursor = b.take<int32_t>((size_t)n_verts);
    w.ndeg = b.take<int32_t>((size_t)n_verts);
    w.longv = b.take<int32_t>((size_t)n_verts);
    w.fstart = b.take<int64_t>((size_t)n_verts + 1);
    w.nstart = b.take<int64_t>((size_t)n_verts + 1);
    w.bsum = b.take<int64_t>((size_t)ceil_div(n_verts > 0 ? n_verts : 1, ADJ_BLOCK));
    w.raw = b.take<int32_t>((size_t)n_faces * 3);
    w.flist = b.take<int32_t>((size_t)n_faces * 3);
    w.he_raw = b.take<int32_t>((size_t)n_faces * 6);
    w.he_sorted = b.take<int32_t>((size_t)n_faces * 6);
    return w;
}

bool adj_shape_ok(int64_t n_verts, int64_t n_faces) { return n_verts >= 0 && n_verts <= INT32_MAX && n_faces >= 0 && n_faces <= INT32_MAX; }

// 0: valid, 1: a corner outside [0, V), 2: two equal corners
__device__ __forceinline__ int adj_face_class(int32_t a, int32_t b, int32_t c, int32_t n_verts)
{
    if (a < 0 || a >= n_verts || b < 0 || b >= n_verts || c < 0 || c >= n_verts) return 1;
    return (a == b || b == c || a == c) ? 2 : 0;
}

// the block's sum of v, added to *dst by one integer atomic (nothing where it is 0)
__device__ __forceinline__ void block_add(unsigned long long v, unsigned long long *dst, unsigned long long *sh)
{
    if (threadIdx.x == 0) *sh = 0;
    __syncthreads();
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(sh, v);
    __syncthreads();
    if (threadIdx.x == 0 && *sh) atomicAdd(dst, *sh);
    __syncthreads();
}

__device__ __forceinline__ void block_max(unsigned long long v, unsigned long long *dst, unsigned long long *sh)
{
    if (threadIdx.x == 0) *sh = 0;
    __syncthreads();
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long t = __shfl_xor(v, off, 64);
        v = t > v ? t : v;
    }
    if ((threadIdx.x & 63) == 0 && v) atomicMax(sh, v);
    __syncthreads();
    if (threadIdx.x == 0 && *sh) atomicMax(dst, *sh);
    __syncthreads();
}

__global__ void __launch_bounds__(ADJ_BLOCK) k_adj_classify(const int32_t *__restrict__ faces, int64_t n_faces, int32_t n_verts, int32_t *deg, unsigned long long *header)
{
    __shared__ unsigned long long sh;
    const int64_t f = (int64_t)blockIdx.x * ADJ_BLOCK + threadIdx.x;
    int cls = -1;
    if (f < n_faces) {
        const int32_t a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
        cls = adj_face_class(a, b, c, n_verts);
        if (cls == 0) {
            atomicAdd(deg + a, 1);
            atomicAdd(deg + b, 1);
            atomicAdd(deg + c, 1);
        }
    }
    block_add(cls == 1 ? 1ull : 0ull, header + 1, &sh);
    block_add(cls == 2 ? 1ull : 0ull, header + 2, &sh);
}

__global__ void __launch_bounds__(ADJ_BLOCK) k_adj_starts(const int32_t *__restrict__ deg, int64_t n_verts, const int64_t *__restrict__ bsum, int64_t *__restrict__ start)
{
    __shared__ int64_t sh[ADJ_BLOCK];
    const int64_t v = (int64_t)blockIdx.x * ADJ_BLOCK + threadIdx.x;
    int64_t total;
    const int64_t before = block_exclusive_scan<int64_t, ADJ_BLOCK>(v < n_verts ? (int64_t)deg[v] : 0, sh, total);
    if (v < n_verts) start[v] = bsum[blockIdx.x] + before;          // start[V] is k_totals_scan's total
}

__global__ void __launch_bounds__(ADJ_BLOCK) k_adj_fill(const int32_t *__restrict__ faces, int64_t n_faces, int32_t n_verts, const int64_t *__restrict__ fstart,
                                                        int32_t *cursor, int32_t *__restrict__ raw)
{
    const int64_t f = (int64_t)blockIdx.x * ADJ_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    const int32_t c[3] = {faces[f * 3 + 0], faces[f * 3 + 1], faces[f * 3 + 2]};
    if (adj_face_class(c[0], c[1], c[2], n_verts) != 0) return;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int64_t at = fstart[c[k]] + atomicAdd(cursor + c[k], 1);          // < fstart[c + 1]: the degrees counted these same faces
        if (at < n_faces * 3) raw[at] = (int32_t)f;
    }
}

// the four steps of one row, by LANES lanes (1: a lane of any workgroup; ADJ_BLOCK: the whole workgroup, every thread of it arrives here)
template <int LANES>
__device__ __forceinline__ void adj_row(const int32_t *__restrict__ faces, int32_t v, int64_t s, int64_t n, const int32_t *__restrict__ raw, int32_t *flist,
                                        int32_t *he_raw, int32_t *he_sorted, int32_t *__restrict__ ndeg, int *sh)
{
    const int t = LANES == 1 ? 0 : (int)threadIdx.x;
    for (int64_t k = t; k < n; k += LANES) {
        const int32_t e = raw[s + k];
        int64_t r = 0;
        for (int64_t j = 0; j < n; j++) r += raw[s + j] < e ? 1 : 0;
        flist[s + r] = e;
    }
    if (LANES > 1) __syncthreads();
    for (int64_t k = t; k < n; k += LANES) {
        const int64_t f = flist[s + k];
        const int32_t a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
        he_raw[2 * (s + k) + 0] = a == v ? b : (b == v ? c : a);
        he_raw[2 * (s + k) + 1] = a == v ? c : (b == v ? a : b);
    }
    if (LANES > 1) __syncthreads();
    for (int64_t k = t; k < 2 * n; k += LANES) {
        const int32_t e = he_raw[2 * s + k];
        int64_t r = 0;
        for (int64_t j = 0; j < 2 * n; j++) {
            const int32_t o = he_raw[2 * s + j];
            r += (o < e || (o == e && j < k)) ? 1 : 0;
        }
        he_sorted[2 * s + r] = e;
    }
    if (LANES > 1) __syncthreads();
    int distinct = 0;
    for (int64_t k = t; k < 2 * n; k += LANES) distinct += (k == 0 || he_sorted[2 * s + k - 1] != he_sorted[2 * s + k]) ? 1 : 0;
    if (LANES > 1) {
        if (threadIdx.x == 0) *sh = 0;
        __syncthreads();
        if (distinct) atomicAdd(sh, distinct);
        __syncthreads();
        distinct = *sh;
        __syncthreads();
    }
    if (t == 0) ndeg[v] = distinct;
}

template <int LANES>
__global__ void __launch_bounds__(ADJ_BLOCK) k_adj_rows(const int32_t *__restrict__ faces, int64_t n_verts, const int64_t *__restrict__ fstart,
                                                        const int32_t *__restrict__ raw, int32_t *flist, int32_t *he_raw, int32_t *he_sorted, int32_t *__restrict__ ndeg,
                                                        int32_t *longv, unsigned long long *header)
{
    __shared__ int sh;
    if (LANES == 1) {
        const int64_t v = (int64_t)blockIdx.x * ADJ_BLOCK + threadIdx.x;
        if (v >= n_verts) return;
        const int64_t s = fstart[v], n = fstart[v + 1] - s;
        if (n > NRF_ADJ_SHORT_ROW) {
            longv[atomicAdd(header, 1ull)] = (int32_t)v;          // at most V entries
            return;
        }
        adj_row<1>(faces, (int32_t)v, s, n, raw, flist, he_raw, he_sorted, ndeg, &sh);
    } else {
        const int64_t rows = (int64_t)*header;          // complete: the launch before has ended
        for (int64_t i = blockIdx.x; i < rows; i += gridDim.x) {
            const int32_t v = longv[i];
            const int64_t s = fstart[v];
            adj_row<ADJ_BLOCK>(faces, v, s, fstart[v + 1] - s, raw, flist, he_raw, he_sorted, ndeg, &sh);
        }
    }
}

__global__ void __launch_bounds__(ADJ_BLOCK) k_adj_emit(int64_t n_verts, const int64_t *__restrict__ fstart, int64_t n_incident, const int32_t *__restrict__ he_sorted,
                                                        const int64_t *__restrict__ nstart, int64_t n_neighbours, int32_t *__restrict__ nbr,
                                                        int32_t *__restrict__ nbr_faces, uint8_t *__restrict__ flags, unsigned long long *stats)
{
    __shared__ unsigned long long sh;
    const int64_t v = (int64_t)blockIdx.x * ADJ_BLOCK + threadIdx.x;
    unsigned long long used = 0, boundary = 0, nonmanifold = 0, frow = 0, nrow = 0;
    if (v < n_verts) {
        // rows of the count call's workspace; clamped so that nothing outside it is read and nothing beyond the caller's totals is written
        const int64_t fb = min(max(fstart[v], (int64_t)0), n_incident), fe = min(max(fstart[v + 1], fb), n_incident);
        const int64_t first = nstart[v];
        int64_t at = first;
        unsigned flag = 0;
        for (int64_t k = 2 * fb; k < 2 * fe;) {
            const int32_t w = he_sorted[k];
            int32_t count = 1;
            while (k + count < 2 * fe && he_sorted[k + count] == w) count++;
            if (at >= 0 && at < n_neighbours) {
                nbr[at] = w;
                nbr_faces[at] = count;
            }
            at++;
            k += count;
            if (count == 1) flag |= NRF_ADJ_BOUNDARY;
            if (count > 2) flag |= NRF_ADJ_NONMANIFOLD;
            if ((int64_t)w > v) {          // every edge once, at its lower end
                boundary += count == 1 ? 1 : 0;
                nonmanifold += count > 2 ? 1 : 0;
            }
        }
        flags[v] = (uint8_t)flag;
        used = fe > fb ? 1 : 0;
        frow = (unsigned long long)(fe - fb);
        nrow = (unsigned long long)(at - first);
        if (v == 0) stats[3] = (unsigned long long)n_neighbours / 2;          // every edge stands in the rows of both its ends
    }
    block_add(used, stats + 2, &sh);
    block_add(boundary, stats + 4, &sh);
    block_add(nonmanifold, stats + 5, &sh);
    block_max(frow, stats + 6, &sh);
    block_max(nrow, stats + 7, &sh);
}

int adj_check(const char *who, const int32_t *d_faces, int64_t n_verts, int64_t n_faces, const void *d_workspace)
{
    if (!adj_shape_ok(n_verts, n_faces)) {
        set_error("%s: %lld vertices, %lld faces (0 .. 2^31 - 1)", who, (long long)n_verts, (long long)n_faces);
        return NRF_ERR_INVALID_ARG;
    }
    if (n_faces > 0 && !d_faces) {
        set_error("%s: null d_faces", who);
        return NRF_ERR_INVALID_ARG;
    }
    if (!d_workspace || (reinterpret_cast<uintptr_t>(d_workspace) & 7) != 0) {
        set_error("%s: the workspace must be non-null and 8-byte aligned", who);
        return NRF_ERR_INVALID_ARG;
    }
    return NRF_OK;
}

// start[0 .. V] = the exclusive scan of deg[0 .. V)
int adj_scan(const int32_t *deg, int64_t n_verts, int64_t *bsum, int64_t *start, hipStream_t st)
{
    const int64_t vb = ceil_div(n_verts, ADJ_BLOCK);
    if (n_verts > 0) {
        hipLaunchKernelGGL((k_block_sums<int32_t, ADJ_BLOCK>), dim3((unsigned)vb), dim3(ADJ_BLOCK), 0, st, n_verts, deg, bsum);
        NRF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL((k_totals_scan<int64_t, int64_t>), dim3(1), dim3(SCAN_BLOCK), 0, st, vb, bsum, start + n_verts);
    NRF_LAUNCH_CHECK();
    if (n_verts > 0) {
        hipLaunchKernelGGL(k_adj_starts, dim3((unsigned)vb), dim3(ADJ_BLOCK), 0, st, deg, n_verts, (const int64_t *)bsum, start);
        NRF_LAUNCH_CHECK();
    }
    return NRF_OK;
}

// ---- the gathers ----

template <int C> struct Vec { float c[C]; };

template <int C> __device__ __forceinline__ Vec<C> load_vec(const float *__restrict__ p, int64_t i)
{
    Vec<C> r;
    if constexpr (C == 2) {
        const float2 t = reinterpret_cast<const float2 *>(p)[i];
        r.c[0] = t.x; r.c[1] = t.y;
    } else if constexpr (C == 4) {
        const float4 t = reinterpret_cast<const float4 *>(p)[i];
        r.c[0] = t.x; r.c[1] = t.y; r.c[2] = t.z; r.c[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < C; k++) r.c[k] = p[i * C + k];          // C == 3: adjacent dwords, one 12-byte load
    }
    return r;
}

template <int C> __device__ __forceinline__ void store_vec(float *__restrict__ p, int64_t i, const Vec<C> &r)
{
    if constexpr (C == 2) {
        reinterpret_cast<float2 *>(p)[i] = make_float2(r.c[0], r.c[1]);
    } else if constexpr (C == 4) {
        reinterpret_cast<float4 *>(p)[i] = make_float4(r.c[0], r.c[1], r.c[2], r.c[3]);
    } else {
#pragma unroll
        for (int k = 0; k < C; k++) p[i * C + k] = r.c[k];
    }
}

// one step: out = x + f * (mean of the neighbour set - x), one lane per vertex
template <int C>
__global__ void __launch_bounds__(ADJ_BLOCK) k_smooth_step(const float *__restrict__ x, float *__restrict__ out, int64_t n_verts, float f, int boundary,
                                                           const int64_t *__restrict__ nbr_start, const int32_t *__restrict__ nbr, const int32_t *__restrict__ nbr_faces,
                                                           const uint8_t *__restrict__ flags, int64_t n_neighbours)
{
    const int64_t i = (int64_t)blockIdx.x * ADJ_BLOCK + threadIdx.x;
    if (i >= n_verts) return;
    const Vec<C> xi = load_vec<C>(x, i);
    const bool on_boundary = boundary != NRF_SMOOTH_FREE && (flags[i] & NRF_ADJ_BOUNDARY) != 0;
    Vec<C> r = xi;
    if (!(on_boundary && boundary == NRF_SMOOTH_FIXED)) {
        const bool curve = on_boundary;          // NRF_SMOOTH_CURVE: only the neighbours across a boundary edge
        const int64_t b = min(max(nbr_start[i], (int64_t)0), n_neighbours), e = min(max(nbr_start[i + 1], b), n_neighbours);
        Vec<C> s = xi;          // replaced by the first neighbour
        int count = 0;
        for (int64_t k = b; k < e; k++) {
            const int32_t j = nbr[k];
            if ((uint32_t)j >= (uint32_t)n_verts) continue;          // never dereferenced; the rows of nrf_mesh_adjacency_emit hold no such index
            if (curve && nbr_faces[k] != 1) continue;
            const Vec<C> xj = load_vec<C>(x, j);
#pragma unroll
            for (int c = 0; c < C; c++) s.c[c] = count == 0 ? xj.c[c] : s.c[c] + xj.c[c];
            count++;
        }
        if (count > 0) {
            const float n = (float)count;
#pragma unroll
            for (int c = 0; c < C; c++) {
                const float m = s.c[c] / n;
                const float d = m - xi.c[c];
                const float p = f * d;
                r.c[c] = xi.c[c] + p;
            }
        }
    }
    store_vec<C>(out, i, r);
}

template <int C>
void smooth_launch(const float *x, float *out, int64_t n_verts, float f, int boundary, const int64_t *nbr_start, const int32_t *nbr, const int32_t *nbr_faces,
                   const uint8_t *flags, int64_t n_neighbours, hipStream_t st)
{
    hipLaunchKernelGGL(k_smooth_step<C>, dim3((unsigned)ceil_div(n_verts, ADJ_BLOCK)), dim3(ADJ_BLOCK), 0, st, x, out, n_verts, f, boundary, nbr_start, nbr, nbr_faces, flags,
                       n_neighbours);
}

__global__ void __launch_bounds__(ADJ_BLOCK) k_vertex_normals(const float *__restrict__ verts, int64_t n_verts, const int32_t *__restrict__ faces, int64_t n_faces,
                                                              const int64_t *__restrict__ face_start, const int32_t *__restrict__ face_list, int64_t n_incident,
                                                              int weighting, float *__restrict__ out)
{
    const int64_t v = (int64_t)blockIdx.x * ADJ_BLOCK + threadIdx.x;
    if (v >= n_verts) return;
    const int64_t b = min(max(face_start[v], (int64_t)0), n_incident), e = min(max(face_start[v + 1], b), n_incident);
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    bool first = true;
    for (int64_t k = b; k < e; k++) {
        const int32_t f = face_list[k];
        if ((uint32_t)f >= (uint32_t)n_faces) continue;          // never dereferenced; the rows of nrf_mesh_adjacency_emit hold no such index
        const int32_t ia = faces[(int64_t)f * 3 + 0], ib = faces[(int64_t)f * 3 + 1], ic = faces[(int64_t)f * 3 + 2];
        if ((uint32_t)ia >= (uint32_t)n_verts || (uint32_t)ib >= (uint32_t)n_verts || (uint32_t)ic >= (uint32_t)n_verts) continue;
        const Vec<3> pa = load_vec<3>(verts, ia), pb = load_vec<3>(verts, ib), pc = load_vec<3>(verts, ic);
        const float e1x = pb.c[0] - pa.c[0], e1y = pb.c[1] - pa.c[1], e1z = pb.c[2] - pa.c[2];
        const float e2x = pc.c[0] - pa.c[0], e2y = pc.c[1] - pa.c[1], e2z = pc.c[2] - pa.c[2];
        float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
        if (weighting == NRF_NORMALS_UNIT) {
            const float l = sqrtf((nx * nx + ny * ny) + nz * nz);
            if (l == 0.0f) {
                nx = 0.0f; ny = 0.0f; nz = 0.0f;
            } else {
                nx = nx / l; ny = ny / l; nz = nz / l;
            }
        }
        sx = first ? nx : sx + nx;
        sy = first ? ny : sy + ny;
        sz = first ? nz : sz + nz;
        first = false;
    }
    const float len = sqrtf((sx * sx + sy * sy) + sz * sz);
    Vec<3> r;
    r.c[0] = len == 0.0f ? 0.0f : sx / len;
    r.c[1] = len == 0.0f ? 0.0f : sy / len;
    r.c[2] = len == 0.0f ? 0.0f : sz / len;
    store_vec<3>(out, v, r);
}

}  // namespace

}  // namespace nrf

using namespace nrf;

extern "C" {

size_t nrf_mesh_adjacency_workspace_bytes(int64_t n_verts, int64_t n_faces)
{
    if (!adj_shape_ok(n_verts, n_faces)) return 0;
    return measure([&](Bump &b) { adj_layout(b, n_verts, n_faces); });
}

int nrf_mesh_adjacency_count(const int32_t *d_faces, int64_t n_verts, int64_t n_faces, int64_t *n_incident, int64_t *n_neighbours, void *d_workspace,
                             size_t workspace_bytes, void *stream)
{
    NRF_TRY(adj_check("nrf_mesh_adjacency_count", d_faces, n_verts, n_faces, d_workspace));
    NRF_CHECK_ARG(n_incident && n_neighbours, "nrf_mesh_adjacency_count: null n_incident or n_neighbours");
    Bump bump(d_workspace, workspace_bytes);
    const AdjWs w = adj_layout(bump, n_verts, n_faces);
    NRF_TRY(ws_check(bump, nrf_mesh_adjacency_workspace_bytes(n_verts, n_faces), "nrf_mesh_adjacency_count"));
    hipStream_t st = as_stream(stream);
    const dim3 block(ADJ_BLOCK);
    const unsigned fb = (unsigned)ceil_div(n_faces, ADJ_BLOCK), vb = (unsigned)ceil_div(n_verts, ADJ_BLOCK);
    NRF_HIP(hipMemsetAsync(w.header, 0, 4 * sizeof(unsigned long long), st));
    if (n_verts > 0) {
        NRF_HIP(hipMemsetAsync(w.deg, 0, (size_t)n_verts * sizeof(int32_t), st));
        NRF_HIP(hipMemsetAsync(w.cursor, 0, (size_t)n_verts * sizeof(int32_t), st));
        NRF_HIP(hipMemsetAsync(w.ndeg, 0, (size_t)n_verts * sizeof(int32_t), st));
    }
    if (n_faces > 0) {
        hipLaunchKernelGGL(k_adj_classify, dim3(fb), block, 0, st, d_faces, n_faces, (int32_t)n_verts, w.deg, w.header);
        NRF_LAUNCH_CHECK();
    }
    NRF_TRY(adj_scan(w.deg, n_verts, w.bsum, w.fstart, st));
    if (n_faces > 0 && n_verts > 0) {
        hipLaunchKernelGGL(k_adj_fill, dim3(fb), block, 0, st, d_faces, n_faces, (int32_t)n_verts, (const int64_t *)w.fstart, w.cursor, w.raw);
        NRF_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_adj_rows<1>, dim3(vb), block, 0, st, d_faces, n_verts, (const int64_t *)w.fstart, (const int32_t *)w.raw, w.flist, w.he_raw, w.he_sorted, w.ndeg,
                           w.longv, w.header);
        NRF_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_adj_rows<ADJ_BLOCK>, dim3(ADJ_LONG_GRID), block, 0, st, d_faces, n_verts, (const int64_t *)w.fstart, (const int32_t *)w.raw, w.flist, w.he_raw,
                           w.he_sorted, w.ndeg, w.longv, w.header);
        NRF_LAUNCH_CHECK();
    }
    NRF_TRY(adj_scan(w.ndeg, n_verts, w.bsum, w.nstart, st));
    int64_t h[2] = {0, 0};
    NRF_HIP(hipMemcpyAsync(h + 0, w.fstart + n_verts, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    NRF_HIP(hipMemcpyAsync(h + 1, w.nstart + n_verts, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    NRF_HIP(hipStreamSynchronize(st));
    *n_incident = h[0];
    *n_neighbours = h[1];
    return NRF_OK;
}

int nrf_mesh_adjacency_emit(const int32_t *d_faces, int64_t n_verts, int64_t n_faces, int64_t n_incident, int64_t n_neighbours, int64_t *d_face_start,
                            int32_t *d_face_list, int64_t *d_nbr_start, int32_t *d_nbr, int32_t *d_nbr_faces, uint8_t *d_flags, int64_t *d_stats, void *d_workspace,
                            size_t workspace_bytes, void *stream)
{
    NRF_TRY(adj_check("nrf_mesh_adjacency_emit", d_faces, n_verts, n_faces, d_workspace));
    NRF_CHECK_ARG(n_incident >= 0 && n_incident <= 3 * n_faces && n_neighbours >= 0 && n_neighbours <= 6 * n_faces,
                  "nrf_mesh_adjacency_emit: %lld incident faces / %lld neighbours cannot come from %lld faces", (long long)n_incident, (long long)n_neighbours,
                  (long long)n_faces);
    NRF_CHECK_ARG(d_face_start && d_nbr_start && d_stats && (d_flags || n_verts == 0) && (d_face_list || n_incident == 0) &&
                      ((d_nbr && d_nbr_faces) || n_neighbours == 0),
                  "nrf_mesh_adjacency_emit: null d_face_start, d_face_list, d_nbr_start, d_nbr, d_nbr_faces, d_flags or d_stats");
    Bump bump(d_workspace, workspace_bytes);
    const AdjWs w = adj_layout(bump, n_verts, n_faces);
    NRF_TRY(ws_check(bump, nrf_mesh_adjacency_workspace_bytes(n_verts, n_faces), "nrf_mesh_adjacency_emit"));
    hipStream_t st = as_stream(stream);
    // the totals are the caller's buffer sizes: a pair that is not the count call's is refused before anything is written (this read waits for the stream)
    int64_t h[2] = {0, 0};
    NRF_HIP(hipMemcpyAsync(h + 0, w.fstart + n_verts, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    NRF_HIP(hipMemcpyAsync(h + 1, w.nstart + n_verts, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    NRF_HIP(hipStreamSynchronize(st));
    NRF_CHECK_ARG(h[0] == n_incident && h[1] == n_neighbours,
                  "nrf_mesh_adjacency_emit: %lld incident faces / %lld neighbours differ from the count call's %lld / %lld (same mesh and workspace?)", (long long)n_incident,
                  (long long)n_neighbours, (long long)h[0], (long long)h[1]);
    NRF_HIP(hipMemsetAsync(d_stats, 0, 8 * sizeof(int64_t), st));
    NRF_HIP(hipMemcpyAsync(d_stats, w.header + 1, 2 * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    NRF_HIP(hipMemcpyAsync(d_face_start, w.fstart, ((size_t)n_verts + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    NRF_HIP(hipMemcpyAsync(d_nbr_start, w.nstart, ((size_t)n_verts + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    if (n_incident > 0) NRF_HIP(hipMemcpyAsync(d_face_list, w.flist, (size_t)n_incident * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    if (n_verts > 0) {
        hipLaunchKernelGGL(k_adj_emit, dim3((unsigned)ceil_div(n_verts, ADJ_BLOCK)), dim3(ADJ_BLOCK), 0, st, n_verts, (const int64_t *)w.fstart, n_incident,
                           (const int32_t *)w.he_sorted, (const int64_t *)w.nstart, n_neighbours, d_nbr, d_nbr_faces, d_flags, reinterpret_cast<unsigned long long *>(d_stats));
        NRF_LAUNCH_CHECK();
    }
    return NRF_OK;
}

int nrf_mesh_smooth(const float *d_x, float *d_out, float *d_tmp, int64_t n_verts, int channels, int iterations, float lambda, float mu, int boundary,
                    const int64_t *d_nbr_start, const int32_t *d_nbr, const int32_t *d_nbr_faces, const uint8_t *d_flags, int64_t n_neighbours, void *stream)
{
    NRF_CHECK_ARG(n_verts >= 0 && n_verts <= INT32_MAX && n_neighbours >= 0, "nrf_mesh_smooth: %lld vertices (0 .. 2^31 - 1), %lld neighbours (>= 0)", (long long)n_verts,
                  (long long)n_neighbours);
    NRF_CHECK_ARG(channels >= 1 && channels <= NRF_SMOOTH_MAX_CHANNELS, "nrf_mesh_smooth: channels must be 1 .. %d, got %d", NRF_SMOOTH_MAX_CHANNELS, channels);
    NRF_CHECK_ARG(iterations >= 0 && iterations <= INT32_MAX / 2, "nrf_mesh_smooth: iterations must be 0 .. 2^30 - 1, got %d", iterations);
    NRF_CHECK_ARG(std::isfinite(lambda) && std::isfinite(mu), "nrf_mesh_smooth: lambda and mu must be finite, got %g and %g", (double)lambda, (double)mu);
    NRF_CHECK_ARG(boundary == NRF_SMOOTH_FREE || boundary == NRF_SMOOTH_FIXED || boundary == NRF_SMOOTH_CURVE,
                  "nrf_mesh_smooth: boundary must be 0 (free), 1 (fixed) or 2 (curve), got %d", boundary);
    if (n_verts > 0) {
        NRF_CHECK_ARG(d_x && d_out && d_tmp && d_nbr_start, "nrf_mesh_smooth: null d_x, d_out, d_tmp or d_nbr_start");
        NRF_CHECK_ARG(d_x != d_out && d_x != d_tmp && d_out != d_tmp, "nrf_mesh_smooth: d_x, d_out and d_tmp must be three different buffers");
        NRF_CHECK_ARG(d_nbr || n_neighbours == 0, "nrf_mesh_smooth: null d_nbr");
        NRF_CHECK_ARG(boundary == NRF_SMOOTH_FREE || d_flags, "nrf_mesh_smooth: null d_flags with a boundary mode that reads them");
        NRF_CHECK_ARG(boundary != NRF_SMOOTH_CURVE || d_nbr_faces || n_neighbours == 0, "nrf_mesh_smooth: null d_nbr_faces with NRF_SMOOTH_CURVE");
        const uintptr_t align = channels == 2 ? 7 : (channels == 4 ? 15 : 3);
        NRF_CHECK_ARG(((reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_out) | reinterpret_cast<uintptr_t>(d_tmp)) & align) == 0,
                      "nrf_mesh_smooth: d_x, d_out and d_tmp must be aligned to a whole vertex (%d bytes)", (int)align + 1);
    }
    if (n_verts == 0) return NRF_OK;
    hipStream_t st = as_stream(stream);
    const int steps = iterations * (mu != 0.0f ? 2 : 1);
    if (steps == 0) {
        NRF_HIP(hipMemcpyAsync(d_out, d_x, (size_t)n_verts * channels * sizeof(float), hipMemcpyDeviceToDevice, st));
        return NRF_OK;
    }
    const float *src = d_x;
    for (int k = 0; k < steps; k++) {
        float *dst = ((steps - 1 - k) & 1) == 0 ? d_out : d_tmp;          // the last step writes d_out
        const float f = (mu != 0.0f && (k & 1)) ? mu : lambda;
        switch (channels) {
        case 1: smooth_launch<1>(src, dst, n_verts, f, boundary, d_nbr_start, d_nbr, d_nbr_faces, d_flags, n_neighbours, st); break;
        case 2: smooth_launch<2>(src, dst, n_verts, f, boundary, d_nbr_start, d_nbr, d_nbr_faces, d_flags, n_neighbours, st); break;
        case 3: smooth_launch<3>(src, dst, n_verts, f, boundary, d_nbr_start, d_nbr, d_nbr_faces, d_flags, n_neighbours, st); break;
        default: smooth_launch<4>(src, dst, n_verts, f, boundary, d_nbr_start, d_nbr, d_nbr_faces, d_flags, n_neighbours, st); break;
        }
        NRF_LAUNCH_CHECK();
        src = dst;
    }
    return NRF_OK;
}

int nrf_mesh_vertex_normals(const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, const int64_t *d_face_start, const int32_t *d_face_list,
                            int64_t n_incident, int weighting, float *d_out, void *stream)
{
    NRF_CHECK_ARG(adj_shape_ok(n_verts, n_faces) && n_incident >= 0 && n_incident <= 3 * n_faces,
                  "nrf_mesh_vertex_normals: %lld vertices, %lld faces (0 .. 2^31 - 1), %lld incident faces (0 .. 3 * faces)", (long long)n_verts, (long long)n_faces,
                  (long long)n_incident);
    NRF_CHECK_ARG(weighting == NRF_NORMALS_AREA || weighting == NRF_NORMALS_UNIT, "nrf_mesh_vertex_normals: weighting must be 0 (area) or 1 (unit), got %d", weighting);
    if (n_verts > 0) {
        NRF_CHECK_ARG(d_verts && d_out && d_face_start && d_verts != d_out, "nrf_mesh_vertex_normals: null d_verts, d_face_start or d_out, or d_out == d_verts");
        NRF_CHECK_ARG((d_faces || n_faces == 0) && (d_face_list || n_incident == 0), "nrf_mesh_vertex_normals: null d_faces or d_face_list");
    }
    if (n_verts == 0) return NRF_OK;
    hipLaunchKernelGGL(k_vertex_normals, dim3((unsigned)ceil_div(n_verts, ADJ_BLOCK)), dim3(ADJ_BLOCK), 0, as_stream(stream), d_verts, n_verts, d_faces, n_faces, d_face_start,
                       d_face_list, n_incident, weighting, d_out);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

}  // extern "C"
