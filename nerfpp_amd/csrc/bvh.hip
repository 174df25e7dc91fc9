// bvh.hip -- a bounding-volume hierarchy over the faces of a mesh and the two queries of the face grid on it: nrf_mesh_bvh_build, nrf_bvh_closest_on_mesh,
// nrf_bvh_ray_cast_mesh, nrf_bvh_point_codes, and the stable radix sort the build needs (nrf_sort_pairs_u32, sort.h).  The contract, the buffer's layout and the
// two pruning proofs are stated in include/nerfpp_hip.h ("Mesh BVH"); tests/bvh_ref.py restates the tree, and the queries equal tests/closest_ref.py and
// tests/raycast_ref.py (brute force over all pairs) bit for bit because they form every candidate through the functions the grid's queries use (face_grid.h, raycast.h).
//
// Build, no host round trip: k_bvh_classify (classes, n_valid, the mesh box by integer atomics on bvh_image) -> k_bvh_codes (the head, a Morton code per face) ->
//   four passes of the radix sort (codes with the face index as payload, into leaf_face) -> k_bvh_topology (Karras 2012 on the 64-bit keys (code << 32) | face, one
//   lane per internal node) -> NRF_BVH_MAX_DEPTH launches of k_bvh_refit.  A refit launch finishes the nodes whose children were finished by EARLIER launches and marks
//   them with its pass number; a mark of the current pass counts as not finished, so no launch reads what the same launch wrote and nothing is handed over between
//   workgroups.  The device's count of unfinished nodes lets the launches after the last level return after one load per block.
//   The build kernels are templates over the LEAF SOURCE (bvh_leaf<POINTS>): a face of a mesh, or -- nrf_point_bvh_build, points.hip -- the point itself, which is
//   what the face (i, i, i) gives; bvh_build_launch / bvh_point_codes_launch (bvh.h) are the one copy both entries run.
// Queries: one lane per query (ray), a private stack of NRF_BVH_MAX_DEPTH node indices, the nearer child first; a child is skipped only by a proven lower bound.
#include "reduce.h"
#include "scan.h"
#include "sort.h"
#include "workspace.h"
#include "face_grid.h"
#include "raycast.h"
#include "bvh.h"

#include <climits>
#include <cmath>

namespace nrf {

namespace {

static_assert(NRF_BVH_MAX_DEPTH == 64, "the refit's launches and the traversal stack are written for 64");

struct BvhWs {
    uint32_t *codes;         // [F] a face's code in face order
    uint32_t *sorted;        // [F] the codes in leaf order
    int32_t *mark;           // [F - 1] the refit pass that finished a node; 0: not finished
    uint32_t *box;           // [8] images: the mesh box's min xyz, max xyz; [6] n_valid; [7] unfinished nodes.  One memset pair clears all
    SortWs sort;
};

BvhWs bvh_ws_layout(Bump &b, int64_t n_faces)
{
    BvhWs s;
    s.codes = b.take<uint32_t>((size_t)n_faces);
    s.sorted = b.take<uint32_t>((size_t)n_faces);
    s.mark = b.take<int32_t>((size_t)(n_faces > 0 ? n_faces - 1 : 0));
    s.box = b.take<uint32_t>(8);
    s.sort = sort_layout(b, n_faces);
    return s;
}

__device__ __forceinline__ void face_box(const float a[3], const float b[3], const float c[3], float lo[3], float hi[3])
{
#pragma unroll
    for (int k = 0; k < 3; k++) {
        lo[k] = fminf(fminf(a[k], b[k]), c[k]);
        hi[k] = fmaxf(fmaxf(a[k], b[k]), c[k]);
    }
}

// the leaf source: the corners of leaf f and its class.  A face (cm_face), or -- POINTS -- the point verts[f] as all three corners: what cm_face gives for the
// face (f, f, f), without a face array (class 2: a non-finite coordinate; f is always inside)
template <bool POINTS>
__device__ __forceinline__ int bvh_leaf(const float *__restrict__ verts, int32_t n_verts, const int32_t *__restrict__ faces, int64_t n_faces, int64_t f, float a[3], float b[3],
                                        float c[3])
{
    if (!POINTS) return cm_face(verts, n_verts, faces, n_faces, f, a, b, c);
    if (f < 0 || f >= n_faces) return 1;
#pragma unroll
    for (int k = 0; k < 3; k++) a[k] = b[k] = c[k] = verts[f * 3 + k];
    return finite3(a) ? 0 : 2;
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const uint32_t t = __shfl_xor(v, o, 64); v = t < v ? t : v; }
    return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const uint32_t t = __shfl_xor(v, o, 64); v = t > v ? t : v; }
    return v;
}

// classes into stats[1], [2]; n_valid; the mesh box as the integer minimum / maximum of the corner images (exact and order-free)
template <bool POINTS>
__global__ void __launch_bounds__(GEO_BLOCK) k_bvh_classify(const float *__restrict__ verts, int32_t n_verts, const int32_t *__restrict__ faces, int64_t n_faces,
                                                            uint32_t *__restrict__ box, uint32_t *__restrict__ stats)
{
    __shared__ int sh[GEO_BLOCK / 64];
    const int64_t f = (int64_t)blockIdx.x * GEO_BLOCK + threadIdx.x;
    int cls = -1;
    uint32_t mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
    if (f < n_faces) {
        float a[3], b[3], c[3];
        cls = bvh_leaf<POINTS>(verts, n_verts, faces, n_faces, f, a, b, c);
        if (cls == 0) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const uint32_t ia = bvh_image(a[k]), ib = bvh_image(b[k]), ic = bvh_image(c[k]);
                mn[k] = min(min(ia, ib), ic);
                mx[k] = max(max(ia, ib), ic);
            }
        }
    }
    const unsigned long long any = __ballot(cls == 0);
    if (any) {          // uniform over the wave
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const uint32_t lo = wave_min_u32(mn[k]), hi = wave_max_u32(mx[k]);
            if ((threadIdx.x & 63) == 0) {
                atomicMin(box + k, lo);
                atomicMax(box + 3 + k, hi);
            }
        }
    }
    const int nv = block_count<GEO_BLOCK>(cls == 0, sh);
    if (threadIdx.x == 0 && nv) atomicAdd(box + 6, (uint32_t)nv);
    if (!stats) return;          // uniform
    const int t1 = block_count<GEO_BLOCK>(cls == 1, sh), t2 = block_count<GEO_BLOCK>(cls == 2, sh);
    if (threadIdx.x == 0) {
        if (t1) atomicAdd(stats + 1, (uint32_t)t1);
        if (t2) atomicAdd(stats + 2, (uint32_t)t2);
    }
}

__device__ __forceinline__ void bvh_tree_from_ws(const uint32_t *__restrict__ box, BvhTree &t)
{
    t.n_valid = box[6];
#pragma unroll
    for (int a = 0; a < 3; a++) {          // no valid face: the images are still 0xffffffff / 0, that is the NaNs of all-ones and all-zero images; the head says +inf / -inf
        t.lo[a] = t.n_valid ? bvh_unimage(box[a]) : INFINITY;
        t.hi[a] = t.n_valid ? bvh_unimage(box[3 + a]) : -INFINITY;
    }
}

// the head, and the code of every face: the centre of its coordinate box, lo * 0.5f + hi * 0.5f per axis, against the mesh box
template <bool POINTS>
__global__ void __launch_bounds__(GEO_BLOCK) k_bvh_codes(const float *__restrict__ verts, int32_t n_verts, const int32_t *__restrict__ faces, int64_t n_faces,
                                                         const uint32_t *__restrict__ box, long long *__restrict__ head, uint32_t *__restrict__ codes)
{
    BvhTree t;
    bvh_tree_from_ws(box, t);
    if (blockIdx.x == 0 && threadIdx.x < 8) {
        long long w = 0;
        const int k = threadIdx.x;
        if (k == 0) w = POINTS ? PBVH_MAGIC : BVH_MAGIC;
        if (k == 1) w = n_faces;
        if (k == 2) w = t.n_valid;
        if (k >= 3 && k < 6) w = (long long)(((unsigned long long)__float_as_uint(t.hi[k - 3]) << 32) | __float_as_uint(t.lo[k - 3]));
        head[k] = w;
    }
    const int64_t f = (int64_t)blockIdx.x * GEO_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    float a[3], b[3], c[3];
    uint32_t code = BVH_CODE_INVALID;
    if (bvh_leaf<POINTS>(verts, n_verts, faces, n_faces, f, a, b, c) == 0) {
        float lo[3], hi[3], ctr[3];
        face_box(a, b, c, lo, hi);
#pragma unroll
        for (int k = 0; k < 3; k++) ctr[k] = lo[k] * 0.5f + hi[k] * 0.5f;
        code = bvh_morton(ctr, t);
    }
    codes[f] = code;
}

// the common prefix of the keys of leaves i and j, -1 where j is no leaf.  The keys differ (the face index is part of them), so the count is below 64
__device__ __forceinline__ int bvh_delta(const uint32_t *__restrict__ sorted, const int32_t *__restrict__ leaf_face, int64_t n, unsigned long long ki, int64_t j)
{
    if (j < 0 || j >= n) return -1;
    const unsigned long long kj = ((unsigned long long)sorted[j] << 32) | (uint32_t)leaf_face[j];
    return __clzll((long long)(ki ^ kj));
}

// Karras 2012: internal node i covers the leaves [min(i, j), max(i, j)], splits them after leaf s into the node of [l, s], index s, and the node of [s + 1, r], index
// s + 1; a range of one leaf is that leaf.  Every loop halves a power of two that starts below 2^31.
__global__ void __launch_bounds__(GEO_BLOCK) k_bvh_topology(const uint32_t *__restrict__ sorted, const int32_t *__restrict__ leaf_face, uint32_t *__restrict__ box,
                                                            BvhNode *__restrict__ node)
{
    const int64_t n = box[6];
    const int64_t i = (int64_t)blockIdx.x * GEO_BLOCK + threadIdx.x;
    if (i == 0) box[7] = n > 1 ? (uint32_t)(n - 1) : 0u;          // the refit's count of unfinished nodes (read by later launches only)
    if (i >= n - 1) return;
    const unsigned long long ki = ((unsigned long long)sorted[i] << 32) | (uint32_t)leaf_face[i];
    const int d = bvh_delta(sorted, leaf_face, n, ki, i + 1) > bvh_delta(sorted, leaf_face, n, ki, i - 1) ? 1 : -1;
    const int dmin = bvh_delta(sorted, leaf_face, n, ki, i - d);
    int64_t lmax = 2;
    while (bvh_delta(sorted, leaf_face, n, ki, i + lmax * d) > dmin) lmax *= 2;          // stops at the array's end at the latest: at most 32 rounds
    int64_t l = 0;
    for (int64_t t = lmax / 2; t >= 1; t /= 2)
        if (bvh_delta(sorted, leaf_face, n, ki, i + (l + t) * d) > dmin) l += t;
    const int64_t j = i + l * d;
    const int dnode = bvh_delta(sorted, leaf_face, n, ki, j);
    int64_t s = 0;
    for (int64_t t = (l + 1) / 2;; t = (t + 1) / 2) {          // t = ceil(l / 2), ceil(l / 4), ..., 1
        if (bvh_delta(sorted, leaf_face, n, ki, i + (s + t) * d) > dnode) s += t;
        if (t <= 1) break;
    }
    const int64_t split = i + s * d + (d < 0 ? -1 : 0);
    const int64_t first = d > 0 ? i : j, last = d > 0 ? j : i;
    const int32_t c0 = first == split ? (int32_t)(-(split + 1)) : (int32_t)split;
    const int32_t c1 = last == split + 1 ? (int32_t)(-(split + 2)) : (int32_t)(split + 1);
    node[i].child[0] = c0;
    node[i].child[1] = c1;
    if (c0 >= 0) node[c0].parent = (int32_t)i;
    if (c1 >= 0) node[c1].parent = (int32_t)i;
    if (i == 0) node[0].parent = -1;
}

// the box of child c of a node: a leaf's is its face's coordinate box, an internal node's the union of the two boxes it stores
template <bool POINTS>
__device__ __forceinline__ void bvh_child_box(int32_t c, const BvhNode *__restrict__ node, const int32_t *__restrict__ leaf_face, const float *__restrict__ verts,
                                              int32_t n_verts, const int32_t *__restrict__ faces, int64_t n_faces, float lo[3], float hi[3])
{
    if (c < 0) {
        float a[3], b[3], cc[3];
        (void)bvh_leaf<POINTS>(verts, n_verts, faces, n_faces, leaf_face[-(c + 1)], a, b, cc);          // a leaf of the tree is a valid face
        face_box(a, b, cc, lo, hi);
    } else {
        const BvhNode &n = node[c];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            lo[k] = fminf(n.lo0[k], n.lo1[k]);
            hi[k] = fmaxf(n.hi0[k], n.hi1[k]);
        }
    }
}

template <bool POINTS>
__global__ void __launch_bounds__(GEO_BLOCK) k_bvh_refit(int pass, const float *__restrict__ verts, int32_t n_verts, const int32_t *__restrict__ faces, int64_t n_faces,
                                                         const int32_t *__restrict__ leaf_face, uint32_t *__restrict__ box, int32_t *__restrict__ mark,
                                                         BvhNode *__restrict__ node)
{
    __shared__ int sh[GEO_BLOCK / 64];
    // 0 only once every node is finished: a block that reads 0 has nothing to do, one that reads more finds its own nodes' state in their marks
    if (__hip_atomic_load(box + 7, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) return;          // uniform: one load per block
    const int64_t n = box[6];
    const int64_t i = (int64_t)blockIdx.x * GEO_BLOCK + threadIdx.x;
    bool done = false;
    if (i < n - 1 && mark[i] == 0) {
        const int32_t c0 = node[i].child[0], c1 = node[i].child[1];
        const int m0 = c0 < 0 ? -1 : mark[c0], m1 = c1 < 0 ? -1 : mark[c1];          // a leaf is finished; a mark of this pass is not
        if (m0 != 0 && m0 != pass && m1 != 0 && m1 != pass) {
            float lo[3], hi[3];
            bvh_child_box<POINTS>(c0, node, leaf_face, verts, n_verts, faces, n_faces, lo, hi);
#pragma unroll
            for (int k = 0; k < 3; k++) { node[i].lo0[k] = lo[k]; node[i].hi0[k] = hi[k]; }
            bvh_child_box<POINTS>(c1, node, leaf_face, verts, n_verts, faces, n_faces, lo, hi);
#pragma unroll
            for (int k = 0; k < 3; k++) { node[i].lo1[k] = lo[k]; node[i].hi1[k] = hi[k]; }
            mark[i] = pass;
            done = true;
        }
    }
    const int total = block_count<GEO_BLOCK>(done, sh);
    if (threadIdx.x == 0 && total) atomicSub(box + 7, (uint32_t)total);
}

// ---------------------------------------------------------------------------------------------- queries
struct BvhMesh {
    const float *verts;
    const int32_t *faces;
    const long long *head;
    const int32_t *leaf_face;
    const BvhNode *node;
    int32_t n_verts;
    int64_t n_faces;
};

__global__ void __launch_bounds__(GEO_BLOCK) k_bvh_closest(const float *__restrict__ query, int64_t nq, const int32_t *__restrict__ order, BvhMesh m, float md2,
                                                           float *__restrict__ dist2, int32_t *__restrict__ face, float *__restrict__ uv, float *__restrict__ point,
                                                           uint32_t *__restrict__ stats)
{
    __shared__ int sh[GEO_BLOCK / 64];
    BvhTree t;
    if (!bvh_head_read(m.head, m.n_faces, t)) return;          // uniform: not a buffer built for these faces; nothing more of it is read, nothing written
    const int64_t lane_i = (int64_t)blockIdx.x * GEO_BLOCK + threadIdx.x;
    int64_t qi = lane_i;
    if (order && lane_i < nq) qi = order[lane_i];
    const bool live = lane_i < nq && qi >= 0 && qi < nq;          // an order that is no permutation is the caller's breach; it still writes nowhere else
    float q[3] = {0.0f, 0.0f, 0.0f};
    if (live) { q[0] = query[qi * 3 + 0]; q[1] = query[qi * 3 + 1]; q[2] = query[qi * 3 + 2]; }
    const bool finite = live && finite3(q);
    unsigned long long best = NN_NONE;
    if (finite && t.n_valid == 1) cm_take(q, m.verts, m.n_verts, m.faces, m.n_faces, m.leaf_face[0], md2, best);
    if (finite && t.n_valid > 1) {
        int32_t stack[NRF_BVH_MAX_DEPTH];
        int sp = 0;
        int32_t at = 0;
        for (;;) {          // every node is visited at most once: the tree's size bounds the loop
            BvhNode n;
            bvh_node_load(m.node, at, n);
            const float b0 = bvh_box_d2(q, n.lo0, n.hi0), b1 = bvh_box_d2(q, n.lo1, n.hi1);
            const bool swap = b1 < b0;          // the nearer child first
            const int32_t ca = swap ? n.child[1] : n.child[0], cb = swap ? n.child[0] : n.child[1];
            const float ba = swap ? b1 : b0, bb = swap ? b0 : b1;
            int32_t next = -1;
            // skipped iff the bound lies strictly above what can still win or tie
            if (!(ba > fminf(key_value(best), md2))) {
                if (ca < 0) cm_take(q, m.verts, m.n_verts, m.faces, m.n_faces, m.leaf_face[-(ca + 1)], md2, best);
                else next = ca;
            }
            if (!(bb > fminf(key_value(best), md2))) {
                if (cb < 0) cm_take(q, m.verts, m.n_verts, m.faces, m.n_faces, m.leaf_face[-(cb + 1)], md2, best);
                else if (next < 0) next = cb;
                else if (sp < NRF_BVH_MAX_DEPTH) stack[sp++] = cb;          // always, for a tree of the build: its height is at most 62
            }
            if (next < 0) {
                if (sp == 0) break;
                next = stack[--sp];
            }
            at = next;
        }
    }
    if (live) cm_write(q, qi, best, m.verts, m.n_verts, m.faces, m.n_faces, dist2, face, uv, point);
    if (!stats) return;          // uniform
    const int total = block_count<GEO_BLOCK>(live && !finite, sh);
    if (threadIdx.x == 0 && total) atomicAdd(stats + 0, (uint32_t)total);
}

template <bool ANY>
__global__ void __launch_bounds__(GEO_BLOCK) k_bvh_ray_cast(const float *__restrict__ rays, int64_t n, int stride, const int32_t *__restrict__ order, BvhMesh m, int cull,
                                                            float *__restrict__ out_t, int32_t *__restrict__ face, float *__restrict__ uv, float *__restrict__ point,
                                                            uint8_t *__restrict__ hit, uint32_t *__restrict__ stats)
{
    __shared__ int sh[GEO_BLOCK / 64];
    BvhTree t;
    if (!bvh_head_read(m.head, m.n_faces, t)) return;          // uniform, as in k_bvh_closest
    const int64_t lane_i = (int64_t)blockIdx.x * GEO_BLOCK + threadIdx.x;
    int64_t i = lane_i;
    if (order && lane_i < n) i = order[lane_i];
    const bool live = lane_i < n && i >= 0 && i < n;
    RcRay r;
    bool valid = false;
    if (live) valid = rc_load_ray(rays, i, stride, r);
    unsigned long long best = NN_NONE;
    if (valid && t.n_valid == 1) rc_take(r, m.verts, m.n_verts, m.faces, m.n_faces, m.leaf_face[0], cull, best);
    if (valid && t.n_valid > 1 && r.lo <= r.hi) {
        int32_t stack[NRF_BVH_MAX_DEPTH];
        int sp = 0;
        int32_t at = 0;
        for (;;) {
            BvhNode nd;
            bvh_node_load(m.node, at, nd);
            float t0 = 0.0f, t1 = 0.0f;
            const bool in0 = bvh_box_ray(r, nd.lo0, nd.hi0, t0), in1 = bvh_box_ray(r, nd.lo1, nd.hi1, t1);
            const bool swap = in1 && (!in0 || t1 < t0);          // the child the ray enters first
            const int32_t ca = swap ? nd.child[1] : nd.child[0], cb = swap ? nd.child[0] : nd.child[1];
            const bool ia = swap ? in1 : in0, ib = swap ? in0 : in1;
            const float ta = swap ? t1 : t0, tb = swap ? t0 : t1;
            int32_t next = -1;
            // visited iff the interval is not empty and begins at or before the best t: an equal t with a lower face index must still be found
            if (ia && ta <= key_value(best)) {
                if (ca < 0) rc_take(r, m.verts, m.n_verts, m.faces, m.n_faces, m.leaf_face[-(ca + 1)], cull, best);
                else next = ca;
            }
            if (ANY && best != NN_NONE) break;
            if (ib && tb <= key_value(best)) {
                if (cb < 0) rc_take(r, m.verts, m.n_verts, m.faces, m.n_faces, m.leaf_face[-(cb + 1)], cull, best);
                else if (next < 0) next = cb;
                else if (sp < NRF_BVH_MAX_DEPTH) stack[sp++] = cb;
            }
            if (ANY && best != NN_NONE) break;
            if (next < 0) {
                if (sp == 0) break;
                next = stack[--sp];
            }
            at = next;
        }
    }
    if (live) rc_write(r, i, best, m.verts, m.n_verts, m.faces, m.n_faces, cull, out_t, face, uv, point, hit);
    if (!stats) return;          // uniform
    const int total = block_count<GEO_BLOCK>(live && !valid, sh);
    if (threadIdx.x == 0 && total) atomicAdd(stats + 0, (uint32_t)total);
}

__global__ void __launch_bounds__(GEO_BLOCK) k_bvh_point_codes(const float *__restrict__ points, int64_t n, int stride, const long long *__restrict__ head, int64_t n_faces,
                                                               long long magic, uint32_t *__restrict__ codes)
{
    BvhTree t;
    if (!bvh_head_read(head, n_faces, t, magic)) return;          // uniform
    const int64_t i = (int64_t)blockIdx.x * GEO_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float c[3] = {points[i * stride + 0], points[i * stride + 1], points[i * stride + 2]};
    codes[i] = bvh_morton(c, t);
}

template <bool POINTS>
static int bvh_build_run(const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, void *d_bvh, size_t bvh_bytes, uint32_t *d_stats, void *d_workspace,
                         size_t workspace_bytes, hipStream_t st, const char *who)
{
    Bump bump(d_workspace, workspace_bytes);
    const BvhWs ws = bvh_ws_layout(bump, n_faces);
    NRF_TRY(ws_check(bump, bvh_build_workspace_bytes(n_faces), who));
    Bump bb(d_bvh, bvh_bytes);
    const BvhBuf buf = bvh_layout(bb, n_faces);
    const int64_t fb = ceil_div(n_faces, GEO_BLOCK), nb = ceil_div(n_faces - 1, GEO_BLOCK);
    NRF_HIP(hipMemsetAsync(d_bvh, 0, bvh_bytes, st));          // unused nodes, spare words and the padding: the same bytes on every run
    NRF_HIP(hipMemsetAsync(ws.box, 0xff, 3 * sizeof(uint32_t), st));
    NRF_HIP(hipMemsetAsync(ws.box + 3, 0, 5 * sizeof(uint32_t), st));
    if (n_faces > 1) NRF_HIP(hipMemsetAsync(ws.mark, 0, (size_t)(n_faces - 1) * sizeof(int32_t), st));
    if (n_faces > 0) {
        hipLaunchKernelGGL(k_bvh_classify<POINTS>, dim3((unsigned)fb), dim3(GEO_BLOCK), 0, st, d_verts, (int32_t)n_verts, d_faces, n_faces, ws.box, d_stats);
        NRF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_bvh_codes<POINTS>, dim3((unsigned)(fb > 0 ? fb : 1)), dim3(GEO_BLOCK), 0, st, d_verts, (int32_t)n_verts, d_faces, n_faces, (const uint32_t *)ws.box,
                       buf.head, ws.codes);
    NRF_LAUNCH_CHECK();
    if (n_faces == 0) return NRF_OK;
    NRF_TRY(sort_pairs_launch(ws.codes, nullptr, n_faces, 0, 32, ws.sorted, buf.leaf_face, ws.sort, st));
    if (n_faces == 1) return NRF_OK;
    hipLaunchKernelGGL(k_bvh_topology, dim3((unsigned)nb), dim3(GEO_BLOCK), 0, st, (const uint32_t *)ws.sorted, (const int32_t *)buf.leaf_face, ws.box, buf.node);
    NRF_LAUNCH_CHECK();
    for (int pass = 1; pass <= NRF_BVH_MAX_DEPTH; pass++) {
        hipLaunchKernelGGL(k_bvh_refit<POINTS>, dim3((unsigned)nb), dim3(GEO_BLOCK), 0, st, pass, d_verts, (int32_t)n_verts, d_faces, n_faces, (const int32_t *)buf.leaf_face,
                           ws.box, ws.mark, buf.node);
        NRF_LAUNCH_CHECK();
    }
    return NRF_OK;
}

}  // namespace

size_t bvh_build_workspace_bytes(int64_t n_leaves)
{
    if (n_leaves < 0 || n_leaves > INT32_MAX) return 0;
    return measure([&](Bump &b) { bvh_ws_layout(b, n_leaves); });
}

int bvh_build_launch(bool points, const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_leaves, void *d_bvh, size_t bvh_bytes, uint32_t *d_stats,
                     void *d_workspace, size_t workspace_bytes, hipStream_t st, const char *who)
{
    return points ? bvh_build_run<true>(d_verts, n_verts, d_faces, n_leaves, d_bvh, bvh_bytes, d_stats, d_workspace, workspace_bytes, st, who)
                  : bvh_build_run<false>(d_verts, n_verts, d_faces, n_leaves, d_bvh, bvh_bytes, d_stats, d_workspace, workspace_bytes, st, who);
}

int bvh_point_codes_launch(const float *d_points, int64_t n, int stride, const void *d_bvh, int64_t n_leaves, long long magic, uint32_t *d_codes, hipStream_t st)
{
    hipLaunchKernelGGL(k_bvh_point_codes, dim3((unsigned)ceil_div(n, GEO_BLOCK)), dim3(GEO_BLOCK), 0, st, d_points, n, stride, (const long long *)d_bvh, n_leaves, magic, d_codes);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

}  // namespace nrf

using namespace nrf;

extern "C" {

size_t nrf_sort_workspace_bytes(int64_t n) { return sort_workspace_bytes(n); }

int nrf_sort_pairs_u32(const uint32_t *d_keys, const int32_t *d_values, int64_t n, int begin_bit, int end_bit, uint32_t *d_keys_out, int32_t *d_values_out,
                       void *d_workspace, size_t workspace_bytes, void *stream)
{
    NRF_CHECK_ARG(n >= 0 && n <= INT32_MAX, "nrf_sort_pairs_u32: %lld pairs (0 .. 2^31 - 1)", (long long)n);
    NRF_CHECK_ARG(begin_bit >= 0 && begin_bit <= end_bit && end_bit <= 32, "nrf_sort_pairs_u32: bits [%d, %d) are no part of [0, 32)", begin_bit, end_bit);
    NRF_CHECK_ARG(n == 0 || (d_keys && d_keys_out && d_values_out), "nrf_sort_pairs_u32: null d_keys, d_keys_out or d_values_out");
    NRF_CHECK_ARG(n == 0 || (d_keys_out != d_keys && d_values_out != d_values), "nrf_sort_pairs_u32: the outputs must not be the inputs");
    NRF_CHECK_ARG(d_workspace && (reinterpret_cast<uintptr_t>(d_workspace) & 7) == 0, "nrf_sort_pairs_u32: the workspace must be non-null and 8-byte aligned");
    Bump bump(d_workspace, workspace_bytes);
    const SortWs ws = sort_layout(bump, n);
    NRF_TRY(ws_check(bump, nrf_sort_workspace_bytes(n), "nrf_sort_pairs_u32"));
    if (n == 0) return NRF_OK;
    return sort_pairs_launch(d_keys, d_values, n, begin_bit, end_bit, d_keys_out, d_values_out, ws, as_stream(stream));
}

size_t nrf_mesh_bvh_bytes(int64_t n_faces)
{
    if (n_faces < 0 || n_faces > INT32_MAX) return 0;
    return measure([&](Bump &b) { bvh_layout(b, n_faces); });
}

size_t nrf_mesh_bvh_workspace_bytes(int64_t n_faces) { return bvh_build_workspace_bytes(n_faces); }

size_t nrf_bvh_query_workspace_bytes(int64_t n)
{
    (void)n;
    return 0;          // the traversal keeps its stack in the lane; the argument pair stays in the entries for a tier that needs one
}

// the checks every entry over a mesh and its BVH buffer makes
#define NRF_BVH_CHECK(who)                                                                                                                                                 \
    NRF_CHECK_ARG(sample_shape_ok(n_verts, n_faces), who ": %lld vertices, %lld faces (both 0 .. 2^31 - 1)", (long long)n_verts, (long long)n_faces);                     \
    NRF_CHECK_ARG(n_faces == 0 || d_faces, who ": null d_faces");                                                                                                         \
    NRF_CHECK_ARG(d_verts || n_verts == 0 || n_faces == 0, who ": null d_verts");                                                                                         \
    NRF_CHECK_ARG(d_bvh && (reinterpret_cast<uintptr_t>(d_bvh) & 63) == 0, who ": the BVH buffer must be non-null and 64-byte aligned");                                  \
    NRF_CHECK_ARG(bvh_bytes == nrf_mesh_bvh_bytes(n_faces), who ": a BVH buffer of %zu bytes was not built for %lld faces (nrf_mesh_bvh_bytes gives %zu)", bvh_bytes,     \
                  (long long)n_faces, nrf_mesh_bvh_bytes(n_faces))

int nrf_mesh_bvh_build(const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, void *d_bvh, size_t bvh_bytes, uint32_t *d_stats, void *d_workspace,
                       size_t workspace_bytes, void *stream)
{
    NRF_BVH_CHECK("nrf_mesh_bvh_build");
    NRF_CHECK_ARG(d_workspace && (reinterpret_cast<uintptr_t>(d_workspace) & 7) == 0, "nrf_mesh_bvh_build: the workspace must be non-null and 8-byte aligned");
    return bvh_build_launch(false, d_verts, n_verts, d_faces, n_faces, d_bvh, bvh_bytes, d_stats, d_workspace, workspace_bytes, as_stream(stream), "nrf_mesh_bvh_build");
}

int nrf_bvh_closest_on_mesh(const float *d_query, int64_t nq, const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, const void *d_bvh,
                            size_t bvh_bytes, const int32_t *d_order, float max_dist, float *d_dist2, int32_t *d_face, float *d_uv, float *d_point, uint32_t *d_stats,
                            void *d_workspace, size_t workspace_bytes, void *stream)
{
    (void)d_workspace;
    (void)workspace_bytes;          // nrf_bvh_query_workspace_bytes is 0: any pair is accepted
    NRF_CHECK_ARG(nq >= 0 && nq <= INT32_MAX, "nrf_bvh_closest_on_mesh: %lld queries (0 .. 2^31 - 1)", (long long)nq);
    NRF_BVH_CHECK("nrf_bvh_closest_on_mesh");
    NRF_CHECK_ARG(nq == 0 || (d_query && d_dist2 && d_face), "nrf_bvh_closest_on_mesh: null d_query, d_dist2 or d_face");
    NRF_CHECK_ARG(max_dist >= 0.0f, "nrf_bvh_closest_on_mesh: max_dist must be >= 0 or +inf (got %g)", (double)max_dist);          // NaN fails
    if (nq == 0) return NRF_OK;
    Bump bb(const_cast<void *>(d_bvh), bvh_bytes);
    const BvhBuf buf = bvh_layout(bb, n_faces);
    const BvhMesh m = {d_verts, d_faces, buf.head, buf.leaf_face, buf.node, (int32_t)n_verts, n_faces};
    hipLaunchKernelGGL(k_bvh_closest, dim3((unsigned)ceil_div(nq, GEO_BLOCK)), dim3(GEO_BLOCK), 0, as_stream(stream), d_query, nq, d_order, m, max_dist * max_dist, d_dist2,
                       d_face, d_uv, d_point, d_stats);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

int nrf_bvh_ray_cast_mesh(const float *d_rays, int64_t n_rays, int stride, const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, const void *d_bvh,
                          size_t bvh_bytes, const int32_t *d_order, int cull, int mode, float *d_t, int32_t *d_face, float *d_uv, float *d_point, uint8_t *d_hit,
                          uint32_t *d_stats, void *d_workspace, size_t workspace_bytes, void *stream)
{
    (void)d_workspace;
    (void)workspace_bytes;
    NRF_CHECK_ARG(n_rays >= 0 && n_rays <= INT32_MAX, "nrf_bvh_ray_cast_mesh: %lld rays (0 .. 2^31 - 1)", (long long)n_rays);
    NRF_CHECK_ARG(stride >= 8 && stride <= NRF_RC_MAX_STRIDE, "nrf_bvh_ray_cast_mesh: a ray stride of %d floats (8 .. %d)", stride, NRF_RC_MAX_STRIDE);
    NRF_BVH_CHECK("nrf_bvh_ray_cast_mesh");
    NRF_CHECK_ARG(cull >= NRF_RC_CULL_NONE && cull <= NRF_RC_CULL_FRONT, "nrf_bvh_ray_cast_mesh: cull %d is none of NRF_RC_CULL_NONE / _BACK / _FRONT", cull);
    NRF_CHECK_ARG(mode == NRF_RC_CLOSEST || mode == NRF_RC_ANY, "nrf_bvh_ray_cast_mesh: mode %d is neither NRF_RC_CLOSEST nor NRF_RC_ANY", mode);
    NRF_CHECK_ARG(n_rays == 0 || d_rays, "nrf_bvh_ray_cast_mesh: null d_rays");
    NRF_CHECK_ARG(n_rays == 0 || mode != NRF_RC_CLOSEST || (d_t && d_face), "nrf_bvh_ray_cast_mesh: null d_t or d_face in closest mode");
    NRF_CHECK_ARG(n_rays == 0 || mode != NRF_RC_ANY || (d_hit && !d_t && !d_face && !d_uv && !d_point),
                  "nrf_bvh_ray_cast_mesh: any mode writes d_hit alone (null d_hit, or a d_t, d_face, d_uv or d_point that is not null)");
    if (n_rays == 0) return NRF_OK;
    Bump bb(const_cast<void *>(d_bvh), bvh_bytes);
    const BvhBuf buf = bvh_layout(bb, n_faces);
    const BvhMesh m = {d_verts, d_faces, buf.head, buf.leaf_face, buf.node, (int32_t)n_verts, n_faces};
    const dim3 blocks((unsigned)ceil_div(n_rays, GEO_BLOCK));
    if (mode == NRF_RC_ANY)
        hipLaunchKernelGGL(k_bvh_ray_cast<true>, blocks, dim3(GEO_BLOCK), 0, as_stream(stream), d_rays, n_rays, stride, d_order, m, cull, d_t, d_face, d_uv, d_point, d_hit,
                           d_stats);
    else
        hipLaunchKernelGGL(k_bvh_ray_cast<false>, blocks, dim3(GEO_BLOCK), 0, as_stream(stream), d_rays, n_rays, stride, d_order, m, cull, d_t, d_face, d_uv, d_point, d_hit,
                           d_stats);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

int nrf_bvh_point_codes(const float *d_points, int64_t n, int stride, const void *d_bvh, size_t bvh_bytes, int64_t n_faces, uint32_t *d_codes, void *stream)
{
    NRF_CHECK_ARG(n >= 0 && n <= INT32_MAX, "nrf_bvh_point_codes: %lld points (0 .. 2^31 - 1)", (long long)n);
    NRF_CHECK_ARG(stride >= 3 && stride <= NRF_RC_MAX_STRIDE, "nrf_bvh_point_codes: a stride of %d floats (3 .. %d)", stride, NRF_RC_MAX_STRIDE);
    NRF_CHECK_ARG(n_faces >= 0 && n_faces <= INT32_MAX, "nrf_bvh_point_codes: %lld faces (0 .. 2^31 - 1)", (long long)n_faces);
    NRF_CHECK_ARG(d_bvh && (reinterpret_cast<uintptr_t>(d_bvh) & 63) == 0, "nrf_bvh_point_codes: the BVH buffer must be non-null and 64-byte aligned");
    NRF_CHECK_ARG(bvh_bytes == nrf_mesh_bvh_bytes(n_faces), "nrf_bvh_point_codes: a BVH buffer of %zu bytes was not built for %lld faces (nrf_mesh_bvh_bytes gives %zu)",
                  bvh_bytes, (long long)n_faces, nrf_mesh_bvh_bytes(n_faces));
    NRF_CHECK_ARG(n == 0 || (d_points && d_codes), "nrf_bvh_point_codes: null d_points or d_codes");
    if (n == 0) return NRF_OK;
    return bvh_point_codes_launch(d_points, n, stride, d_bvh, n_faces, BVH_MAGIC, d_codes, as_stream(stream));
}

}  // extern "C"
