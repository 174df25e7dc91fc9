// bvh.h -- the layout of the caller-owned BVH buffer of nrf_mesh_bvh_build and what its build and its queries (bvh.hip) share: the head (BvhHead), the 64-byte node
// (BvhNode), the order-preserving integer image of a float the mesh box is reduced on, the Morton code of a point against that box, and the two pruning bounds of a
// node box (bvh_box_d2 for a point, bvh_box_ray for a ray).  The contract, the layout and both proofs are stated in include/nerfpp_hip.h ("Mesh BVH");
// tests/bvh_ref.py restates the tree and reads a built buffer back word for word.
#pragma once

#include "common.h"
#include "workspace.h"
#include "raycast.h"

namespace nrf {

constexpr long long BVH_MAGIC = 0x4e52464256483031ll;          // "NRFBVH01": the first word of a built buffer
constexpr long long PBVH_MAGIC = 0x4e52465042563031ll;         // "NRFPBV01": the first word of a buffer built over points (nrf_point_bvh_build); every other byte is the mesh build's
constexpr uint32_t BVH_CODE_INVALID = 1u << 30;                // the code of a face that is not valid: above every 30-bit code, so such faces sort last

struct BvhNode {             // 64 bytes: one fetch brings both children's boxes
    float lo0[3], hi0[3], lo1[3], hi1[3];
    int32_t child[2];        // >= 0: an internal node; -(k + 1): the leaf at sorted position k
    int32_t parent;          // -1 for the root
    int32_t spare;           // 0
};
static_assert(sizeof(BvhNode) == 64, "a node is one 64-byte read");

struct BvhBuf {
    long long *head;         // [8] magic, F, n_valid, the bits of the mesh box two floats to a word (lo | hi << 32 per axis), 0, 0
    int32_t *leaf_face;      // [F] the face of sorted position k; positions n_valid .. F - 1 hold the faces that are not valid
    BvhNode *node;           // [max(F - 1, 0)] internal nodes 0 .. n_valid - 2, node 0 the root; the rest stays zero
};

inline BvhBuf bvh_layout(Bump &b, int64_t n_faces)
{
    BvhBuf s;
    s.head = b.take<long long>(8);
    s.leaf_face = b.take<int32_t>((size_t)n_faces);
    s.node = b.take<BvhNode>((size_t)(n_faces > 0 ? n_faces - 1 : 0));
    return s;
}

// what a query reads of the head before anything else; false: not a buffer built for these faces
struct BvhTree {
    int64_t n_valid;
    float lo[3], hi[3];
};

__device__ __forceinline__ bool bvh_head_read(const long long *__restrict__ head, int64_t n_faces, BvhTree &t, long long magic = BVH_MAGIC)
{
    if (head[0] != magic || head[1] != (long long)n_faces) return false;
    t.n_valid = head[2];
    if (t.n_valid < 0 || t.n_valid > n_faces) return false;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const unsigned long long w = (unsigned long long)head[3 + a];
        t.lo[a] = __uint_as_float((uint32_t)w);
        t.hi[a] = __uint_as_float((uint32_t)(w >> 32));
    }
    return true;
}

// a node as four 16-byte reads
__device__ __forceinline__ void bvh_node_load(const BvhNode *__restrict__ node, int32_t i, BvhNode &n)
{
    const float4 *src = reinterpret_cast<const float4 *>(node + i);
    float4 *dst = reinterpret_cast<float4 *>(&n);
#pragma unroll
    for (int k = 0; k < 4; k++) dst[k] = src[k];
}

// the image of a float whose unsigned order is the float's order (-0 below +0); finite inputs only
__device__ __forceinline__ uint32_t bvh_image(float x)
{
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float bvh_unimage(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

// 10 bits of one axis: c against [lo, hi] of the mesh box, clamped; an axis of zero or non-finite extent, or a NaN, gives cell 0
__device__ __forceinline__ uint32_t bvh_axis_cell(float c, float lo, float hi)
{
    const float e = hi - lo;
    if (!(e > 0.0f) || !(e < INFINITY)) return 0u;
    const float x = floorf(((c - lo) / e) * 1024.0f);
    return (uint32_t)fminf(fmaxf(x, 0.0f), 1023.0f);          // fmaxf(NaN, 0) is 0
}

__device__ __forceinline__ uint32_t bvh_spread(uint32_t v)          // bit k of a 10-bit v goes to bit 3k
{
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

__device__ __forceinline__ uint32_t bvh_morton(const float c[3], const BvhTree &t)
{
    return bvh_spread(bvh_axis_cell(c[0], t.lo[0], t.hi[0])) | (bvh_spread(bvh_axis_cell(c[1], t.lo[1], t.hi[1])) << 1) |
           (bvh_spread(bvh_axis_cell(c[2], t.lo[2], t.hi[2])) << 2);
}

// the squared distance of q to the box [lo, hi] in nn_d2's order: a lower bound of d2 for every face whose coordinate box lies inside (header: WHY IT IS EXACT)
__device__ __forceinline__ float bvh_box_d2(const float q[3], const float lo[3], const float hi[3])
{
    float g[3];
#pragma unroll
    for (int a = 0; a < 3; a++) g[a] = q[a] < lo[a] ? lo[a] - q[a] : (q[a] > hi[a] ? q[a] - hi[a] : 0.0f);
    return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
}

constexpr float BVH_RAY_MARGIN = 1.0f / 1024.0f;               // the widening of a node box, relative to max(|o|_inf, |lo|_inf, |hi|_inf)
constexpr float BVH_RAY_MIN_SCALE = 7.888609052210118e-31f;    // 2^-100: below it the widening is infinite (every node is visited)

// the parameter interval of ray r inside the widened box: false where it is empty; t_in is the interval's lower end (header: WHY THE TRAVERSAL CANNOT MISS)
__device__ __forceinline__ bool bvh_box_ray(const RcRay &r, const float lo[3], const float hi[3], float &t_in)
{
    float M = r.o_inf;
#pragma unroll
    for (int a = 0; a < 3; a++) M = fmaxf(M, fmaxf(fabsf(lo[a]), fabsf(hi[a])));
    const float m = M >= BVH_RAY_MIN_SCALE ? BVH_RAY_MARGIN * M : INFINITY;
    float t0 = r.lo, t1 = r.hi;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float wlo = lo[a] - m, whi = hi[a] + m;
        if (r.d[a] == 0.0f) {
            if (r.o[a] < wlo || r.o[a] > whi) return false;
        } else {
            float ta = (wlo - r.o[a]) / r.d[a], tb = (whi - r.o[a]) / r.d[a];
            if (ta > tb) { const float s = ta; ta = tb; tb = s; }
            t0 = ta > t0 ? ta : t0;
            t1 = tb < t1 ? tb : t1;
        }
    }
    t_in = t0;
    return t0 <= t1;
}

// ---- what bvh.hip offers points.hip: the one copy of the build and of the code kernel, over either leaf source (host side; defined in bvh.hip) ----
// points == false: leaf f is face d_faces[f] of d_verts, the head says BVH_MAGIC.  points == true: leaf f is the point d_verts[f] (d_faces unused, n_verts == n_leaves),
// the head says PBVH_MAGIC; every other byte is what the face build writes for faces [[i, i, i]].  The caller has checked its arguments; the workspace is checked here
size_t bvh_build_workspace_bytes(int64_t n_leaves);
int bvh_build_launch(bool points, const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_leaves, void *d_bvh, size_t bvh_bytes, uint32_t *d_stats,
                     void *d_workspace, size_t workspace_bytes, hipStream_t st, const char *who);
int bvh_point_codes_launch(const float *d_points, int64_t n, int stride, const void *d_bvh, int64_t n_leaves, long long magic, uint32_t *d_codes, hipStream_t st);

}  // namespace nrf
