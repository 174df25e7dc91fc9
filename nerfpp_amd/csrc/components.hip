// components.hip -- connected components of a triangle list (nrf_mesh_components) and of a masked lattice (nrf_lattice_components).  The reference has neither;
// the contract is stated in include/nerfpp_hip.h and restated in numpy by tests/components_ref.py, which the GPU tests compare with integer for integer.
//
// A lock-free union-find over int32 parent[n] (item = vertex or lattice point), six launches:
//   k_cc_init      parent[i] = i (mesh: label[i] = -1, "used by no face")
//   k_cc_union_*   one thread per face: union(v0, v1), union(v1, v2); one thread per set lattice point: union with its set neighbours of the forward
//                  half-neighbourhood (every undirected edge once)
//   k_cc_resolve   root[i] = the root of i, by pointer chasing, into the label array; per-block count of the roots (root[i] == i) among the items that take part
//   k_totals_scan  (scan.h) one workgroup: exclusive scan of the per-block counts; header[0] = K
//   k_cc_rank      rank of every root = its block's offset + the count of roots before it in the block (written over parent, which is dead by then)
//   k_cc_label     label[i] = rank[root[i]]
// Invariants of the union launch:
//   * parent[i] <= i always, and a parent only ever decreases: the root of a tree is its smallest member.
//   * a root r is hooked only by an agent-scope compare-and-swap parent[r]: r -> lo with lo < r, so exactly one thread hooks it and nobody overwrites a hook.
//   * after a failed compare-and-swap the thread goes on from the value the operation returned (r's new parent, which is in r's component); it never reads the
//     word again and never waits for another thread.
//   * every loop strictly decreases an index (find: x -> parent[x] < x; unite: the larger of the pair), so every loop is bounded by the index it started from.
//   * while unions are in flight parent is read with relaxed agent-scope atomic loads only: the vector L1 is per CU and other CUs' stores never refresh it.  A
//     stale value is an older, larger ancestor of the same tree: the walk gets longer, never wrong, and the compare-and-swap decides on the current value.
//   * path shortening is an atomic min on nodes seen as non-roots (a non-root never becomes a root again), with a value that is an ancestor: it keeps all of the above.
// Resolve is a launch of its own, so it sees every hook through the kernel boundary and reads with plain loads.  The labels are canonical: the rank of a
// component is the rank of its smallest member, whatever the order the unions ran in, so two runs -- and any correct implementation -- give the same array.
#include "common.h"
#include "scan.h"
#include "workspace.h"

#include <climits>

namespace nrf {

namespace {

constexpr int CC_BLOCK = 256;

__device__ __forceinline__ int32_t load_parent(const int32_t *parent, int32_t x) { return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x's tree as far as this thread can see it; halves the path on the way (x -> grandparent when x's parent is no root)
__device__ __forceinline__ int32_t find_root(int32_t *parent, int32_t x)
{
    int32_t p = load_parent(parent, x);
    while (p != x) {                                       // p < x: the walk goes down
        const int32_t g = load_parent(parent, p);
        if (g != p) __hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);         // x is no root (p < x) and g < p is an ancestor of x
        x = p;
        p = g;
    }
    return x;
}

__device__ __forceinline__ void unite(int32_t *parent, int32_t a, int32_t b)
{
    while (true) {                                         // max(a, b) decreases in every round: a failed hook replaces it by its smaller parent
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        int32_t seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        a = seen;                                          // hi was hooked meanwhile: seen < hi is in hi's component; unite it with lo
        b = lo;
    }
}

__global__ void __launch_bounds__(CC_BLOCK) k_cc_init(int64_t n, int32_t *__restrict__ parent, int32_t *__restrict__ label)
{
    const int64_t i = (int64_t)blockIdx.x * CC_BLOCK + threadIdx.x;
    if (i >= n) return;
    parent[i] = (int32_t)i;
    if (label) label[i] = -1;
}

// header[1] counts the vertex indices outside [0, n_verts); a face that holds one is skipped whole (nothing is read or written at a bad index)
__global__ void __launch_bounds__(CC_BLOCK) k_cc_union_faces(const int32_t *__restrict__ faces, int64_t n_tris, int32_t n_verts, int32_t *parent, int32_t *label,
                                                             unsigned long long *__restrict__ bad)
{
    const int64_t t = (int64_t)blockIdx.x * CC_BLOCK + threadIdx.x;
    if (t >= n_tris) return;
    const int32_t v0 = faces[t * 3 + 0], v1 = faces[t * 3 + 1], v2 = faces[t * 3 + 2];
    const int nbad = (v0 < 0 || v0 >= n_verts) + (v1 < 0 || v1 >= n_verts) + (v2 < 0 || v2 >= n_verts);
    if (nbad) {
        atomicAdd(bad, (unsigned long long)nbad);          // a count: its value does not depend on the order of the additions
        return;
    }
    label[v0] = 0; label[v1] = 0; label[v2] = 0;           // "used by a face" (every writer stores the same value; resolve replaces it by the root)
    unite(parent, v0, v1);
    unite(parent, v1, v2);
}

struct Lattice {
    int nx, ny, nz;
    int64_t n;
    int n_offsets;           // 3, 7 or 13: the forward half of the 6-, 14- (Kuhn) or 26-neighbourhood
    int8_t off[13][3];
};

__global__ void __launch_bounds__(CC_BLOCK) k_cc_union_lattice(Lattice g, const uint8_t *__restrict__ mask, int32_t *parent)
{
    const int64_t i = (int64_t)blockIdx.x * CC_BLOCK + threadIdx.x;
    if (i >= g.n || !mask[i]) return;
    const int64_t yz = i / g.nx;
    const int x = (int)(i - yz * g.nx), y = (int)(yz % g.ny), z = (int)(yz / g.ny);
    for (int o = 0; o < g.n_offsets; o++) {
        const int xx = x + g.off[o][0], yy = y + g.off[o][1], zz = z + g.off[o][2];
        if (xx < 0 || xx >= g.nx || yy < 0 || yy >= g.ny || zz < 0 || zz >= g.nz) continue;         // a neighbour never wraps across a row or a plane
        const int64_t j = ((int64_t)zz * g.ny + yy) * g.nx + xx;
        if (mask[j]) unite(parent, (int32_t)i, (int32_t)j);
    }
}

// takes part: mask[i] != 0 (lattice) or label[i] != -1 (mesh: a face marked it).  label[i] = root, -1 for the others; bsum[block] = roots in the block
__global__ void __launch_bounds__(CC_BLOCK) k_cc_resolve(int64_t n, const int32_t *__restrict__ parent, const uint8_t *__restrict__ mask, int32_t *__restrict__ label,
                                                         int32_t *__restrict__ bsum)
{
    __shared__ int sh[CC_BLOCK / 64];
    const int64_t i = (int64_t)blockIdx.x * CC_BLOCK + threadIdx.x;
    bool is_root = false;
    if (i < n) {
        int32_t r = -1;
        if (mask ? mask[i] != 0 : label[i] != -1) {
            r = (int32_t)i;
            for (int32_t p = parent[r]; p != r; p = parent[r]) r = p;          // p < r: bounded by i
        }
        label[i] = r;
        is_root = r == (int32_t)i;
    }
    const int total = block_count<CC_BLOCK>(is_root, sh);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ void __launch_bounds__(CC_BLOCK) k_cc_rank(int64_t n, const int32_t *__restrict__ label, const int32_t *__restrict__ bsum, int32_t *__restrict__ rank)
{
    __shared__ int sh[CC_BLOCK / 64];
    const int64_t i = (int64_t)blockIdx.x * CC_BLOCK + threadIdx.x;
    const bool is_root = i < n && label[i] == (int32_t)i;
    int total;
    const int before = block_rank<CC_BLOCK>(is_root, sh, total);
    if (is_root) rank[i] = bsum[blockIdx.x] + before;
}

__global__ void __launch_bounds__(CC_BLOCK) k_cc_label(int64_t n, const int32_t *__restrict__ rank, int32_t *__restrict__ label)
{
    const int64_t i = (int64_t)blockIdx.x * CC_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t r = label[i];
    if (r >= 0) label[i] = rank[r];
}

struct CcWs {
    int64_t *header;         // [0] K, [1] vertex indices out of range
    int32_t *parent;         // [n]; the roots' ranks after k_cc_rank
    int32_t *bsum;           // [nb]
    int64_t nb;
};
CcWs cc_layout(Bump &b, int64_t n)
{
    CcWs w;
    w.nb = ceil_div(n, CC_BLOCK);
    w.header = b.take<int64_t>(2);
    w.parent = b.take<int32_t>((size_t)n);
    w.bsum = b.take<int32_t>((size_t)w.nb);
    return w;
}

// everything after the union launch, and the read-back of the header (synchronises the stream)
int cc_finish(const CcWs &w, int64_t n, const uint8_t *mask, int32_t *label, int64_t h[2], hipStream_t st)
{
    const dim3 grid((unsigned)w.nb), block(CC_BLOCK);
    hipLaunchKernelGGL(k_cc_resolve, grid, block, 0, st, n, w.parent, mask, label, w.bsum);
    NRF_LAUNCH_CHECK();
    hipLaunchKernelGGL((k_totals_scan<int32_t, int64_t>), dim3(1), dim3(SCAN_BLOCK), 0, st, w.nb, w.bsum, w.header);          // K <= n < 2^31; header[0] = K
    NRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cc_rank, grid, block, 0, st, n, label, w.bsum, w.parent);
    NRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cc_label, grid, block, 0, st, n, w.parent, label);
    NRF_LAUNCH_CHECK();
    NRF_HIP(hipMemcpyAsync(h, w.header, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    NRF_HIP(hipStreamSynchronize(st));
    return NRF_OK;
}

}  // namespace

}  // namespace nrf

using namespace nrf;

extern "C" {

size_t nrf_mesh_components_workspace_bytes(int64_t n_verts, int64_t n_tris)
{
    (void)n_tris;
    if (n_verts < 0 || n_verts > INT32_MAX) return 0;
    return measure([&](Bump &b) { cc_layout(b, n_verts); });
}

int nrf_mesh_components(const int32_t *d_faces, int64_t n_verts, int64_t n_tris, int32_t *d_labels, int64_t *n_components, void *d_workspace, size_t workspace_bytes,
                        void *stream)
{
    NRF_CHECK_ARG(n_components, "nrf_mesh_components: null n_components");
    NRF_CHECK_ARG(n_verts >= 0 && n_tris >= 0 && n_verts <= INT32_MAX && n_tris <= INT32_MAX, "nrf_mesh_components: %lld vertices / %lld faces outside [0, 2^31)",
                  (long long)n_verts, (long long)n_tris);
    *n_components = 0;
    if (n_verts == 0) {
        NRF_CHECK_ARG(n_tris == 0, "nrf_mesh_components: %lld face(s) over no vertices", (long long)n_tris);
        return NRF_OK;
    }
    NRF_CHECK_ARG(d_labels && d_workspace && (d_faces || n_tris == 0), "nrf_mesh_components: null faces, labels or workspace");
    Bump bump(d_workspace, workspace_bytes);
    const CcWs w = cc_layout(bump, n_verts);
    NRF_TRY(ws_check(bump, nrf_mesh_components_workspace_bytes(n_verts, n_tris), "nrf_mesh_components"));
    hipStream_t st = as_stream(stream);
    NRF_HIP(hipMemsetAsync(w.header, 0, 2 * sizeof(int64_t), st));
    hipLaunchKernelGGL(k_cc_init, dim3((unsigned)w.nb), dim3(CC_BLOCK), 0, st, n_verts, w.parent, d_labels);
    NRF_LAUNCH_CHECK();
    if (n_tris > 0) {
        hipLaunchKernelGGL(k_cc_union_faces, dim3((unsigned)ceil_div(n_tris, CC_BLOCK)), dim3(CC_BLOCK), 0, st, d_faces, n_tris, (int32_t)n_verts, w.parent, d_labels,
                           reinterpret_cast<unsigned long long *>(w.header + 1));
        NRF_LAUNCH_CHECK();
    }
    int64_t h[2] = {0, 0};
    NRF_TRY(cc_finish(w, n_verts, nullptr, d_labels, h, st));
    NRF_CHECK_ARG(h[1] == 0, "nrf_mesh_components: %lld vertex index(es) outside [0, %lld); their faces were skipped and the labels are unspecified", (long long)h[1],
                  (long long)n_verts);
    *n_components = h[0];
    return NRF_OK;
}

size_t nrf_lattice_components_workspace_bytes(int nx, int ny, int nz)
{
    if (nx < 1 || ny < 1 || nz < 1 || (int64_t)nx * ny > INT32_MAX || (int64_t)nx * ny * nz > INT32_MAX) return 0;
    return measure([&](Bump &b) { cc_layout(b, (int64_t)nx * ny * nz); });
}

int nrf_lattice_components(const uint8_t *d_mask, int nx, int ny, int nz, int connectivity, int32_t *d_labels, int64_t *n_components, void *d_workspace,
                           size_t workspace_bytes, void *stream)
{
    NRF_CHECK_ARG(d_mask && d_labels && n_components && d_workspace, "nrf_lattice_components: null pointer");
    NRF_CHECK_ARG(nx >= 1 && ny >= 1 && nz >= 1 && (int64_t)nx * ny <= INT32_MAX && (int64_t)nx * ny * nz <= INT32_MAX,
                  "nrf_lattice_components: lattice %d x %d x %d must have every dimension >= 1 and fewer than 2^31 points", nx, ny, nz);
    NRF_CHECK_ARG(connectivity == 6 || connectivity == 14 || connectivity == 26, "nrf_lattice_components: connectivity must be 6, 14 or 26 (got %d)", connectivity);
    *n_components = 0;
    Lattice g{};
    g.nx = nx; g.ny = ny; g.nz = nz;
    g.n = (int64_t)nx * ny * nz;
    for (int dz = 0; dz <= 1; dz++)
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++) {
                const bool forward = dz > 0 || (dz == 0 && (dy > 0 || (dy == 0 && dx > 0)));           // one of each +-pair
                const int taxi = (dx != 0) + (dy != 0) + (dz != 0);
                const bool kuhn = dx >= 0 && dy >= 0;                                                  // with dz >= 0: the 7 edge types of the isosurface's split
                if (!forward || (connectivity == 6 && taxi != 1) || (connectivity == 14 && !kuhn)) continue;
                g.off[g.n_offsets][0] = (int8_t)dx; g.off[g.n_offsets][1] = (int8_t)dy; g.off[g.n_offsets][2] = (int8_t)dz;
                g.n_offsets++;
            }
    Bump bump(d_workspace, workspace_bytes);
    const CcWs w = cc_layout(bump, g.n);
    NRF_TRY(ws_check(bump, nrf_lattice_components_workspace_bytes(nx, ny, nz), "nrf_lattice_components"));
    hipStream_t st = as_stream(stream);
    NRF_HIP(hipMemsetAsync(w.header, 0, 2 * sizeof(int64_t), st));
    hipLaunchKernelGGL(k_cc_init, dim3((unsigned)w.nb), dim3(CC_BLOCK), 0, st, g.n, w.parent, (int32_t *)nullptr);
    NRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cc_union_lattice, dim3((unsigned)w.nb), dim3(CC_BLOCK), 0, st, g, d_mask, w.parent);
    NRF_LAUNCH_CHECK();
    int64_t h[2] = {0, 0};
    NRF_TRY(cc_finish(w, g.n, d_mask, d_labels, h, st));
    *n_components = h[0];
    return NRF_OK;
}

}  // extern "C"
