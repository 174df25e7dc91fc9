// mesh.hip -- geometry out of a trained scene: the density lattice (nrf_density_grid) and its isosurface (nrf_isosurface_*).  The reference has no mesh export;
// the contract is stated in include/nerfpp_hip.h and restated in numpy by tests/mesh_ref.py, which the GPU tests compare with bit for bit.
//
// Density lattice.  Slabs of lattice points in linear order: k_lattice_points writes P(i, j, k) of the slab to the workspace, renderer_density (render.hip) runs the
// coarse pass's exact-fp32 sigma kernels on them straight into the caller's grid.  A value depends on its point alone, so slabs change nothing.
//
// Isosurface: marching tetrahedra on the Kuhn split (6 tetrahedra per cell, all sharing the cell's (0,0,0)-(1,1,1) diagonal).  Five launches, four of them one thread per
// lattice point in blocks of ISO_BLOCK:
//   k_iso_classify   7-bit crossing mask of the edges starting at the point, triangle count of the cell whose min corner it is (<= 12), non-finite count;
//                    per-block totals of both counts
//   k_totals_scan    (scan.h; once for the vertices, once for the faces) one workgroup: exclusive int64 scan of the per-block totals (the totals of the whole
//                    lattice land in the workspace header)
//   k_iso_vertices   block-local exclusive scan of popcount(mask) + the block's offset = the point's first vertex id (kept: the faces need it); vertex and normal
//   k_iso_faces      block-local exclusive scan of the triangle counts + the block's offset = the cell's first triangle; a vertex id is its edge origin's first
//                    id + popcount of the origin's lower mask bits
// Every output position comes from an integer prefix sum: no atomics decide an order, so two runs give the same arrays.
#include "common.h"
#include "scan.h"
#include "workspace.h"

#include <climits>
#include <cmath>

namespace nrf {

namespace {

constexpr int ISO_BLOCK = 256;

// edge type t starts at corner 0 of a cell and ends at corner EDGE_END[t] (corner bits: 1 = +x, 2 = +y, 4 = +z)
__constant__ const uint8_t EDGE_END[7] = {1, 2, 4, 3, 5, 6, 7};
// type of the edge between two corners whose bits differ by d (d = 1..7)
__constant__ const int8_t TYPE_OF_DIFF[8] = {-1, 0, 1, 3, 2, 4, 5, 6};
// the 6 axis permutations xyz, xzy, yxz, yzx, zxy, zyx as the two middle corners of their chain (c, c + e_p0, c + e_p0 + e_p1, c + (1,1,1)) and their parity
__constant__ const uint8_t CHAIN1[6] = {1, 1, 2, 2, 4, 4};
__constant__ const uint8_t CHAIN2[6] = {3, 5, 3, 6, 5, 6};
__constant__ const uint8_t PERM_ODD[6] = {0, 1, 1, 0, 0, 1};

struct Grid {
    int nx, ny, nz;
    int64_t n;               // nx * ny * nz
    float bmin[3], step[3];
};

__device__ __forceinline__ void coords(const Grid &g, int64_t i, int &x, int &y, int &z)
{
    const int64_t yz = i / g.nx;
    x = (int)(i - yz * g.nx);
    y = (int)(yz % g.ny);
    z = (int)(yz / g.ny);
}

__device__ __forceinline__ float lattice_coord(const Grid &g, int axis, int i) { return g.bmin[axis] + (float)i * g.step[axis]; }

// inside bits of the 8 corners of the cell at (x, y, z) (corners outside the lattice: 0) and which corners exist
__device__ __forceinline__ void cell_corners(const Grid &g, const float *__restrict__ f, int64_t i, int x, int y, int z, float iso, unsigned &inside, unsigned &exists)
{
    inside = 0; exists = 0;
    const int64_t sy = g.nx, sz = (int64_t)g.nx * g.ny;
#pragma unroll
    for (int o = 0; o < 8; o++) {
        const int ox = o & 1, oy = (o >> 1) & 1, oz = o >> 2;
        if (x + ox < g.nx && y + oy < g.ny && z + oz < g.nz) {
            exists |= 1u << o;
            if (f[i + ox + oy * sy + oz * sz] > iso) inside |= 1u << o;
        }
    }
}

// 4-bit inside mask of tetrahedron `perm` (bit j = chain corner j)
__device__ __forceinline__ unsigned tet_mask(unsigned inside, int perm)
{
    return (inside & 1u) | ((inside >> CHAIN1[perm] & 1u) << 1) | ((inside >> CHAIN2[perm] & 1u) << 2) | ((inside >> 7 & 1u) << 3);
}

__global__ void __launch_bounds__(ISO_BLOCK) k_iso_classify(Grid g, const float *__restrict__ f, float iso, uint8_t *__restrict__ vmask, uint8_t *__restrict__ tcount,
                                                            int64_t *__restrict__ bsum_v, int64_t *__restrict__ bsum_f, unsigned long long *__restrict__ nonfinite)
{
    __shared__ int sh[ISO_BLOCK / 64];
    const int64_t i = (int64_t)blockIdx.x * ISO_BLOCK + threadIdx.x;
    int m = 0, tc = 0, bad = 0;
    if (i < g.n) {
        int x, y, z;
        coords(g, i, x, y, z);
        bad = !isfinite(f[i]);
        unsigned inside, exists;
        cell_corners(g, f, i, x, y, z, iso, inside, exists);
#pragma unroll
        for (int t = 0; t < 7; t++)
            if ((exists >> EDGE_END[t] & 1u) && (inside >> EDGE_END[t] & 1u) != (inside & 1u)) m |= 1 << t;
        if (exists == 0xffu) {
#pragma unroll
            for (int p = 0; p < 6; p++) {
                const int pc = __popc(tet_mask(inside, p));
                tc += pc == 2 ? 2 : (pc & 1);
            }
        }
        vmask[i] = (uint8_t)m;
        tcount[i] = (uint8_t)tc;
    }
    const int tv = block_sum<int, ISO_BLOCK>(__popc(m), sh), tf = block_sum<int, ISO_BLOCK>(tc, sh), tb = block_count<ISO_BLOCK>(bad, sh);
    if (threadIdx.x == 0) {
        bsum_v[blockIdx.x] = tv;
        bsum_f[blockIdx.x] = tf;
        if (tb) atomicAdd(nonfinite, (unsigned long long)tb);        // a count: its value does not depend on the order of the additions
    }
}

// central difference of the lattice along one axis, one-sided at the border
__device__ __forceinline__ float lattice_grad(const Grid &g, const float *__restrict__ f, int64_t i, int axis, int c, int n, int64_t stride)
{
    const int lo = c > 0 ? c - 1 : c, hi = c < n - 1 ? c + 1 : c;
    return (f[i + (hi - c) * stride] - f[i + (lo - c) * stride]) / (lattice_coord(g, axis, hi) - lattice_coord(g, axis, lo));
}

__device__ __forceinline__ void lattice_grad3(const Grid &g, const float *__restrict__ f, int64_t i, int x, int y, int z, float gr[3])
{
    gr[0] = lattice_grad(g, f, i, 0, x, g.nx, 1);
    gr[1] = lattice_grad(g, f, i, 1, y, g.ny, g.nx);
    gr[2] = lattice_grad(g, f, i, 2, z, g.nz, (int64_t)g.nx * g.ny);
}

__global__ void __launch_bounds__(ISO_BLOCK) k_iso_vertices(Grid g, const float *__restrict__ f, float iso, const uint8_t *__restrict__ vmask,
                                                            const int64_t *__restrict__ bsum_v, int32_t *__restrict__ voff, float *__restrict__ verts,
                                                            float *__restrict__ normals)
{
    __shared__ int sh[ISO_BLOCK];
    const int64_t i = (int64_t)blockIdx.x * ISO_BLOCK + threadIdx.x;
    const int m = i < g.n ? vmask[i] : 0;
    int total;
    const int64_t base = bsum_v[blockIdx.x] + block_exclusive_scan<int, ISO_BLOCK>(__popc(m), sh, total);
    if (i >= g.n) return;
    voff[i] = (int32_t)base;
    if (!m) return;
    int x, y, z;
    coords(g, i, x, y, z);
    const float fa = f[i];
    const float pa[3] = {lattice_coord(g, 0, x), lattice_coord(g, 1, y), lattice_coord(g, 2, z)};
    float ga[3] = {0.0f, 0.0f, 0.0f};
    if (normals) lattice_grad3(g, f, i, x, y, z, ga);
    int64_t v = base;
    for (int t = 0; t < 7; t++) {
        if (!(m >> t & 1)) continue;
        const int dx = EDGE_END[t] & 1, dy = (EDGE_END[t] >> 1) & 1, dz = EDGE_END[t] >> 2;
        const int64_t j = i + dx + dy * (int64_t)g.nx + dz * (int64_t)g.nx * g.ny;
        const float fb = f[j];
        const float tt = (iso - fa) / (fb - fa);
        const float pb[3] = {lattice_coord(g, 0, x + dx), lattice_coord(g, 1, y + dy), lattice_coord(g, 2, z + dz)};
#pragma unroll
        for (int a = 0; a < 3; a++) verts[v * 3 + a] = pa[a] + tt * (pb[a] - pa[a]);
        if (normals) {
            float gb[3], gv[3];
            lattice_grad3(g, f, j, x + dx, y + dy, z + dz, gb);
#pragma unroll
            for (int a = 0; a < 3; a++) gv[a] = ga[a] + tt * (gb[a] - ga[a]);
            const float len = sqrtf(gv[0] * gv[0] + gv[1] * gv[1] + gv[2] * gv[2]);
#pragma unroll
            for (int a = 0; a < 3; a++) normals[v * 3 + a] = len > 0.0f ? -gv[a] / len : 0.0f;
        }
        v++;
    }
}

__global__ void __launch_bounds__(ISO_BLOCK) k_iso_faces(Grid g, const float *__restrict__ f, float iso, const uint8_t *__restrict__ vmask, const int32_t *__restrict__ voff,
                                                         const uint8_t *__restrict__ tcount, const int64_t *__restrict__ bsum_f, int32_t *__restrict__ faces)
{
    __shared__ int sh[ISO_BLOCK];
    const int64_t i = (int64_t)blockIdx.x * ISO_BLOCK + threadIdx.x;
    const int tc = i < g.n ? tcount[i] : 0;
    int total;
    const int64_t base = bsum_f[blockIdx.x] + block_exclusive_scan<int, ISO_BLOCK>(tc, sh, total);
    if (!tc) return;
    int x, y, z;
    coords(g, i, x, y, z);
    unsigned inside, exists;
    cell_corners(g, f, i, x, y, z, iso, inside, exists);
    const int64_t sy = g.nx, sz = (int64_t)g.nx * g.ny;
    // vertex id of the edge between cell corners lo and hi (lo's bits a subset of hi's: chain order)
    auto edge_vertex = [&](unsigned lo, unsigned hi) -> int32_t {
        const int64_t a = i + (lo & 1) + (lo >> 1 & 1) * sy + (lo >> 2) * sz;
        const int t = TYPE_OF_DIFF[lo ^ hi];
        return voff[a] + __popc(vmask[a] & ((1u << t) - 1u));
    };
    int64_t tri = base;
    auto put = [&](int32_t a, int32_t b, int32_t c, bool flip) {
        faces[tri * 3 + 0] = a;
        faces[tri * 3 + 1] = flip ? c : b;
        faces[tri * 3 + 2] = flip ? b : c;
        tri++;
    };
    for (int p = 0; p < 6; p++) {
        const unsigned chain[4] = {0u, CHAIN1[p], CHAIN2[p], 7u};
        const unsigned tm = tet_mask(inside, p);
        const int pc = __popc(tm);
        if (pc == 0 || pc == 4) continue;
        // winding: a positively oriented tetrahedron (even permutation) has its triangles counter-clockwise seen from outside when the odd corner k sits at an even
        // chain position and is inside, or at an odd one and is outside; for two inside corners {a, b} when a + b is odd.  An odd permutation reverses all of it.
        if (pc & 1) {
            const int k = pc == 1 ? __ffs(tm) - 1 : __ffs(~tm & 15u) - 1;
            int32_t e[3];
            int n = 0;
            for (int j = 0; j < 4; j++)
                if (j != k) e[n++] = j < k ? edge_vertex(chain[j], chain[k]) : edge_vertex(chain[k], chain[j]);
            put(e[0], e[1], e[2], ((k & 1) ^ (pc == 3) ^ PERM_ODD[p]) != 0);
        } else {
            int in[2], out[2], ni = 0, no = 0;
            for (int j = 0; j < 4; j++) {
                if (tm >> j & 1) in[ni++] = j;
                else out[no++] = j;
            }
            const int a = in[0], b = in[1], c = out[0], d = out[1];
            auto ev = [&](int u, int w) { return u < w ? edge_vertex(chain[u], chain[w]) : edge_vertex(chain[w], chain[u]); };
            const int32_t ac = ev(a, c), ad = ev(a, d), bd = ev(b, d), bc = ev(b, c);
            const bool flip = (((a + b) & 1) == 0) ^ (PERM_ODD[p] != 0);
            put(ac, ad, bd, flip);
            put(ac, bd, bc, flip);
        }
    }
}

__global__ void k_lattice_points(Grid g, int64_t first, int64_t count, float *__restrict__ pts)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= count) return;
    int x, y, z;
    coords(g, first + q, x, y, z);
    pts[q * 3 + 0] = lattice_coord(g, 0, x);
    pts[q * 3 + 1] = lattice_coord(g, 1, y);
    pts[q * 3 + 2] = lattice_coord(g, 2, z);
}

constexpr int64_t DEFAULT_SLAB = (int64_t)1 << 22;
constexpr int64_t MAX_SLAB = (int64_t)1 << 30;
constexpr int64_t MAX_LATTICE = (int64_t)1 << 36;            // 64 G points: far beyond any device's memory, keeps block counts within the launch grid

// the grid of a call; bbox / dims checked (message names the call)
int make_grid(const char *who, const float *bbox, int nx, int ny, int nz, Grid &g)
{
    NRF_CHECK_ARG(nx >= 2 && ny >= 2 && nz >= 2, "%s: every lattice dimension must be >= 2 (got %d x %d x %d)", who, nx, ny, nz);
    NRF_CHECK_ARG(bbox, "%s: null bbox", who);
    for (int a = 0; a < 3; a++)
        NRF_CHECK_ARG(std::isfinite(bbox[a]) && std::isfinite(bbox[3 + a]) && bbox[3 + a] > bbox[a], "%s: empty, inverted or non-finite box on axis %d ([%g, %g])", who, a,
                      (double)bbox[a], (double)bbox[3 + a]);
    g.nx = nx; g.ny = ny; g.nz = nz;
    g.n = (int64_t)nx * ny * nz;
    NRF_CHECK_ARG(g.n <= MAX_LATTICE, "%s: lattice of %lld points is too large", who, (long long)g.n);
    const int n[3] = {nx, ny, nz};
    for (int a = 0; a < 3; a++) {
        g.bmin[a] = bbox[a];
        g.step[a] = (bbox[3 + a] - bbox[a]) / (float)(n[a] - 1);      // fp32, one rounding per operation
    }
    return NRF_OK;
}

struct IsoWs {
    int64_t *header;         // [0] V, [1] F, [2] non-finite count
    uint8_t *vmask, *tcount;
    int32_t *voff;
    int64_t *bsum_v, *bsum_f;
    int64_t nb;
    size_t bytes;
};

IsoWs iso_layout(void *ws, int64_t n)
{
    IsoWs w{};
    size_t off = 0;
    char *base = static_cast<char *>(ws);
    auto take = [&](size_t b) { char *p = base ? base + off : nullptr; off += align_up(b, 256); return p; };
    w.nb = ceil_div(n, ISO_BLOCK);
    w.header = reinterpret_cast<int64_t *>(take(4 * sizeof(int64_t)));
    w.vmask = reinterpret_cast<uint8_t *>(take((size_t)n));
    w.tcount = reinterpret_cast<uint8_t *>(take((size_t)n));
    w.voff = reinterpret_cast<int32_t *>(take((size_t)n * sizeof(int32_t)));
    w.bsum_v = reinterpret_cast<int64_t *>(take((size_t)w.nb * sizeof(int64_t)));
    w.bsum_f = reinterpret_cast<int64_t *>(take((size_t)w.nb * sizeof(int64_t)));
    w.bytes = off;
    return w;
}

// nrf_density_grid's workspace: one slab of lattice points and renderer_density's own workspace for them
struct GridWs {
    int64_t slab;
    float *pts;
    void *density;
    size_t density_bytes;
};
GridWs grid_layout(Bump &b, const nrf_renderer *r, int64_t n, int64_t slab_points)
{
    GridWs w;
    w.slab = slab_points > 0 ? slab_points : DEFAULT_SLAB;
    if (w.slab > MAX_SLAB) w.slab = MAX_SLAB;
    if (w.slab > n) w.slab = n;
    w.pts = b.take<float>((size_t)w.slab * 3);
    w.density_bytes = renderer_density_ws_bytes(r, w.slab);
    w.density = b.take<char>(w.density_bytes);
    return w;
}

}  // namespace

}  // namespace nrf

using namespace nrf;

extern "C" {

size_t nrf_density_grid_workspace_bytes(const nrf_renderer *r, int nx, int ny, int nz, int64_t slab_points)
{
    if (!r || nx < 2 || ny < 2 || nz < 2) return 0;
    return measure([&](Bump &b) { grid_layout(b, r, (int64_t)nx * ny * nz, slab_points); });
}

int nrf_density_grid(const nrf_renderer *r, const float *bbox, int nx, int ny, int nz, float *d_sigma, int64_t slab_points, void *d_workspace, size_t workspace_bytes,
                     void *stream)
{
    NRF_CHECK_ARG(r, "nrf_density_grid: null renderer");
    NRF_CHECK_ARG(d_sigma && d_workspace, "nrf_density_grid: null output or workspace");
    NRF_CHECK_ARG(slab_points <= MAX_SLAB, "nrf_density_grid: slab_points %lld above 2^30", (long long)slab_points);
    Grid g;
    NRF_TRY(make_grid("nrf_density_grid", bbox, nx, ny, nz, g));
    Bump bump(d_workspace, workspace_bytes);
    const GridWs w = grid_layout(bump, r, g.n, slab_points);
    NRF_TRY(ws_check(bump, nrf_density_grid_workspace_bytes(r, nx, ny, nz, slab_points), "nrf_density_grid"));
    const int64_t slab = w.slab;
    hipStream_t st = as_stream(stream);
    float *pts = w.pts;
    for (int64_t first = 0; first < g.n; first += slab) {
        const int64_t cnt = g.n - first < slab ? g.n - first : slab;
        hipLaunchKernelGGL(k_lattice_points, dim3((unsigned)ceil_div(cnt, 256)), dim3(256), 0, st, g, first, cnt, pts);
        NRF_LAUNCH_CHECK();
        NRF_TRY(renderer_density(r, pts, cnt, d_sigma + first, w.density, w.density_bytes, st));
    }
    return NRF_OK;
}

size_t nrf_isosurface_workspace_bytes(int nx, int ny, int nz)
{
    if (nx < 2 || ny < 2 || nz < 2) return 0;
    return iso_layout(nullptr, (int64_t)nx * ny * nz).bytes;
}

int nrf_isosurface_count(const float *d_sigma, int nx, int ny, int nz, const float *bbox, float iso, int64_t *n_verts, int64_t *n_tris, int64_t *n_nonfinite,
                         void *d_workspace, size_t workspace_bytes, void *stream)
{
    NRF_CHECK_ARG(d_sigma && d_workspace && n_verts && n_tris, "nrf_isosurface_count: null pointer");
    NRF_CHECK_ARG(std::isfinite(iso), "nrf_isosurface_count: iso level %g is not finite", (double)iso);
    Grid g;
    NRF_TRY(make_grid("nrf_isosurface_count", bbox, nx, ny, nz, g));
    const IsoWs w = iso_layout(d_workspace, g.n);
    if (workspace_bytes < w.bytes) { set_error("nrf_isosurface_count: workspace %zu < %zu bytes", workspace_bytes, w.bytes); return NRF_ERR_WORKSPACE; }
    hipStream_t st = as_stream(stream);
    NRF_HIP(hipMemsetAsync(w.header, 0, 4 * sizeof(int64_t), st));
    hipLaunchKernelGGL(k_iso_classify, dim3((unsigned)w.nb), dim3(ISO_BLOCK), 0, st, g, d_sigma, iso, w.vmask, w.tcount, w.bsum_v, w.bsum_f,
                       reinterpret_cast<unsigned long long *>(w.header + 2));
    NRF_LAUNCH_CHECK();
    hipLaunchKernelGGL((k_totals_scan<int64_t, int64_t>), dim3(1), dim3(SCAN_BLOCK), 0, st, w.nb, w.bsum_v, w.header + 0);          // header[0] = V
    NRF_LAUNCH_CHECK();
    hipLaunchKernelGGL((k_totals_scan<int64_t, int64_t>), dim3(1), dim3(SCAN_BLOCK), 0, st, w.nb, w.bsum_f, w.header + 1);          // header[1] = F
    NRF_LAUNCH_CHECK();
    int64_t h[4] = {0, 0, 0, 0};
    NRF_HIP(hipMemcpyAsync(h, w.header, sizeof(h), hipMemcpyDeviceToHost, st));
    NRF_HIP(hipStreamSynchronize(st));
    *n_verts = h[0];
    *n_tris = h[1];
    if (n_nonfinite) *n_nonfinite = h[2];
    NRF_CHECK_ARG(h[0] <= INT32_MAX && h[1] <= INT32_MAX, "nrf_isosurface_count: %lld vertices / %lld triangles exceed the int32 range of the face indices",
                  (long long)h[0], (long long)h[1]);
    return NRF_OK;
}

int nrf_isosurface_emit(const float *d_sigma, int nx, int ny, int nz, const float *bbox, float iso, float *d_verts, int32_t *d_faces, float *d_normals,
                        int64_t n_verts, int64_t n_tris, void *d_workspace, size_t workspace_bytes, void *stream)
{
    NRF_CHECK_ARG(d_sigma && d_workspace, "nrf_isosurface_emit: null lattice or workspace");
    NRF_CHECK_ARG(std::isfinite(iso), "nrf_isosurface_emit: iso level %g is not finite", (double)iso);
    NRF_CHECK_ARG(n_verts >= 0 && n_tris >= 0 && n_verts <= INT32_MAX && n_tris <= INT32_MAX, "nrf_isosurface_emit: counts %lld / %lld outside the int32 range",
                  (long long)n_verts, (long long)n_tris);
    NRF_CHECK_ARG((d_verts || n_verts == 0) && (d_faces || n_tris == 0), "nrf_isosurface_emit: null vertex or face output");
    Grid g;
    NRF_TRY(make_grid("nrf_isosurface_emit", bbox, nx, ny, nz, g));
    const IsoWs w = iso_layout(d_workspace, g.n);
    if (workspace_bytes < w.bytes) { set_error("nrf_isosurface_emit: workspace %zu < %zu bytes", workspace_bytes, w.bytes); return NRF_ERR_WORKSPACE; }
    hipStream_t st = as_stream(stream);
    int64_t h[4] = {0, 0, 0, 0};
    NRF_HIP(hipMemcpyAsync(h, w.header, sizeof(h), hipMemcpyDeviceToHost, st));
    NRF_HIP(hipStreamSynchronize(st));
    if (h[2] != 0) {
        set_error("nrf_isosurface_emit: the lattice holds %lld non-finite value(s)", (long long)h[2]);
        return NRF_ERR_NONFINITE;
    }
    NRF_CHECK_ARG(h[0] == n_verts && h[1] == n_tris, "nrf_isosurface_emit: counts %lld / %lld differ from the count call's %lld / %lld (same lattice, iso and workspace?)",
                  (long long)n_verts, (long long)n_tris, (long long)h[0], (long long)h[1]);
    hipLaunchKernelGGL(k_iso_vertices, dim3((unsigned)w.nb), dim3(ISO_BLOCK), 0, st, g, d_sigma, iso, w.vmask, w.bsum_v, w.voff, d_verts, d_normals);
    NRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_iso_faces, dim3((unsigned)w.nb), dim3(ISO_BLOCK), 0, st, g, d_sigma, iso, w.vmask, w.voff, w.tcount, w.bsum_f, d_faces);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

}  // extern "C"
