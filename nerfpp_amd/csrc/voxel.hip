// voxel.hip -- scan conversion of a triangle list onto the lattice of nrf_density_grid (nrf_mesh_voxelize): an integer winding number per lattice point, a truncated
// signed distance with the nearest face's index, and so the SDF lattice nrf_isosurface_* takes.  The reference has no voxeliser; the contract is stated in
// include/nerfpp_hip.h and restated in numpy by tests/voxel_ref.py, which the GPU tests compare with bit for bit.
//
// Both passes are scatters, as the rasteriser's is: work in proportion to the faces and to what they cover, not to the lattice.
//   k_vox_init      one lane per lattice point: delta = 0 and, with a distance pass, key = NN_NONE
//   k_vox_project   one lane per vertex: step 1 of the header into a 16-byte record {X, Y, gz, ok}, so a face gathers 16 B per corner and a vertex pays its
//                   divisions once, not once per face that uses it
//   k_vox_faces     a fixed grid strides the face list, one lane per face: class (cm_face: bad / non-finite; then clipped), the columns of the winding pass and
//                   the dilated lattice box of the distance pass.  A face scans what holds at most NRF_VOXEL_WIDE_COLUMNS / _POINTS entries itself and is appended
//                   to the wide list of the other kind otherwise (scan.h's wave_append).  Every lane counts its faces by class
//                   in registers: three atomic adds on d_stats per WORKGROUP (DESIGN 8k has what one add per wave cost the rasteriser)
//   k_vox_wide      a fixed grid of workgroups strides both wide lists (their lengths are read on the device: the host never sees them); the 256 lanes of a workgroup
//                   stride the columns or the lattice points of one face, so no lane's time grows with a face's size
//   k_vox_finish    one lane per column, lanes along x so every level is a coalesced row: top-down, the suffix sum of delta is the winding; the key gives distance
//                   and face, the rule gives the sign.  The volume is read once
// The winding pass adds s = +-1 to delta[kc][j][i] by an integer atomic add; the distance pass lowers reduce.h's packed key (d2, face) by key_lower.
// Integer sums and minima do not depend on the order their terms arrive in: neither scheduling nor the order of the face list reaches the result.  d2 >= 0, so its
// bit pattern orders as the value does.  Kernel boundaries make delta and the keys visible to the finish pass.
// Coverage is decided in int64 (exact; edge_fn.h's edge_cover, the rasteriser's); every edge value is e(0, 0) + i * step_x + j * step_y, which in integers is the header's E_ab(p) whatever the visiting order.
// vx_column and vx_point are the one copy of steps 2-5 and 8: the face kernel and the wide kernel call them, so the bits cannot differ between the two.
// Every loop is bounded by a clamped range or by a count; no kernel waits on another workgroup.
#include "edge_fn.h"
#include "scan.h"
#include "workspace.h"
#include "face_grid.h"

#include <climits>
#include <cmath>

namespace nrf {

namespace {

constexpr int VX_BLOCK = 256;
constexpr int VX_FACE_GRID = 768;        // workgroups of k_vox_faces, striding the face list: 3 per CU, what its 155 registers admit
constexpr int VX_WIDE_GRID = 1024;       // workgroups of k_vox_wide: 4 per CU

struct VxLat {
    int n[3];
    float bmin[3], step[3];
    float trunc, t2;                 // t2 = fl(trunc * trunc)
};

struct VoxWs {
    int4 *vert;                      // [V] {X, Y, float_bits(gz), ok}
    int32_t *wide_col;               // [F] the faces whose columns the wide kernel rasterises, in any order
    int32_t *wide_pts;               // [F] the faces whose lattice box the wide kernel scans
    uint32_t *n_wide;                // [2] the two lengths
    int32_t *delta;                  // [nz][ny][nx]
    unsigned long long *key;         // [nz][ny][nx]; last, and only with a distance output
};

VoxWs vox_layout(Bump &b, int64_t n_verts, int64_t n_faces, int nx, int ny, int nz, bool with_dist)
{
    VoxWs s;
    const size_t n_pts = (size_t)nx * ny * nz;
    s.vert = b.take<int4>((size_t)n_verts);
    s.wide_col = b.take<int32_t>((size_t)n_faces);
    s.wide_pts = b.take<int32_t>((size_t)n_faces);
    s.n_wide = b.take<uint32_t>(2);
    s.delta = b.take<int32_t>(n_pts);
    s.key = with_dist ? b.take<unsigned long long>(n_pts) : nullptr;
    return s;
}

bool vox_shape_ok(int64_t n_verts, int64_t n_faces, int nx, int ny, int nz)
{
    return n_verts >= 0 && n_verts <= INT32_MAX && n_faces >= 0 && n_faces <= (int64_t)INT32_MAX - 1 && nx >= 2 && ny >= 2 && nz >= 2 &&
           (int64_t)nx * ny * nz <= (int64_t)INT32_MAX;
}

size_t vox_bytes(int64_t n_verts, int64_t n_faces, int nx, int ny, int nz, bool with_dist)
{
    return measure([&](Bump &b) { vox_layout(b, n_verts, n_faces, nx, ny, nz, with_dist); });
}

// a face set up for steps 2-4: the three edge functions as e(0, 0) and their steps per column, already multiplied by s = sign(A); sA = s * A > 0
struct VxTri {
    int64_t e00[3], sx[3], sy[3];
    int64_t sA;
    float gz[3];
    bool tl[3];
    int s;
    int i0, i1, j0, j1;              // step 3's columns and rows (empty where i1 < i0 or j1 < j0)
};

// step 2: A = E_01(v2), and -- for A != 0 -- the face's VxTri.  a, b, c: the corners' records
__device__ __forceinline__ int64_t vx_setup(const int4 &a, const int4 &b, const int4 &c, const VxLat &g, VxTri &t)
{
    const int64_t x[3] = {a.x, b.x, c.x}, y[3] = {a.y, b.y, c.y};
    const int64_t A = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0]);
    const int64_t s = A > 0 ? 1 : -1;
    t.s = (int)s;
    t.sA = s * A;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int ia = (k + 1) % 3, ib = (k + 2) % 3;          // edge k runs v1->v2, v2->v0, v0->v1
        const int64_t dx = s * (x[ib] - x[ia]), dy = s * (y[ib] - y[ia]);
        t.e00[k] = dx * (-y[ia]) - dy * (-x[ia]);              // s * E_ab((0, 0))
        t.sx[k] = -dy * NRF_RASTER_SUBPIXEL;
        t.sy[k] = dx * NRF_RASTER_SUBPIXEL;
        t.tl[k] = dy < 0 || (dy == 0 && dx > 0);
    }
    t.gz[0] = __int_as_float(a.z);
    t.gz[1] = __int_as_float(b.z);
    t.gz[2] = __int_as_float(c.z);
    const int xmin = min(a.x, min(b.x, c.x)), xmax = max(a.x, max(b.x, c.x));
    const int ymin = min(a.y, min(b.y, c.y)), ymax = max(a.y, max(b.y, c.y));
    edge_box(xmin, xmax, ymin, ymax, g.n[0], g.n[1], t.i0, t.i1, t.j0, t.j1);
    return A;
}

// steps 3-5 at column (i, j)
__device__ __forceinline__ void vx_column(const VxTri &t, const VxLat &g, int i, int j, int32_t *__restrict__ delta)
{
    int64_t se[3];
    if (!edge_cover(t.e00, t.sx, t.sy, t.tl, i, j, se)) return;
    float b[3];
    edge_bary(se, t.sA, b);
    const float zc = (b[0] * t.gz[0] + b[1] * t.gz[1]) + b[2] * t.gz[2];
    const float tt = ceilf(zc) - 1.0f;
    if (!(tt >= 0.0f)) return;          // at or below level 0; NaN
    const int kc = (int)fminf(tt, (float)(g.n[2] - 1));
    atomicAdd(delta + ((int64_t)kc * g.n[1] + j) * g.n[0] + i, t.s);
}

// step 7: the face's lattice box; false where it is empty
__device__ __forceinline__ bool vx_box(const float a[3], const float b[3], const float c[3], const VxLat &g, int lo[3], int hi[3])
{
    bool any = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float l = fminf(fminf(a[k], b[k]), c[k]), h = fmaxf(fmaxf(a[k], b[k]), c[k]);
        const float top = (float)(g.n[k] - 1);
        const float fl = floorf(((l - g.trunc) - g.bmin[k]) / g.step[k]) - 1.0f;
        const float fh = ceilf(((h + g.trunc) - g.bmin[k]) / g.step[k]) + 1.0f;
        any = any && fh >= 0.0f && fl <= top;
        lo[k] = (int)fmaxf(fminf(fl, top), 0.0f);          // the inner clamp only keeps the conversion defined where the box is empty
        hi[k] = (int)fminf(fmaxf(fh, 0.0f), top);
    }
    return any;
}

// step 8 at lattice point (i, j, k)
__device__ __forceinline__ void vx_point(const float a[3], const float b[3], const float c[3], const VxLat &g, int i, int j, int k, uint32_t face,
                                         unsigned long long *__restrict__ key)
{
    const float q[3] = {g.bmin[0] + (float)i * g.step[0], g.bmin[1] + (float)j * g.step[1], g.bmin[2] + (float)k * g.step[2]};
    CmHit h;
    cm_closest(q, a, b, c, h);
    if (!(h.d2 <= g.t2)) return;          // a NaN d2 fails the comparison
    key_lower(key + ((int64_t)k * g.n[1] + j) * g.n[0] + i, key_pack(h.d2, face));
}

__global__ void __launch_bounds__(VX_BLOCK) k_vox_init(int64_t n, int32_t *__restrict__ delta, unsigned long long *__restrict__ key)
{
    const int64_t p = (int64_t)blockIdx.x * VX_BLOCK + threadIdx.x;
    if (p >= n) return;
    delta[p] = 0;
    if (key) key[p] = NN_NONE;
}

__global__ void __launch_bounds__(VX_BLOCK) k_vox_project(const float *__restrict__ verts, int64_t n, const VxLat g, int4 *__restrict__ rec)
{
    const int64_t i = (int64_t)blockIdx.x * VX_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float gx = (verts[i * 3 + 0] - g.bmin[0]) / g.step[0];
    const float gy = (verts[i * 3 + 1] - g.bmin[1]) / g.step[1];
    const float gz = (verts[i * 3 + 2] - g.bmin[2]) / g.step[2];
    const bool ok = fabsf(gx) <= (float)NRF_RASTER_GUARD && fabsf(gy) <= (float)NRF_RASTER_GUARD;          // as floats: NaN and +-inf clip
    int4 o;
    o.x = ok ? (int)rintf(gx * (float)NRF_RASTER_SUBPIXEL) : 0;
    o.y = ok ? (int)rintf(gy * (float)NRF_RASTER_SUBPIXEL) : 0;
    o.z = __float_as_int(gz);
    o.w = ok ? 1 : 0;
    rec[i] = o;
}

// the winding set-up of valid face f: 0 with its VxTri, 1 clipped, 2 no projected area
__device__ __forceinline__ int vx_face_tri(const int32_t *__restrict__ faces, int64_t f, const int4 *__restrict__ rec, const VxLat &g, VxTri &t)
{
    const int4 a = rec[faces[f * 3 + 0]], b = rec[faces[f * 3 + 1]], c = rec[faces[f * 3 + 2]];
    if (!(a.w && b.w && c.w)) return 1;
    return vx_setup(a, b, c, g, t) == 0 ? 2 : 0;
}

__global__ void __launch_bounds__(VX_BLOCK) k_vox_faces(const float *__restrict__ verts, int32_t n_verts, const int32_t *__restrict__ faces, int64_t n_faces,
                                                        const int4 *__restrict__ rec, const VxLat g, int32_t *__restrict__ delta, unsigned long long *__restrict__ key,
                                                        int32_t *__restrict__ wide_col, int32_t *__restrict__ wide_pts, uint32_t *__restrict__ n_wide,
                                                        uint32_t *__restrict__ stats)
{
    __shared__ uint32_t s_count[3];
    if (threadIdx.x < 3) s_count[threadIdx.x] = 0;
    __syncthreads();
    uint32_t count[3] = {0, 0, 0};          // this lane's clipped, bad and non-finite faces
    // the bound is the workgroup's: every lane of a wave makes every round (a lane past the last face has no class), so wave_append's ballots see the whole wave
    for (int64_t base = (int64_t)blockIdx.x * VX_BLOCK; base < n_faces; base += (int64_t)gridDim.x * VX_BLOCK) {
        const int64_t f = base + threadIdx.x;
        float a[3], b[3], c[3];
        const int cls = f < n_faces ? cm_face(verts, n_verts, faces, n_faces, f, a, b, c) : -1;
        count[1] += cls == 1;
        count[2] += cls == 2;
        VxTri t;
        const int wcls = cls == 0 ? vx_face_tri(faces, f, rec, g, t) : -1;
        count[0] += wcls == 1;
        const bool cols = wcls == 0 && t.i1 >= t.i0 && t.j1 >= t.j0;
        const bool wide_c = cols && (int64_t)(t.i1 - t.i0 + 1) * (t.j1 - t.j0 + 1) > NRF_VOXEL_WIDE_COLUMNS;
        int lo[3] = {0, 0, 0}, hi[3] = {-1, -1, -1};
        const bool pts = key && cls == 0 && vx_box(a, b, c, g, lo, hi);
        const bool wide_p = pts && (int64_t)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1) > NRF_VOXEL_WIDE_POINTS;
        wave_append(wide_c, (int32_t)f, wide_col, n_wide + 0);          // every face is appended at most once to each list
        wave_append(wide_p, (int32_t)f, wide_pts, n_wide + 1);
        if (cols && !wide_c)
            for (int j = t.j0; j <= t.j1; j++)
                for (int i = t.i0; i <= t.i1; i++) vx_column(t, g, i, j, delta);
        if (pts && !wide_p)
            for (int k = lo[2]; k <= hi[2]; k++)
                for (int j = lo[1]; j <= hi[1]; j++)
                    for (int i = lo[0]; i <= hi[0]; i++) vx_point(a, b, c, g, i, j, k, (uint32_t)f, key);
    }
    if (!stats) return;          // uniform
#pragma unroll
    for (int k = 0; k < 3; k++)
        if (count[k]) atomicAdd(&s_count[k], count[k]);
    __syncthreads();
    if (threadIdx.x < 3 && s_count[threadIdx.x]) atomicAdd(stats + threadIdx.x, s_count[threadIdx.x]);
}

__global__ void __launch_bounds__(VX_BLOCK) k_vox_wide(const float *__restrict__ verts, int32_t n_verts, const int32_t *__restrict__ faces, int64_t n_faces,
                                                       const int4 *__restrict__ rec, const VxLat g, int32_t *__restrict__ delta, unsigned long long *__restrict__ key,
                                                       const int32_t *__restrict__ wide_col, const int32_t *__restrict__ wide_pts, const uint32_t *__restrict__ n_wide)
{
    const uint32_t n_col = n_wide[0], n_pts = key ? n_wide[1] : 0;
    for (uint32_t q = blockIdx.x; q < n_col; q += VX_WIDE_GRID) {
        const int32_t f = wide_col[q];
        VxTri t;
        if (vx_face_tri(faces, f, rec, g, t) != 0) continue;          // never taken: only faces with columns are listed
        const int bw = t.i1 - t.i0 + 1, n = bw * (t.j1 - t.j0 + 1);    // < 2^31: a slice of the lattice
        for (int p = threadIdx.x; p < n; p += VX_BLOCK) {
            const int row = p / bw;
            vx_column(t, g, t.i0 + (p - row * bw), t.j0 + row, delta);
        }
    }
    for (uint32_t q = blockIdx.x; q < n_pts; q += VX_WIDE_GRID) {
        const int32_t f = wide_pts[q];
        float a[3], b[3], c[3];
        int lo[3], hi[3];
        if (cm_face(verts, n_verts, faces, n_faces, f, a, b, c) != 0 || !vx_box(a, b, c, g, lo, hi)) continue;          // never taken: only faces with a box are listed
        const int bw = hi[0] - lo[0] + 1, bh = hi[1] - lo[1] + 1, n = bw * bh * (hi[2] - lo[2] + 1);          // < 2^31: a part of the lattice
        for (int p = threadIdx.x; p < n; p += VX_BLOCK) {
            const int row = p / bw, k = row / bh;
            vx_point(a, b, c, g, lo[0] + (p - row * bw), lo[1] + (row - k * bh), lo[2] + k, (uint32_t)f, key);
        }
    }
}

__global__ void __launch_bounds__(VX_BLOCK) k_vox_finish(const VxLat g, int rule, const int32_t *__restrict__ delta, const unsigned long long *__restrict__ key,
                                                         int32_t *__restrict__ winding, float *__restrict__ sdf, int32_t *__restrict__ face)
{
    const int64_t col = (int64_t)blockIdx.x * VX_BLOCK + threadIdx.x, plane = (int64_t)g.n[0] * g.n[1];
    if (col >= plane) return;
    int32_t w = 0;
    for (int k = g.n[2] - 1; k >= 0; k--) {
        const int64_t p = (int64_t)k * plane + col;
        w += delta[p];
        if (winding) winding[p] = w;
        if (!key) continue;          // uniform
        const unsigned long long v = key[p];
        const bool found = v != NN_NONE;
        if (face) face[p] = found ? key_index(v) : -1;
        if (sdf) {
            const float dist = fminf(found ? sqrtf(key_value(v)) : g.trunc, g.trunc);
            const bool inside = rule == NRF_VOX_NONZERO ? w != 0 : (rule == NRF_VOX_POSITIVE ? w > 0 : (w & 1) != 0);
            sdf[p] = inside ? -dist : dist;
        }
    }
}

}  // namespace

}  // namespace nrf

using namespace nrf;

extern "C" {

size_t nrf_mesh_voxelize_workspace_bytes(int64_t n_verts, int64_t n_faces, int nx, int ny, int nz)
{
    if (!vox_shape_ok(n_verts, n_faces, nx, ny, nz)) return 0;
    return vox_bytes(n_verts, n_faces, nx, ny, nz, true);
}

int nrf_mesh_voxelize(const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, const float *bbox, int nx, int ny, int nz, float trunc, int rule,
                      int32_t *d_winding, float *d_sdf, int32_t *d_face, uint32_t *d_stats, void *d_workspace, size_t workspace_bytes, void *stream)
{
    NRF_CHECK_ARG(nx >= 2 && ny >= 2 && nz >= 2 && (int64_t)nx * ny * nz <= (int64_t)INT32_MAX, "nrf_mesh_voxelize: lattice %d x %d x %d (each >= 2, product < 2^31)", nx, ny,
                  nz);
    NRF_CHECK_ARG(n_faces >= 0 && n_faces <= (int64_t)INT32_MAX - 1, "nrf_mesh_voxelize: %lld faces (0 .. 2^31 - 2)", (long long)n_faces);
    NRF_CHECK_ARG(n_verts >= 0 && n_verts <= INT32_MAX, "nrf_mesh_voxelize: %lld vertices (0 .. 2^31 - 1)", (long long)n_verts);
    NRF_CHECK_ARG(bbox, "nrf_mesh_voxelize: null bbox");
    NRF_CHECK_ARG(n_faces == 0 || d_faces, "nrf_mesh_voxelize: null d_faces");
    NRF_CHECK_ARG(d_verts || n_verts == 0 || n_faces == 0, "nrf_mesh_voxelize: null d_verts");
    NRF_CHECK_ARG(d_winding || d_sdf || d_face, "nrf_mesh_voxelize: d_winding, d_sdf and d_face are all null");
    NRF_CHECK_ARG(rule == NRF_VOX_NONZERO || rule == NRF_VOX_POSITIVE || rule == NRF_VOX_ODD, "nrf_mesh_voxelize: rule must be 0, 1 or 2 (got %d)", rule);
    const bool with_dist = d_sdf || d_face;
    NRF_CHECK_ARG(!with_dist || (std::isfinite(trunc) && trunc > 0.0f), "nrf_mesh_voxelize: trunc must be finite and > 0 (got %g)", (double)trunc);
    VxLat g;
    const int n[3] = {nx, ny, nz};
    for (int a = 0; a < 3; a++) {
        g.n[a] = n[a];
        g.bmin[a] = bbox[a];
        g.step[a] = (bbox[3 + a] - bbox[a]) / (float)(n[a] - 1);          // fp32, one rounding per operation
        NRF_CHECK_ARG(std::isfinite(bbox[a]) && std::isfinite(bbox[3 + a]) && bbox[3 + a] > bbox[a] && std::isfinite(g.step[a]) && g.step[a] > 0.0f,
                      "nrf_mesh_voxelize: empty, inverted or non-finite box on axis %d ([%g, %g])", a, (double)bbox[a], (double)bbox[3 + a]);
    }
    g.trunc = with_dist ? trunc : 0.0f;
    g.t2 = g.trunc * g.trunc;
    NRF_CHECK_ARG(d_workspace && (reinterpret_cast<uintptr_t>(d_workspace) & 255) == 0, "nrf_mesh_voxelize: the workspace must be non-null and 256-byte aligned");
    Bump bump(d_workspace, workspace_bytes);
    const VoxWs ws = vox_layout(bump, n_verts, n_faces, nx, ny, nz, with_dist);
    NRF_CHECK_ARG(bump.cap >= vox_bytes(n_verts, n_faces, nx, ny, nz, with_dist) && bump.ok(), "nrf_mesh_voxelize: workspace %zu < %zu bytes", workspace_bytes,
                  vox_bytes(n_verts, n_faces, nx, ny, nz, with_dist));

    hipStream_t st = as_stream(stream);
    const int64_t n_pts = (int64_t)nx * ny * nz;
    hipLaunchKernelGGL(k_vox_init, dim3((unsigned)ceil_div(n_pts, VX_BLOCK)), dim3(VX_BLOCK), 0, st, n_pts, ws.delta, ws.key);
    NRF_LAUNCH_CHECK();
    if (n_faces > 0) {
        NRF_HIP(hipMemsetAsync(ws.n_wide, 0, 2 * sizeof(uint32_t), st));
        if (n_verts > 0) {
            hipLaunchKernelGGL(k_vox_project, dim3((unsigned)ceil_div(n_verts, VX_BLOCK)), dim3(VX_BLOCK), 0, st, d_verts, n_verts, g, ws.vert);
            NRF_LAUNCH_CHECK();
        }
        const int64_t face_blocks = ceil_div(n_faces, VX_BLOCK);
        hipLaunchKernelGGL(k_vox_faces, dim3((unsigned)(face_blocks < VX_FACE_GRID ? face_blocks : VX_FACE_GRID)), dim3(VX_BLOCK), 0, st, d_verts, (int32_t)n_verts, d_faces,
                           n_faces, (const int4 *)ws.vert, g, ws.delta, ws.key, ws.wide_col, ws.wide_pts, ws.n_wide, d_stats);
        NRF_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_vox_wide, dim3(VX_WIDE_GRID), dim3(VX_BLOCK), 0, st, d_verts, (int32_t)n_verts, d_faces, n_faces, (const int4 *)ws.vert, g, ws.delta, ws.key,
                           (const int32_t *)ws.wide_col, (const int32_t *)ws.wide_pts, (const uint32_t *)ws.n_wide);
        NRF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_vox_finish, dim3((unsigned)ceil_div((int64_t)nx * ny, VX_BLOCK)), dim3(VX_BLOCK), 0, st, g, rule, (const int32_t *)ws.delta,
                       (const unsigned long long *)ws.key, d_winding, d_sdf, d_face);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

}  // extern "C"
