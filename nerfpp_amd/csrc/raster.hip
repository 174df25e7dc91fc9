// raster.hip -- a deterministic z-buffer rasteriser for the project's own meshes and its own camera (nrf_raster_mesh): depth, face id, barycentrics and
// interpolated vertex attributes of a triangle list seen from one pose.  The reference has no rasteriser; the contract is stated in include/nerfpp_hip.h and restated
// in numpy by tests/raster_ref.py, which the GPU tests compare with bit for bit.
//
// The meshes here are isosurfaces of 10^7 - 10^8 triangles, most of them smaller than a pixel: per-triangle scan with a 64-bit atomic min, no binning.
//   k_raster_project   one lane per vertex: steps 1-3 of the header into a 16-byte record {X, Y, zd, ok} in the workspace, so a face gathers 16 B per corner and the
//                      divisions of a vertex are paid once, not once per face that uses it
//   k_raster_faces     one lane per face: classify (bad index / clipped / degenerate or culled / drawn), the clamped bounding box, then either scan it (at most
//                      NRF_RASTER_WIDE_PIXELS pixels) or append the face to the wide list (scan.h's wave_append).  A fixed grid strides
//                      the face list and every lane counts its faces by class in registers: four atomic adds on d_stats per WORKGROUP.  With one add per wave and class
//                      -- 7 M waves at 447 M faces, all on one 16-byte line -- those adds were the whole kernel: 87.6 ms a view, and 159 ms with culling, which puts
//                      two classes into every wave (tools/raster_bench.py)
//   k_raster_wide      a fixed grid of workgroups strides the wide list (its length is read on the device: the host never sees it); the 256 lanes of a workgroup
//                      stride the pixels of one face's box, so no lane's time grows with a face's area
//   k_raster_resolve   one lane per pixel: depth and face from the key; barycentrics and attributes recomputed from the winner by the same device functions
// The z-buffer holds reduce.h's packed key (depth, face) per pixel, lowered by key_lower; depth > 0, so its bit pattern orders as the value does, and the result depends
// neither on scheduling nor on the order of the face list (beyond the tie-break by index the key states).  The kernel boundary makes the keys visible to the resolve pass.
// Coverage is decided in int64 (exact; edge_fn.h's edge_cover, the voxeliser's too); every edge value is e(0, 0) + i * step_x + j * step_y, which in integers is the header's E_ab(p) whatever the visiting order.
// Both face kernels and the resolve pass call tri_setup / tri_pixel for steps 4-7: one copy of the arithmetic, so the bits cannot differ between them.
// Every loop is bounded by a clamped bounding box or by a count; no kernel waits on another workgroup.
#include "edge_fn.h"
#include "reduce.h"
#include "scan.h"
#include "workspace.h"

#include <climits>
#include <cmath>

namespace nrf {

namespace {

constexpr int RS_BLOCK = 256;
constexpr int FACE_GRID = 1536;          // workgroups of k_raster_faces, striding the face list: 6 per CU, what its 80 registers admit
constexpr int WIDE_GRID = 1024;          // workgroups of k_raster_wide: 4 per CU

struct RCam {
    float fx, fy, cx, cy;
    float r[9];              // c2w's rotation, row-major
    float t[3];
    float near_z;
};

struct RasterWs {
    int4 *vert;                      // [V] {X, Y, float_bits(zd), ok}
    unsigned long long *key;         // [h * w]
    int32_t *wide;                   // [F] the faces of the wide kernel, in any order
    uint32_t *n_wide;                // [1]
};

RasterWs raster_layout(Bump &b, int64_t n_verts, int64_t n_faces, int h, int w)
{
    RasterWs s;
    s.vert = b.take<int4>((size_t)n_verts);
    s.key = b.take<unsigned long long>((size_t)h * w);
    s.wide = b.take<int32_t>((size_t)n_faces);
    s.n_wide = b.take<uint32_t>(1);
    return s;
}

bool raster_shape_ok(int64_t n_verts, int64_t n_faces, int h, int w)
{
    return n_verts >= 0 && n_verts <= INT32_MAX && n_faces >= 0 && n_faces <= (int64_t)INT32_MAX - 1 && h >= 1 && h <= NRF_RASTER_GUARD && w >= 1 && w <= NRF_RASTER_GUARD;
}

// a face set up for steps 4-7: the three edge functions as e(0, 0) and their steps per pixel, already multiplied by s = sign(A); sA = s * A > 0
struct Tri {
    int64_t e00[3], sx[3], sy[3];
    int64_t sA;
    float r[3];                      // 1 / zd of the corners
    bool tl[3];
    int xmin, xmax, ymin, ymax;      // of the snapped corners
};

// step 4: A = E_01(v2), and -- for A != 0 -- the face's Tri.  a, b, c: the corners' records
__device__ __forceinline__ int64_t tri_setup(const int4 &a, const int4 &b, const int4 &c, Tri &t)
{
    const int64_t x[3] = {a.x, b.x, c.x}, y[3] = {a.y, b.y, c.y};
    const int64_t A = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0]);
    const int64_t s = A > 0 ? 1 : -1;
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
    t.r[0] = 1.0f / __int_as_float(a.z);
    t.r[1] = 1.0f / __int_as_float(b.z);
    t.r[2] = 1.0f / __int_as_float(c.z);
    t.xmin = min(a.x, min(b.x, c.x)); t.xmax = max(a.x, max(b.x, c.x));
    t.ymin = min(a.y, min(b.y, c.y)); t.ymax = max(a.y, max(b.y, c.y));
    return A;
}

// step 5's pixels: columns i0 .. i1 and rows j0 .. j1 (empty where i1 < i0 or j1 < j0).  >> of a negative int is arithmetic: floor
__device__ __forceinline__ void tri_box(const Tri &t, int h, int w, int &i0, int &i1, int &j0, int &j1)
{
    edge_box(t.xmin, t.xmax, t.ymin, t.ymax, w, h, i0, i1, j0, j1);
}

// steps 5-6 at pixel (column i, row j): inside?  and, where inside, b_k, p_k = b_k / zd_k, S and depth
__device__ __forceinline__ bool tri_pixel(const Tri &t, int i, int j, float b[3], float p[3], float &S, float &depth)
{
    int64_t se[3];
    if (!edge_cover(t.e00, t.sx, t.sy, t.tl, i, j, se)) return false;
    edge_bary(se, t.sA, b);
#pragma unroll
    for (int k = 0; k < 3; k++) p[k] = b[k] * t.r[k];
    S = (p[0] + p[1]) + p[2];
    depth = 1.0f / S;
    return true;
}

// step 7
__device__ __forceinline__ void tri_draw(const Tri &t, int i, int j, int w, uint32_t face, unsigned long long *__restrict__ key)
{
    float b[3], p[3], S, depth;
    if (!tri_pixel(t, i, j, b, p, S, depth)) return;
    key_lower(key + (int64_t)j * w + i, key_pack(depth, face));
}

__global__ void __launch_bounds__(RS_BLOCK) k_raster_project(const float *__restrict__ verts, int64_t n, const RCam c, int4 *__restrict__ rec)
{
    const int64_t i = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float qx = verts[i * 3 + 0] - c.t[0], qy = verts[i * 3 + 1] - c.t[1], qz = verts[i * 3 + 2] - c.t[2];
    const float xc = (c.r[0] * qx + c.r[3] * qy) + c.r[6] * qz;
    const float yc = (c.r[1] * qx + c.r[4] * qy) + c.r[7] * qz;
    const float zc = (c.r[2] * qx + c.r[5] * qy) + c.r[8] * qz;
    const float zd = -zc;
    const float u = c.fx * (xc / zd) + c.cx;
    const float v = c.cy - c.fy * (yc / zd);
    const bool ok = zd > c.near_z && fabsf(u) <= (float)NRF_RASTER_GUARD && fabsf(v) <= (float)NRF_RASTER_GUARD;          // as floats: NaN and +-inf clip
    int4 o;
    o.x = ok ? (int)rintf(u * (float)NRF_RASTER_SUBPIXEL) : 0;
    o.y = ok ? (int)rintf(v * (float)NRF_RASTER_SUBPIXEL) : 0;
    o.z = __float_as_int(zd);
    o.w = ok ? 1 : 0;
    rec[i] = o;
}

// the face's class (0 drawn, 1 clipped, 2 degenerate or culled, 3 bad index) and, for a drawn face, its Tri
__device__ __forceinline__ int face_setup(const int32_t *__restrict__ faces, int64_t f, int32_t n_verts, const int4 *__restrict__ rec, int cull, Tri &t)
{
    const int32_t v0 = faces[f * 3 + 0], v1 = faces[f * 3 + 1], v2 = faces[f * 3 + 2];
    if (v0 < 0 || v0 >= n_verts || v1 < 0 || v1 >= n_verts || v2 < 0 || v2 >= n_verts) return 3;
    const int4 a = rec[v0], b = rec[v1], c = rec[v2];
    if (!(a.w && b.w && c.w)) return 1;
    const int64_t A = tri_setup(a, b, c, t);
    return A == 0 || (cull && A > 0) ? 2 : 0;
}

__global__ void __launch_bounds__(RS_BLOCK) k_raster_faces(const int32_t *__restrict__ faces, int64_t n_faces, int32_t n_verts, const int4 *__restrict__ rec, int h,
                                                           int w, int cull, unsigned long long *__restrict__ key, int32_t *__restrict__ wide,
                                                           uint32_t *__restrict__ n_wide, uint32_t *__restrict__ stats)
{
    __shared__ uint32_t s_count[4];
    if (threadIdx.x < 4) s_count[threadIdx.x] = 0;
    __syncthreads();
    uint32_t count[4] = {0, 0, 0, 0};          // this lane's faces by class
    // the bound is the workgroup's: every lane of a wave makes every round (a lane past the last face has no class), so wave_append's ballot sees the whole wave
    for (int64_t base = (int64_t)blockIdx.x * RS_BLOCK; base < n_faces; base += (int64_t)gridDim.x * RS_BLOCK) {
        const int64_t f = base + threadIdx.x;
        Tri t;
        const int cls = f < n_faces ? face_setup(faces, f, n_verts, rec, cull, t) : -1;
#pragma unroll
        for (int c = 0; c < 4; c++) count[c] += cls == c;
        int i0 = 0, i1 = -1, j0 = 0, j1 = -1;
        if (cls == 0) tri_box(t, h, w, i0, i1, j0, j1);
        const bool any = i1 >= i0 && j1 >= j0;
        const bool is_wide = any && (int64_t)(i1 - i0 + 1) * (j1 - j0 + 1) > NRF_RASTER_WIDE_PIXELS;
        wave_append(is_wide, (int32_t)f, wide, n_wide);          // every face is appended at most once
        if (!any || is_wide) continue;
        for (int j = j0; j <= j1; j++)
            for (int i = i0; i <= i1; i++) tri_draw(t, i, j, w, (uint32_t)f, key);
    }
    if (!stats) return;          // uniform
#pragma unroll
    for (int c = 0; c < 4; c++)
        if (count[c]) atomicAdd(&s_count[c], count[c]);
    __syncthreads();
    if (threadIdx.x < 4 && s_count[threadIdx.x]) atomicAdd(stats + threadIdx.x, s_count[threadIdx.x]);
}

__global__ void __launch_bounds__(RS_BLOCK) k_raster_wide(const int32_t *__restrict__ faces, int32_t n_verts, const int4 *__restrict__ rec, int h, int w, int cull,
                                                          unsigned long long *__restrict__ key, const int32_t *__restrict__ wide, const uint32_t *__restrict__ n_wide)
{
    const uint32_t n = *n_wide;
    for (uint32_t q = blockIdx.x; q < n; q += WIDE_GRID) {
        const int32_t f = wide[q];
        Tri t;
        if (face_setup(faces, f, n_verts, rec, cull, t) != 0) continue;          // never taken: only drawn faces are listed
        int i0, i1, j0, j1;
        tri_box(t, h, w, i0, i1, j0, j1);
        const int bw = i1 - i0 + 1, n_pix = bw * (j1 - j0 + 1);                  // <= 2^28
        for (int p = threadIdx.x; p < n_pix; p += RS_BLOCK) {
            const int row = p / bw;
            tri_draw(t, i0 + (p - row * bw), j0 + row, w, (uint32_t)f, key);
        }
    }
}

__global__ void __launch_bounds__(RS_BLOCK) k_raster_resolve(const int32_t *__restrict__ faces, const int4 *__restrict__ rec, const float *__restrict__ attr, int n_attr,
                                                             int h, int w, const unsigned long long *__restrict__ key, float *__restrict__ depth,
                                                             int32_t *__restrict__ face, float *__restrict__ bary, float *__restrict__ out_attr)
{
    const int64_t pix = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
    if (pix >= (int64_t)h * w) return;
    const unsigned long long k = key[pix];
    const bool hit = k != NO_KEY;
    const int32_t f = hit ? key_index(k) : -1;
    depth[pix] = hit ? key_value(k) : 0.0f;
    if (face) face[pix] = f;
    if (!bary && n_attr == 0) return;
    float b[3] = {0.0f, 0.0f, 0.0f}, p[3] = {0.0f, 0.0f, 0.0f}, S = 1.0f, d;
    int32_t v[3] = {0, 0, 0};
    if (hit) {
        const int j = (int)(pix / w), i = (int)(pix - (int64_t)j * w);
#pragma unroll
        for (int c = 0; c < 3; c++) v[c] = faces[(int64_t)f * 3 + c];
        Tri t;
        tri_setup(rec[v[0]], rec[v[1]], rec[v[2]], t);
        tri_pixel(t, i, j, b, p, S, d);          // inside: the face drew this pixel
    }
    if (bary) {
#pragma unroll
        for (int c = 0; c < 3; c++) bary[pix * 3 + c] = b[c];
    }
    for (int c = 0; c < n_attr; c++) {
        float o = 0.0f;
        if (hit) o = ((p[0] * attr[(int64_t)v[0] * n_attr + c] + p[1] * attr[(int64_t)v[1] * n_attr + c]) + p[2] * attr[(int64_t)v[2] * n_attr + c]) / S;
        out_attr[pix * n_attr + c] = o;
    }
}

}  // namespace

}  // namespace nrf

using namespace nrf;

extern "C" {

size_t nrf_raster_workspace_bytes(int64_t n_verts, int64_t n_faces, int h, int w)
{
    if (!raster_shape_ok(n_verts, n_faces, h, w)) return 0;
    return measure([&](Bump &b) { raster_layout(b, n_verts, n_faces, h, w); });
}

int nrf_raster_mesh(const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, const float *d_attr, int n_attr, int h, int w, const float *K,
                    const float *c2w, float near_z, int cull, float *d_depth, int32_t *d_face, float *d_bary, float *d_out_attr, uint32_t *d_stats, void *d_workspace,
                    size_t workspace_bytes, void *stream)
{
    NRF_CHECK_ARG(h >= 1 && h <= NRF_RASTER_GUARD && w >= 1 && w <= NRF_RASTER_GUARD, "nrf_raster_mesh: image %d x %d (h, w in 1 .. %d)", h, w, NRF_RASTER_GUARD);
    NRF_CHECK_ARG(n_faces >= 0 && n_faces <= (int64_t)INT32_MAX - 1, "nrf_raster_mesh: %lld faces (0 .. 2^31 - 2)", (long long)n_faces);
    NRF_CHECK_ARG(n_verts >= 0 && n_verts <= INT32_MAX, "nrf_raster_mesh: %lld vertices (0 .. 2^31 - 1)", (long long)n_verts);
    NRF_CHECK_ARG(n_attr >= 0 && n_attr <= NRF_RASTER_MAX_ATTR, "nrf_raster_mesh: %d attributes (0 .. %d)", n_attr, NRF_RASTER_MAX_ATTR);
    NRF_CHECK_ARG(n_attr == 0 || (d_attr && d_out_attr), "nrf_raster_mesh: %d attributes with a null d_attr or d_out_attr", n_attr);
    NRF_CHECK_ARG(d_depth, "nrf_raster_mesh: null d_depth");
    NRF_CHECK_ARG(n_faces == 0 || (d_faces && K && c2w), "nrf_raster_mesh: null d_faces, K or c2w");
    NRF_CHECK_ARG(d_verts || n_verts == 0 || n_faces == 0, "nrf_raster_mesh: null d_verts");
    NRF_CHECK_ARG(std::isfinite(near_z) && near_z > 0.0f, "nrf_raster_mesh: near_z must be finite and > 0 (got %g)", (double)near_z);
    NRF_CHECK_ARG(cull == 0 || cull == 1, "nrf_raster_mesh: cull must be 0 or 1 (got %d)", cull);
    Bump bump(d_workspace, workspace_bytes);
    const RasterWs ws = raster_layout(bump, n_verts, n_faces, h, w);
    NRF_CHECK_ARG(d_workspace && bump.cap >= nrf_raster_workspace_bytes(n_verts, n_faces, h, w) && bump.ok(), "nrf_raster_mesh: workspace %zu < %zu bytes at %p",
                  workspace_bytes, nrf_raster_workspace_bytes(n_verts, n_faces, h, w), d_workspace);

    hipStream_t st = as_stream(stream);
    const int64_t n_pix = (int64_t)h * w;
    NRF_HIP(hipMemsetAsync(ws.key, 0xFF, (size_t)n_pix * sizeof(unsigned long long), st));          // NO_KEY
    if (n_faces > 0) {
        RCam c{};
        c.fx = K[0]; c.cx = K[2]; c.fy = K[4]; c.cy = K[5];
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) c.r[3 * i + j] = c2w[4 * i + j];
            c.t[i] = c2w[4 * i + 3];
        }
        c.near_z = near_z;
        NRF_HIP(hipMemsetAsync(ws.n_wide, 0, sizeof(uint32_t), st));
        if (n_verts > 0) {
            hipLaunchKernelGGL(k_raster_project, dim3((unsigned)ceil_div(n_verts, RS_BLOCK)), dim3(RS_BLOCK), 0, st, d_verts, n_verts, c, ws.vert);
            NRF_LAUNCH_CHECK();
        }
        const int64_t face_blocks = ceil_div(n_faces, RS_BLOCK);
        hipLaunchKernelGGL(k_raster_faces, dim3((unsigned)(face_blocks < FACE_GRID ? face_blocks : FACE_GRID)), dim3(RS_BLOCK), 0, st, d_faces, n_faces, (int32_t)n_verts, ws.vert, h, w, cull,
                           ws.key, ws.wide, ws.n_wide, d_stats);
        NRF_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_raster_wide, dim3(WIDE_GRID), dim3(RS_BLOCK), 0, st, d_faces, (int32_t)n_verts, ws.vert, h, w, cull, ws.key, ws.wide, ws.n_wide);
        NRF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_raster_resolve, dim3((unsigned)ceil_div(n_pix, RS_BLOCK)), dim3(RS_BLOCK), 0, st, d_faces, ws.vert, d_attr, n_attr, h, w, ws.key, d_depth,
                       d_face, d_bary, d_out_attr);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

}  // extern "C"
