// tsdf.hip -- fuse rendered depth into a truncated signed distance volume on the lattice of nrf_density_grid (nrf_tsdf_integrate), and the two per-point queries the
// mesh front end needs on it (nrf_tsdf_observed, nrf_tsdf_sample_color).  The reference has no mesh export; the contract is stated in include/nerfpp_hip.h and
// restated in numpy by tests/tsdf_ref.py, which the GPU tests compare with bit for bit.
//
// k_tsdf_integrate is a streaming pass: per launch every voxel's tsdf / weight (and the four colour planes) are read once, updated by up to TSDF_BATCH views in
// array order in registers, and written once -- 8 B per voxel (40 B with colour) per batch, whatever the number of views in it.  The cameras of the batch travel in
// the kernel arguments (uniform: scalar loads, scalar registers), so a call allocates nothing and copies nothing.
//   * a wave covers 256 consecutive x of one lattice row: each lane owns 4 x-adjacent voxels and moves them with one 16-byte load / store per plane; the last
//     nx % 4 voxels of a row are a scalar tail (one dword each).  Rows of a lattice whose nx is no multiple of 4 start at a 4-byte-aligned address only, so the
//     16-byte type is declared with alignment 4: the same global_load_dwordx4 / global_store_dwordx4, legal at any dword address.
//   * y, z and everything that depends on them only are the wave's (readfirstlane of the wave id): formed once per view, not once per voxel.
//   * every voxel's projection is evaluated from its own lattice point by the header's formula, never incrementally along x: the bits do not depend on the blocking.
//   * no atomics, no workspace, no synchronisation; a voxel is owned by one lane, views are taken in order: two runs give the same bits, and one call over V views
//     gives what V calls of one view give (the state passes through fp32 memory unchanged between launches).
// The depth / acc / rgb images are gathered, one pixel per voxel and view (12.8 MB per view of 800 x 800: served from L2 / Infinity Cache).  Per view a lane first
// projects its 4 voxels, then issues all their depth and acc reads, then updates: the gathers overlap instead of queueing behind one another's latency.  The colour
// is read inside the update, by the voxels of the band |sdf| <= trunc only.
#include "common.h"

#include <cmath>
#include <climits>

namespace nrf {

namespace {

constexpr int TSDF_BATCH = 16;           // views per launch (16 x 96 B of cameras in the kernel arguments)
constexpr int TSDF_BLOCK = 256;          // 4 waves = 4 (row, x-chunk) tasks
constexpr int TSDF_WAVE_X = 256;         // x covered by a wave: 64 lanes x 4 voxels
constexpr int PT_BLOCK = 256;

typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

struct Lat {
    int nx, ny, nz;
    float bmin[3], step[3];
};

struct Cam {
    const float *depth, *acc, *rgb;
    int h, w;
    float fx, fy, cx, cy;
    float r[9];              // c2w's rotation, row-major: r[3 * i + j] = R_ij
    float t[3];
};

struct IntegrateArgs {
    Lat g;
    float *tsdf, *weight, *color;          // color: 4 planes of g.nx * g.ny * g.nz, or NULL
    int n_views, carve;
    float trunc, acc_min, max_weight;
    Cam cam[TSDF_BATCH];
};

// what the 4 voxels of a lane share in one view: the products of R^T (P - t) that hold y and z only (the lattice row's, so the wave's), and the image size as floats
struct RowTerms {
    float xy, xz, yy, yz, zy, zz;          // R10*qy, R20*qz; R11*qy, R21*qz; R12*qy, R22*qz
    float fw, fh;
};

// steps 1-2 of the header for one voxel: zd and the pixel index, or -1 where the view is skipped (behind the camera, outside the image)
__device__ __forceinline__ int64_t project(const Cam &c, const RowTerms &t, float px_, float &zd)
{
    const float qx = px_ - c.t[0];
    const float xc = (c.r[0] * qx + t.xy) + t.xz;
    const float yc = (c.r[1] * qx + t.yy) + t.yz;
    const float zc = (c.r[2] * qx + t.zy) + t.zz;
    zd = -zc;
    const float u = c.fx * (xc / zd) + c.cx;
    const float v = c.cy - c.fy * (yc / zd);
    const float fu = floorf(u + 0.5f), fv = floorf(v + 0.5f);
    const bool in = zd > 0.0f && fu >= 0.0f && fu < t.fw && fv >= 0.0f && fv < t.fh;          // as floats: NaN and huge values skip
    return in ? (int64_t)(int)(in ? fv : 0.0f) * c.w + (int)(in ? fu : 0.0f) : -1;
}

// steps 3-6 for one voxel whose depth d and (has_acc) acc a have been read; rgb: the pixel's colour, or NULL.  The colour is read here, by the few voxels of the band
// |sdf| <= trunc only: read for every voxel in the image beside depth and acc, it made the kernel 1.2-1.8x slower (the gathers are what the kernel waits for)
__device__ __forceinline__ void update(bool has_acc, const float *rgb, int carve, float trunc, float acc_min, float max_weight, float zd, float d, float a, float &D,
                                       float &W, float &cr, float &cg, float &cb, float &cw)
{
    float s, sdf = 0.0f;
    bool surface = true;
    if (has_acc) {
        if (a >= acc_min) d = d / a;
        else if (a < acc_min && carve) surface = false;          // a background observation
        else return;                                             // NaN a, or a < acc_min with carve off
    }
    if (surface) {
        if (!(d > 0.0f && d < INFINITY)) return;
        sdf = d - zd;
        if (sdf < -trunc) return;
        s = fminf(1.0f, sdf / trunc);
    } else {
        s = 1.0f;
    }
    const float Wn = W + 1.0f;
    D = (D * W + s) / Wn;
    W = fminf(Wn, max_weight);
    if (rgb && surface && fabsf(sdf) <= trunc) {
        const float cn = cw + 1.0f;
        cr = (cr * cw + rgb[0]) / cn;
        cg = (cg * cw + rgb[1]) / cn;
        cb = (cb * cw + rgb[2]) / cn;
        cw = fminf(cn, max_weight);
    }
}

template <bool COLOR> __global__ void __launch_bounds__(TSDF_BLOCK) k_tsdf_integrate(const IntegrateArgs a)
{
    const Lat &g = a.g;
    const int x_chunks = (g.nx + TSDF_WAVE_X - 1) / TSDF_WAVE_X;
    const int64_t task = (int64_t)blockIdx.x * (TSDF_BLOCK / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));          // wave-uniform
    const int64_t row = task / x_chunks;
    if (row >= (int64_t)g.ny * g.nz) return;
    const int chunk = (int)(task - row * x_chunks);
    const int iz = (int)(row / g.ny), iy = (int)(row - (int64_t)iz * g.ny);
    const int x0 = chunk * TSDF_WAVE_X + (int)(threadIdx.x & 63) * 4;
    if (x0 >= g.nx) return;
    const float py = g.bmin[1] + (float)iy * g.step[1], pz = g.bmin[2] + (float)iz * g.step[2];
    const int64_t base = row * g.nx + x0, plane = (int64_t)g.nx * g.ny * g.nz;
    const int m = g.nx - x0 < 4 ? g.nx - x0 : 4;           // 4, or the row's tail

    float D[4], W[4], C[4][4];            // C[plane][voxel]
    if (m == 4) {
        const f32x4_a4 d4 = *reinterpret_cast<const f32x4_a4 *>(a.tsdf + base), w4 = *reinterpret_cast<const f32x4_a4 *>(a.weight + base);
#pragma unroll
        for (int k = 0; k < 4; k++) { D[k] = d4[k]; W[k] = w4[k]; }
        if (COLOR) {
#pragma unroll
            for (int p = 0; p < 4; p++) {
                const f32x4_a4 c4 = *reinterpret_cast<const f32x4_a4 *>(a.color + p * plane + base);
#pragma unroll
                for (int k = 0; k < 4; k++) C[p][k] = c4[k];
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool in = k < m;
            D[k] = in ? a.tsdf[base + k] : 1.0f;
            W[k] = in ? a.weight[base + k] : 0.0f;
#pragma unroll
            for (int p = 0; p < 4; p++) C[p][k] = COLOR && in ? a.color[p * plane + base + k] : 0.0f;
        }
    }
    if (!COLOR) {
#pragma unroll
        for (int k = 0; k < 4; k++) C[0][k] = C[1][k] = C[2][k] = C[3][k] = 0.0f;
    }

    float px[4];
#pragma unroll
    for (int k = 0; k < 4; k++) px[k] = g.bmin[0] + (float)(x0 + k) * g.step[0];

    for (int v = 0; v < a.n_views; v++) {
        const Cam c = a.cam[v];           // read once per view, in front of the per-voxel branches: scalar loads, scalar registers
        const float qy = py - c.t[1], qz = pz - c.t[2];
        const RowTerms t = {c.r[3] * qy, c.r[6] * qz, c.r[4] * qy, c.r[7] * qz, c.r[5] * qy, c.r[8] * qz, (float)c.w, (float)c.h};
        // project the 4 voxels, then issue all their depth and acc reads together, then update: the gathers of a view overlap instead of queueing behind one another
        float zd[4];
        int64_t pix[4];
        bool any = false;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            pix[k] = project(c, t, px[k], zd[k]);
            if (k >= m) pix[k] = -1;
            any = any || pix[k] >= 0;
        }
        if (!any) continue;
        const bool has_acc = c.acc != nullptr, has_rgb = COLOR && c.rgb != nullptr;          // uniform
        float d[4], ac[4];
#pragma unroll
        for (int k = 0; k < 4; k++) d[k] = c.depth[pix[k] < 0 ? 0 : pix[k]];                 // pixel 0 exists (h, w >= 1): a skipped voxel reads it and drops it
#pragma unroll
        for (int k = 0; k < 4; k++) ac[k] = has_acc ? c.acc[pix[k] < 0 ? 0 : pix[k]] : 1.0f;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (pix[k] >= 0)
                update(has_acc, has_rgb ? c.rgb + pix[k] * 3 : nullptr, a.carve, a.trunc, a.acc_min, a.max_weight, zd[k], d[k], ac[k], D[k], W[k], C[0][k], C[1][k], C[2][k],
                       C[3][k]);
    }

    if (m == 4) {
        f32x4_a4 d4, w4;
#pragma unroll
        for (int k = 0; k < 4; k++) { d4[k] = D[k]; w4[k] = W[k]; }
        *reinterpret_cast<f32x4_a4 *>(a.tsdf + base) = d4;
        *reinterpret_cast<f32x4_a4 *>(a.weight + base) = w4;
        if (COLOR) {
#pragma unroll
            for (int p = 0; p < 4; p++) {
                f32x4_a4 c4;
#pragma unroll
                for (int k = 0; k < 4; k++) c4[k] = C[p][k];
                *reinterpret_cast<f32x4_a4 *>(a.color + p * plane + base) = c4;
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (k >= m) continue;
            a.tsdf[base + k] = D[k];
            a.weight[base + k] = W[k];
            if (COLOR) {
#pragma unroll
                for (int p = 0; p < 4; p++) a.color[p * plane + base + k] = C[p][k];
            }
        }
    }
}

// g = (pt - bmin) / step of one axis
__device__ __forceinline__ float lattice_g(const Lat &g, int axis, float x) { return (x - g.bmin[axis]) / g.step[axis]; }

__global__ void __launch_bounds__(PT_BLOCK) k_tsdf_observed(const Lat g, const float *__restrict__ weight, const float *__restrict__ pts, int64_t p, uint8_t *__restrict__ ok)
{
    const int64_t i = (int64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
    if (i >= p) return;
    const float x[3] = {pts[i * 3 + 0], pts[i * 3 + 1], pts[i * 3 + 2]};
    const int n[3] = {g.nx, g.ny, g.nz};
    int r[3];
    bool finite = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        finite = finite && fabsf(x[a]) < INFINITY;
        // clamped to [-1, n] as a float first: the conversion is exact, and after the index clamp below the result is what any larger value would give
        r[a] = (int)fminf(fmaxf(floorf(lattice_g(g, a, x[a]) + 0.5f), -1.0f), (float)n[a]);
    }
    bool all = finite;
    if (finite) {
        for (int dz = -1; dz <= 1; dz++)
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++) {
                    const int ix = min(max(r[0] + dx, 0), g.nx - 1), iy = min(max(r[1] + dy, 0), g.ny - 1), iz = min(max(r[2] + dz, 0), g.nz - 1);
                    all = all && weight[((int64_t)iz * g.ny + iy) * g.nx + ix] > 0.0f;
                }
    }
    ok[i] = all ? 1 : 0;
}

__global__ void __launch_bounds__(PT_BLOCK) k_tsdf_sample_color(const Lat g, const float *__restrict__ color, const float *__restrict__ pts, int64_t p,
                                                                float *__restrict__ rgb)
{
    const int64_t i = (int64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
    if (i >= p) return;
    const int n[3] = {g.nx, g.ny, g.nz};
    int i0[3];
    float f[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float gg = lattice_g(g, a, pts[i * 3 + a]);
        i0[a] = (int)fminf(fmaxf(floorf(gg), 0.0f), (float)(n[a] - 2));          // clamp((int)floorf(g), 0, n - 2), clamped as a float (NaN: 0)
        f[a] = fminf(fmaxf(gg - (float)i0[a], 0.0f), 1.0f);
    }
    const int64_t plane = (int64_t)g.nx * g.ny * g.nz;
    float den = 0.0f, num[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const int bx = c & 1, by = c >> 1 & 1, bz = c >> 2;
        const float wx = bx ? f[0] : 1.0f - f[0], wy = by ? f[1] : 1.0f - f[1], wz = bz ? f[2] : 1.0f - f[2];
        const float lam = (wx * wy) * wz;
        const int64_t j = ((int64_t)(i0[2] + bz) * g.ny + (i0[1] + by)) * g.nx + (i0[0] + bx);
        if (color[3 * plane + j] > 0.0f) {
            den = den + lam;
#pragma unroll
            for (int k = 0; k < 3; k++) num[k] = num[k] + lam * color[k * plane + j];
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) rgb[i * 3 + k] = den == 0.0f ? 0.0f : num[k] / den;
}

// the lattice of a call; bbox / dims checked (message names the call)
int make_lattice(const char *who, const float *bbox, int nx, int ny, int nz, Lat &g)
{
    NRF_CHECK_ARG(nx >= 2 && ny >= 2 && nz >= 2, "%s: lattice %d x %d x %d needs at least 2 points per axis", who, nx, ny, nz);
    NRF_CHECK_ARG(bbox, "%s: null bbox", who);
    const int n[3] = {nx, ny, nz};
    for (int a = 0; a < 3; a++) {
        NRF_CHECK_ARG(std::isfinite(bbox[a]) && std::isfinite(bbox[3 + a]) && bbox[3 + a] > bbox[a], "%s: empty, inverted or non-finite box on axis %d ([%g, %g])", who, a,
                      (double)bbox[a], (double)bbox[3 + a]);
        g.bmin[a] = bbox[a];
        g.step[a] = (bbox[3 + a] - bbox[a]) / (float)(n[a] - 1);          // fp32, one rounding per operation
    }
    g.nx = nx; g.ny = ny; g.nz = nz;
    return NRF_OK;
}

}  // namespace

}  // namespace nrf

using namespace nrf;

extern "C" {

int nrf_tsdf_integrate(float *d_tsdf, float *d_weight, float *d_color, int nx, int ny, int nz, const float *bbox, const nrf_tsdf_view *views, int n_views, float trunc,
                       float acc_min, float max_weight, int carve, void *stream)
{
    NRF_CHECK_ARG(d_tsdf && d_weight, "nrf_tsdf_integrate: null tsdf or weight");
    IntegrateArgs a{};
    NRF_TRY(make_lattice("nrf_tsdf_integrate", bbox, nx, ny, nz, a.g));
    NRF_CHECK_ARG(std::isfinite(trunc) && trunc > 0.0f, "nrf_tsdf_integrate: trunc must be finite and > 0 (got %g)", (double)trunc);
    NRF_CHECK_ARG(std::isfinite(acc_min) && acc_min > 0.0f, "nrf_tsdf_integrate: acc_min must be finite and > 0 (got %g)", (double)acc_min);
    NRF_CHECK_ARG(max_weight >= 1.0f, "nrf_tsdf_integrate: max_weight must be >= 1 (got %g)", (double)max_weight);
    NRF_CHECK_ARG(n_views >= 0 && (views || n_views == 0), "nrf_tsdf_integrate: %d views at %p", n_views, (const void *)views);
    for (int v = 0; v < n_views; v++)
        NRF_CHECK_ARG(views[v].d_depth && views[v].h >= 1 && views[v].w >= 1, "nrf_tsdf_integrate: view %d has a null depth image or an empty shape (%d x %d)", v, views[v].h,
                      views[v].w);
    const int64_t tasks = (int64_t)ny * nz * ceil_div(nx, TSDF_WAVE_X), blocks = ceil_div(tasks, TSDF_BLOCK / 64);
    NRF_CHECK_ARG(blocks <= INT32_MAX, "nrf_tsdf_integrate: lattice %d x %d x %d is too large for one launch", nx, ny, nz);
    a.tsdf = d_tsdf; a.weight = d_weight; a.color = d_color;
    a.carve = carve != 0;
    a.trunc = trunc; a.acc_min = acc_min; a.max_weight = max_weight;
    hipStream_t st = as_stream(stream);
    for (int v0 = 0; v0 < n_views; v0 += TSDF_BATCH) {
        a.n_views = n_views - v0 < TSDF_BATCH ? n_views - v0 : TSDF_BATCH;
        for (int v = 0; v < a.n_views; v++) {
            const nrf_tsdf_view &s = views[v0 + v];
            Cam &c = a.cam[v];
            c.depth = s.d_depth; c.acc = s.d_acc; c.rgb = s.d_rgb;
            c.h = s.h; c.w = s.w;
            c.fx = s.K[0]; c.cx = s.K[2]; c.fy = s.K[4]; c.cy = s.K[5];
            for (int i = 0; i < 3; i++) {
                for (int j = 0; j < 3; j++) c.r[3 * i + j] = s.c2w[4 * i + j];
                c.t[i] = s.c2w[4 * i + 3];
            }
        }
        if (d_color) hipLaunchKernelGGL(k_tsdf_integrate<true>, dim3((unsigned)blocks), dim3(TSDF_BLOCK), 0, st, a);
        else hipLaunchKernelGGL(k_tsdf_integrate<false>, dim3((unsigned)blocks), dim3(TSDF_BLOCK), 0, st, a);
        NRF_LAUNCH_CHECK();
    }
    return NRF_OK;
}

int nrf_tsdf_observed(const float *d_weight, int nx, int ny, int nz, const float *bbox, const float *d_pts, int64_t p, uint8_t *d_ok, void *stream)
{
    Lat g{};
    NRF_TRY(make_lattice("nrf_tsdf_observed", bbox, nx, ny, nz, g));
    NRF_CHECK_ARG(p >= 0 && p <= (int64_t)INT32_MAX * PT_BLOCK, "nrf_tsdf_observed: %lld points", (long long)p);
    if (p == 0) return NRF_OK;
    NRF_CHECK_ARG(d_weight && d_pts && d_ok, "nrf_tsdf_observed: null weight, points or output");
    hipLaunchKernelGGL(k_tsdf_observed, dim3((unsigned)ceil_div(p, PT_BLOCK)), dim3(PT_BLOCK), 0, as_stream(stream), g, d_weight, d_pts, p, d_ok);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

int nrf_tsdf_sample_color(const float *d_color, int nx, int ny, int nz, const float *bbox, const float *d_pts, int64_t p, float *d_rgb, void *stream)
{
    Lat g{};
    NRF_TRY(make_lattice("nrf_tsdf_sample_color", bbox, nx, ny, nz, g));
    NRF_CHECK_ARG(p >= 0 && p <= (int64_t)INT32_MAX * PT_BLOCK, "nrf_tsdf_sample_color: %lld points", (long long)p);
    if (p == 0) return NRF_OK;
    NRF_CHECK_ARG(d_color && d_pts && d_rgb, "nrf_tsdf_sample_color: null colour volume, points or output");
    hipLaunchKernelGGL(k_tsdf_sample_color, dim3((unsigned)ceil_div(p, PT_BLOCK)), dim3(PT_BLOCK), 0, as_stream(stream), g, d_color, d_pts, p, d_rgb);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

}  // extern "C"
