// texture.hip -- per-face texture atlases for the project's own meshes: the layout (nrf_atlas_dims), what to bake at every texel (nrf_atlas_texels), the sampler
// (nrf_texture_sample) and deferred texturing of a rasterised view (nrf_texture_shade).  The reference has no textures; the contract is stated in
// include/nerfpp_hip.h and restated in numpy by tests/texture_ref.py, which the GPU tests compare with bit for bit.
//
// Streaming kernels, one lane per texel, point or pixel, no LDS, no atomics, no workspace:
//   k_atlas_texels     consecutive lanes take consecutive texels of an atlas row, so the T lanes of a tile row share one face: its 12-byte index record and its three
//                      (or six, with normals) 12-byte vertex records are gathered once per wave from L1/L2, and the stores are the traffic: 4 + 12 + 12 + 44 B a texel
//   k_texture_sample   one lane per (face, barycentrics) pair: up to four texel gathers of C floats
//   k_texture_shade    one lane per pixel of a face map: the winner's three vertices, 1 / zd per corner by the rasteriser's own expressions, then the same sampler
// atlas_owner is the one copy of the layout on the device and atlas_sample the one copy of the filters: both sampling entries give the same bits for the same
// (face, barycentrics).  Every index is formed from a face < F and local indices inside a tile, so no read leaves the atlas (see atlas_sample).
#include "common.h"

#include <climits>
#include <cmath>

namespace nrf {

namespace {

constexpr int TX_BLOCK = 256;

struct AtlasDims {
    int cols, rows, width, height;
};

// the layout's integers on the host, or the header's refusal in the name of the entry `who`
int atlas_dims(const char *who, int64_t n_faces, int tile, AtlasDims &d)
{
    NRF_CHECK_ARG(tile >= NRF_ATLAS_MIN_TILE && tile <= NRF_ATLAS_MAX_TILE, "%s: tile %d (%d .. %d texels)", who, tile, NRF_ATLAS_MIN_TILE, NRF_ATLAS_MAX_TILE);
    NRF_CHECK_ARG(n_faces >= 0 && n_faces <= (int64_t)INT32_MAX - 1, "%s: %lld faces (0 .. 2^31 - 2)", who, (long long)n_faces);
    const int64_t cells = (n_faces + 1) / 2;
    int64_t cols = (int64_t)std::sqrt((double)cells);
    while (cols * cols < cells) cols++;
    while (cols > 0 && (cols - 1) * (cols - 1) >= cells) cols--;
    const int64_t rows = cols > 0 ? (cells + cols - 1) / cols : 0;
    const int64_t fit = NRF_ATLAS_MAX_SIZE / tile;
    NRF_CHECK_ARG(cols * tile <= NRF_ATLAS_MAX_SIZE && rows * tile <= NRF_ATLAS_MAX_SIZE,
                  "%s: %lld faces at tile %d need an atlas of %lld x %lld texels; a side is at most %d, so %lld faces fit", who, (long long)n_faces, tile,
                  (long long)(cols * tile), (long long)(rows * tile), NRF_ATLAS_MAX_SIZE, (long long)(2 * fit * fit));
    d.cols = (int)cols;
    d.rows = (int)rows;
    d.width = (int)(cols * tile);
    d.height = (int)(rows * tile);
    return NRF_OK;
}

// the owner of texel (X, Y) and its indices (i, j) in that face's own frame; -1 where the texel has no owner
__device__ __forceinline__ int32_t atlas_owner(int X, int Y, int T, int cols, int64_t n_faces, int &i, int &j)
{
    const int cc = X / T, cr = Y / T;
    i = X - cc * T;
    j = Y - cr * T;
    const bool upper = i + j > T - 2;
    if (upper) {
        i = T - 1 - i;
        j = T - 1 - j;
    }
    const int64_t f = 2 * ((int64_t)cr * cols + cc) + (upper ? 1 : 0);
    return f < n_faces ? (int32_t)f : -1;
}

struct Atlas {
    const float *tex;          // [height, width, C]
    int T, cols, width, C;
};

// steps 2-5 of nrf_texture_sample for a face 0 <= f < n_faces.  Every texel read has local indices 0 <= i, j and i + j <= n + 1 = T - 2, inside the tile of a cell
// f >> 1 < cells <= cols * rows: inside the atlas.
__device__ __forceinline__ void atlas_sample(const Atlas &a, int32_t f, float b1, float b2, int filter, float *__restrict__ out)
{
    const int n = a.T - 3;
    const float nf = (float)n;
    float x = b1 * nf, y = b2 * nf;
    if (!(x > 0.0f)) x = 0.0f;
    if (x > nf) x = nf;
    if (!(y > 0.0f)) y = 0.0f;
    if (y > nf) y = nf;
    const int cell = f >> 1;
    const int cr = cell / a.cols;
    const int X0 = (cell - cr * a.cols) * a.T, Y0 = cr * a.T;
    const bool odd = f & 1;
    auto texel = [&](int i, int j) -> const float * {
        const int X = odd ? X0 + a.T - 1 - i : X0 + i, Y = odd ? Y0 + a.T - 1 - j : Y0 + j;
        return a.tex + ((int64_t)Y * a.width + X) * a.C;
    };
    if (filter == NRF_TEXTURE_NEAREST) {
        const int i = (int)rintf(x);
        int j = (int)rintf(y);
        if (i + j > n + 1) j = n + 1 - i;
        const float *t = texel(i, j);
        for (int c = 0; c < a.C; c++) out[c] = t[c];
        return;
    }
    const float ix = floorf(x), iy = floorf(y);
    const float fx = x - ix, fy = y - iy;
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    const int i0 = (int)ix, j0 = (int)iy;
    const float w[4] = {gx * gy, fx * gy, gx * fy, fx * fy};
    const float *t[4];
    bool read[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int i = i0 + (k & 1), j = j0 + (k >> 1);
        read[k] = i + j <= n + 1;
        t[k] = read[k] ? texel(i, j) : a.tex;          // never dereferenced where !read
    }
    for (int c = 0; c < a.C; c++) {
        float o = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (read[k]) o = o + w[k] * t[k][c];
        out[c] = o;
    }
}

__global__ void __launch_bounds__(TX_BLOCK) k_atlas_texels(const float *__restrict__ verts, int32_t n_verts, const int32_t *__restrict__ faces, int64_t n_faces,
                                                           const float *__restrict__ normals, int T, int cols, int width, float offset, int row0, int64_t n_texels,
                                                           int32_t *__restrict__ out_face, float *__restrict__ out_bary, float *__restrict__ out_pos,
                                                           float *__restrict__ out_rays)
{
    const int64_t q = (int64_t)blockIdx.x * TX_BLOCK + threadIdx.x;          // < 2^28 + 256
    if (q >= n_texels) return;
    const int row = (int)((uint32_t)q / (uint32_t)width);
    const int X = (int)q - row * width;
    int i, j;
    int32_t f = atlas_owner(X, row0 + row, T, cols, n_faces, i, j);
    float b[3] = {0.0f, 0.0f, 0.0f}, P[3] = {0.0f, 0.0f, 0.0f}, N[3] = {0.0f, 0.0f, 0.0f};
    int32_t v[3] = {0, 0, 0};
    if (f >= 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) v[k] = faces[(int64_t)f * 3 + k];
        if (v[0] < 0 || v[0] >= n_verts || v[1] < 0 || v[1] >= n_verts || v[2] < 0 || v[2] >= n_verts) f = -1;
    }
    if (f >= 0) {
        float p0[3], e1[3], e2[3];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            p0[a] = verts[(int64_t)v[0] * 3 + a];
            e1[a] = verts[(int64_t)v[1] * 3 + a] - p0[a];
            e2[a] = verts[(int64_t)v[2] * 3 + a] - p0[a];
        }
        const float c[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const float len = sqrtf((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
        if (len > 0.0f) {
            const float nf = (float)(T - 3);
            b[1] = (float)i / nf;
            b[2] = (float)j / nf;
            b[0] = (1.0f - b[1]) - b[2];
#pragma unroll
            for (int a = 0; a < 3; a++) {
                P[a] = p0[a] + (b[1] * e1[a] + b[2] * e2[a]);
                N[a] = c[a] / len;
            }
            if (normals) {
                float m[3];
#pragma unroll
                for (int a = 0; a < 3; a++)
                    m[a] = (b[0] * normals[(int64_t)v[0] * 3 + a] + b[1] * normals[(int64_t)v[1] * 3 + a]) + b[2] * normals[(int64_t)v[2] * 3 + a];
                const float l = sqrtf((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
                if (l > 0.0f) {
#pragma unroll
                    for (int a = 0; a < 3; a++) N[a] = m[a] / l;
                }
            }
        } else {
            f = -1;
        }
    }
    out_face[q] = f;
    if (out_bary) {
#pragma unroll
        for (int a = 0; a < 3; a++) out_bary[q * 3 + a] = b[a];
    }
    if (out_pos) {
#pragma unroll
        for (int a = 0; a < 3; a++) out_pos[q * 3 + a] = P[a];
    }
    if (out_rays) {
        float *r = out_rays + q * 11;
        const bool owned = f >= 0;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            r[a] = owned ? P[a] + offset * N[a] : 0.0f;
            r[3 + a] = owned ? -N[a] : 0.0f;
            r[8 + a] = owned ? -N[a] : 0.0f;
        }
        r[6] = 0.0f;
        r[7] = owned ? 2.0f * offset : 0.0f;
    }
}

__global__ void __launch_bounds__(TX_BLOCK) k_texture_sample(const Atlas a, int64_t n_faces, const int32_t *__restrict__ face, const float *__restrict__ bary, int64_t p,
                                                             int filter, float *__restrict__ out)
{
    const int64_t q = (int64_t)blockIdx.x * TX_BLOCK + threadIdx.x;
    if (q >= p) return;
    const int32_t f = face[q];
    float *o = out + q * a.C;
    if (f < 0 || f >= n_faces) {
        for (int c = 0; c < a.C; c++) o[c] = 0.0f;
        return;
    }
    atlas_sample(a, f, bary[q * 3 + 1], bary[q * 3 + 2], filter, o);
}

struct ShadeCam {
    float rz[3];          // column 2 of c2w's rotation: R02, R12, R22
    float t[3];
};

__global__ void __launch_bounds__(TX_BLOCK) k_texture_shade(const float *__restrict__ verts, int32_t n_verts, const int32_t *__restrict__ faces, int64_t n_faces,
                                                            const int32_t *__restrict__ face_map, const float *__restrict__ bary_map, int64_t n_pix, const ShadeCam cam,
                                                            const Atlas a, int filter, float *__restrict__ out)
{
    const int64_t q = (int64_t)blockIdx.x * TX_BLOCK + threadIdx.x;
    if (q >= n_pix) return;
    const int32_t f = face_map[q];
    float *o = out + q * a.C;
    int32_t v[3] = {-1, -1, -1};
    if (f >= 0 && f < n_faces) {
#pragma unroll
        for (int k = 0; k < 3; k++) v[k] = faces[(int64_t)f * 3 + k];
    }
    if (v[0] < 0 || v[0] >= n_verts || v[1] < 0 || v[1] >= n_verts || v[2] < 0 || v[2] >= n_verts) {
        for (int c = 0; c < a.C; c++) o[c] = 0.0f;
        return;
    }
    float pk[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float qx = verts[(int64_t)v[k] * 3 + 0] - cam.t[0], qy = verts[(int64_t)v[k] * 3 + 1] - cam.t[1], qz = verts[(int64_t)v[k] * 3 + 2] - cam.t[2];
        const float zc = (cam.rz[0] * qx + cam.rz[1] * qy) + cam.rz[2] * qz;
        const float zd = -zc;
        pk[k] = bary_map[q * 3 + k] * (1.0f / zd);
    }
    const float S = (pk[0] + pk[1]) + pk[2];
    atlas_sample(a, f, pk[1] / S, pk[2] / S, filter, o);
}

int sampler_args_ok(const char *who, int64_t n_faces, int tile, int channels, int filter, AtlasDims &d)
{
    NRF_TRY(atlas_dims(who, n_faces, tile, d));
    NRF_CHECK_ARG(channels >= 1 && channels <= NRF_TEXTURE_MAX_CHANNELS, "%s: %d channels (1 .. %d)", who, channels, NRF_TEXTURE_MAX_CHANNELS);
    NRF_CHECK_ARG(filter == NRF_TEXTURE_NEAREST || filter == NRF_TEXTURE_BILINEAR, "%s: filter %d (NRF_TEXTURE_NEAREST or NRF_TEXTURE_BILINEAR)", who, filter);
    return NRF_OK;
}

}  // namespace

}  // namespace nrf

using namespace nrf;

extern "C" {

int nrf_atlas_dims(int64_t n_faces, int tile, int *width, int *height)
{
    NRF_CHECK_ARG(width && height, "nrf_atlas_dims: null width or height");
    AtlasDims d;
    NRF_TRY(atlas_dims("nrf_atlas_dims", n_faces, tile, d));
    *width = d.width;
    *height = d.height;
    return NRF_OK;
}

int nrf_atlas_texels(const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, const float *d_normals, int tile, float offset, int row0, int rows,
                     int32_t *d_face, float *d_bary, float *d_pos, float *d_rays, void *stream)
{
    AtlasDims d;
    NRF_TRY(atlas_dims("nrf_atlas_texels", n_faces, tile, d));
    NRF_CHECK_ARG(n_verts >= 0 && n_verts <= INT32_MAX, "nrf_atlas_texels: %lld vertices (0 .. 2^31 - 1)", (long long)n_verts);
    NRF_CHECK_ARG(std::isfinite(offset) && offset >= 0.0f, "nrf_atlas_texels: offset must be finite and >= 0 (got %g)", (double)offset);
    NRF_CHECK_ARG(row0 >= 0 && rows >= 0 && (int64_t)row0 + rows <= d.height, "nrf_atlas_texels: rows %d .. %lld of an atlas of %d rows", row0, (long long)row0 + rows,
                  d.height);
    NRF_CHECK_ARG(d_face || rows == 0, "nrf_atlas_texels: null d_face");
    NRF_CHECK_ARG(n_faces == 0 || (d_faces && (d_verts || n_verts == 0)), "nrf_atlas_texels: null d_verts or d_faces");
    const int64_t n_texels = (int64_t)rows * d.width;
    if (n_texels == 0) return NRF_OK;
    hipLaunchKernelGGL(k_atlas_texels, dim3((unsigned)ceil_div(n_texels, TX_BLOCK)), dim3(TX_BLOCK), 0, as_stream(stream), d_verts, (int32_t)n_verts, d_faces, n_faces,
                       d_normals, tile, d.cols, d.width, offset, row0, n_texels, d_face, d_bary, d_pos, d_rays);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

int nrf_texture_sample(const float *d_tex, int64_t n_faces, int tile, int channels, const int32_t *d_face, const float *d_bary, int64_t p, int filter, float *d_out,
                       void *stream)
{
    AtlasDims d;
    NRF_TRY(sampler_args_ok("nrf_texture_sample", n_faces, tile, channels, filter, d));
    NRF_CHECK_ARG(p >= 0, "nrf_texture_sample: %lld points", (long long)p);
    NRF_CHECK_ARG(p == 0 || (d_face && d_bary && d_out), "nrf_texture_sample: null d_face, d_bary or d_out");
    NRF_CHECK_ARG(p == 0 || n_faces == 0 || d_tex, "nrf_texture_sample: null d_tex");
    if (p == 0) return NRF_OK;
    const Atlas a{d_tex, tile, d.cols, d.width, channels};
    hipLaunchKernelGGL(k_texture_sample, dim3((unsigned)ceil_div(p, TX_BLOCK)), dim3(TX_BLOCK), 0, as_stream(stream), a, n_faces, d_face, d_bary, p, filter, d_out);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

int nrf_texture_shade(const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, const int32_t *d_face_map, const float *d_bary_map, int h, int w,
                      const float *K, const float *c2w, const float *d_tex, int tile, int channels, int filter, float *d_out, void *stream)
{
    AtlasDims d;
    NRF_TRY(sampler_args_ok("nrf_texture_shade", n_faces, tile, channels, filter, d));
    NRF_CHECK_ARG(h >= 1 && h <= NRF_RASTER_GUARD && w >= 1 && w <= NRF_RASTER_GUARD, "nrf_texture_shade: image %d x %d (h, w in 1 .. %d)", h, w, NRF_RASTER_GUARD);
    NRF_CHECK_ARG(n_verts >= 0 && n_verts <= INT32_MAX, "nrf_texture_shade: %lld vertices (0 .. 2^31 - 1)", (long long)n_verts);
    NRF_CHECK_ARG(d_face_map && d_bary_map && d_out, "nrf_texture_shade: null d_face_map, d_bary_map or d_out");
    NRF_CHECK_ARG(n_faces == 0 || (d_faces && K && c2w && d_tex && (d_verts || n_verts == 0)), "nrf_texture_shade: null d_verts, d_faces, K, c2w or d_tex");
    ShadeCam cam{};
    if (n_faces > 0) {
        for (int i = 0; i < 3; i++) {
            cam.rz[i] = c2w[4 * i + 2];
            cam.t[i] = c2w[4 * i + 3];
        }
    }
    const int64_t n_pix = (int64_t)h * w;
    const Atlas a{d_tex, tile, d.cols, d.width, channels};
    hipLaunchKernelGGL(k_texture_shade, dim3((unsigned)ceil_div(n_pix, TX_BLOCK)), dim3(TX_BLOCK), 0, as_stream(stream), d_verts, (int32_t)n_verts, d_faces, n_faces,
                       d_face_map, d_bary_map, n_pix, cam, a, filter, d_out);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

}  // extern "C"
