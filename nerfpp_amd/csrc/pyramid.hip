// pyramid.hip -- the language targets of LeRF training read from a cached CLIP pyramid: PyramidEmbedding::GetPixelValue (PyramidEmbedder.cpp:4-196,
// :230-310) for a batch of pixels on the device, and the relevancy preview loop of NeRFExecutor::Train (NeRFExecutor.h:803-831).  Building a pyramid (RuCLIP on
// OpenCV tiles, PyramidEmbedder::operator()) is out of scope; a pyramid is the reference's cache (pyramid_embeddings.pt) handed over entry by entry.
//
// Layout: one dense fp32 block [nh][nw][D] per (image, level), levels -1 .. max_zoom_out, grid geometry as GetNearestPatchIndicesSingleScale computes it.
// The scale-dependent choices (the two levels, which of the three cross-level forms) are made on the host once per call and reach the kernel as arguments
// (the two levels' {block, nw, nh, win} by value: no table load on the device).  The per-pixel choices (patch indices, centres, which Interpolate form) are
// the kernel's, one wave per pixel, so each is wave-uniform.  Arithmetic is the reference's ATen fp32 sequence, one rounding per op (-ffp-contract=off,
// correctly rounded fp32 division), so results equal the LibTorch CPU path bit for bit, NaN rows included.
#include "common.h"
#include "workspace.h"

#include <cmath>
#include <vector>

using namespace nrf;

namespace {

constexpr int PYR_WAVES = 4;         // pixels per 256-thread block

// GetNearestPatchIndicesSingleScale (PyramidEmbedder.cpp:15-19) -- the reference's own types: int * double -> int window; (int - int * float) is fp32,
// divided in double by int * (1. - float), truncated toward zero
static inline int pyr_window(int clip, int zoom) { return (int)(clip * pow(2.0, (double)zoom)); }
static inline int pyr_count(int img, int win, float overlap) { return (int)((img - win * overlap) / (win * (1. - overlap))); }

// patch centre (:47-60): float(int(idx * win * (1. - Overlap))) + win/2 (integer division)
__device__ inline float pyr_centre(int idx, int win, double omo) { return (float)(int)((double)(idx * win) * omo) + (float)(win / 2); }

struct PyrLevel {                    // one (image, level) block
    const float *emb;                // [nh][nw][D]
    int nw, nh, win;
};

struct PyrCall {
    PyrLevel lv[2];                  // levels z1, z2
    int use;                         // 1: e1 only, 2: e2 only, 3: e1 + (e2 - e1) / dz * tz   (PyramidEmbedder.cpp:300-307)
    float dz, tz;                    // zoom_out2 - zoom_out1, zoom_out - zoom_out1
    float omo;                       // 1.f - Overlap
    double omo_d;                    // 1. - Overlap
    int d;
};

// The per-pixel part of one level: Interpolate's form (PyramidEmbedder.cpp:174-195) and its scalars
struct PyrSel {
    const float *e11, *e21, *e12, *e22;
    int form;                        // 0: E11; 1: x2 == x1; 2: y2 == y1; 3: bilinear
    float d1, a, b, c, e;
};

__device__ inline int pyr_clamp(int i, int n)
{
    if (i < 0) i = 0;
    if (i >= n) i = n - 1;
    return i;
}

__device__ inline PyrSel pyr_select(const PyrLevel &l, float x, float y, const PyrCall &c)
{
    const float hp = x / (float)l.win / c.omo, vp = y / (float)l.win / c.omo;          // :21-22
    const int h1 = pyr_clamp((int)(hp - 2.0f), l.nw), h2 = pyr_clamp((int)(hp - 1.0f), l.nw);
    const int v1 = pyr_clamp((int)(vp - 2.0f), l.nh), v2 = pyr_clamp((int)(vp - 1.0f), l.nh);
    const float x1 = pyr_centre(h1, l.win, c.omo_d), x2 = pyr_centre(h2, l.win, c.omo_d);
    const float y1 = pyr_centre(v1, l.win, c.omo_d), y2 = pyr_centre(v2, l.win, c.omo_d);
    const int64_t D = c.d;
    PyrSel s;
    s.e11 = l.emb + ((int64_t)v1 * l.nw + h1) * D;          // {hor idx1, vert idx1}
    s.e21 = l.emb + ((int64_t)v1 * l.nw + h2) * D;          // {hor idx2, vert idx1}
    s.e12 = l.emb + ((int64_t)v2 * l.nw + h1) * D;          // {hor idx1, vert idx2}
    s.e22 = l.emb + ((int64_t)v2 * l.nw + h2) * D;
    s.a = s.b = s.c = s.e = 0.0f; s.d1 = 1.0f;
    if (x2 == x1 && y2 == y1) {
        s.form = 0;
    } else if (x2 == x1) {
        s.form = 1; s.d1 = y2 - y1; s.c = y - y1;
    } else if (y2 == y1) {
        s.form = 2; s.d1 = x2 - x1; s.c = x - x1;
    } else {
        s.form = 3; s.d1 = (x2 - x1) * (y2 - y1); s.a = x2 - x; s.b = y2 - y; s.c = x - x1; s.e = y - y1;
    }
    return s;
}

template <int VEC>
struct Vf {
    float v[VEC];
};

template <int VEC>
__device__ inline Vf<VEC> ldv(const float *p)
{
    Vf<VEC> r;
    if constexpr (VEC == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
    } else {
        r.v[0] = *p;
    }
    return r;
}

template <int VEC>
__device__ inline void stv(float *p, const Vf<VEC> &r)
{
    if constexpr (VEC == 4) *reinterpret_cast<float4 *>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    else *p = r.v[0];
}

// Interpolate on elements [j, j + VEC): ATen tensor-by-scalar ops, one rounding each, the four terms summed left to right
template <int VEC>
__device__ inline Vf<VEC> pyr_interp(const PyrSel &s, int j)
{
    Vf<VEC> r = ldv<VEC>(s.e11 + j);
    if (s.form == 1 || s.form == 2) {
        const Vf<VEC> o = ldv<VEC>((s.form == 1 ? s.e12 : s.e21) + j);
#pragma unroll
        for (int k = 0; k < VEC; k++) r.v[k] = r.v[k] + (o.v[k] - r.v[k]) / s.d1 * s.c;
    } else if (s.form == 3) {
        const Vf<VEC> e21 = ldv<VEC>(s.e21 + j), e12 = ldv<VEC>(s.e12 + j), e22 = ldv<VEC>(s.e22 + j);
#pragma unroll
        for (int k = 0; k < VEC; k++) {
            const float t1 = r.v[k] / s.d1 * s.a * s.b, t2 = e21.v[k] / s.d1 * s.c * s.b;
            const float t3 = e12.v[k] / s.d1 * s.a * s.e, t4 = e22.v[k] / s.d1 * s.c * s.e;
            r.v[k] = t1 + t2 + t3 + t4;
        }
    }
    return r;
}

// One wave per pixel.  Pixel p's coordinates are (xs[p], ys[p]) or, without arrays, the raster position q = q0 + p of a grid_w wide image: x = column, y = row
// (the preview's GetPixelValue(i, j, ...)).  Row p of the output starts at out + p * out_stride.
template <int VEC>
__global__ void __launch_bounds__(64 * PYR_WAVES) k_pyramid_pixels(PyrCall c, const int64_t *__restrict__ xs, const int64_t *__restrict__ ys, int64_t n, int grid_w,
                                                                   int64_t q0, float *__restrict__ out, int64_t out_stride)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t p = (int64_t)blockIdx.x * PYR_WAVES + wave;
    if (p >= n) return;
    const int lane = (int)(threadIdx.x & 63);
    float x, y;
    if (xs) {
        x = (float)xs[p];                                     // rand_h.to(kFloat).item<float>() (NeRFDataset.cpp:186-187)
        y = (float)ys[p];
    } else {
        const int64_t q = q0 + p;
        x = (float)(int)(q % grid_w);
        y = (float)(int)(q / grid_w);
    }
    float *o = out + p * out_stride;
    if (c.use != 3) {
        const PyrSel s = pyr_select(c.use == 2 ? c.lv[1] : c.lv[0], x, y, c);
        for (int j = lane * VEC; j < c.d; j += 64 * VEC) stv<VEC>(o + j, pyr_interp<VEC>(s, j));
        return;
    }
    const PyrSel s1 = pyr_select(c.lv[0], x, y, c), s2 = pyr_select(c.lv[1], x, y, c);
    for (int j = lane * VEC; j < c.d; j += 64 * VEC) {
        const Vf<VEC> e1 = pyr_interp<VEC>(s1, j), e2 = pyr_interp<VEC>(s2, j);
        Vf<VEC> r;
#pragma unroll
        for (int k = 0; k < VEC; k++) r.v[k] = e1.v[k] + (e2.v[k] - e1.v[k]) / c.dz * c.tz;
        stv<VEC>(o + j, r);
    }
}

// set_entries: row mv[2k] of src goes to the block position mv[2k + 1] (in floats)
__global__ void k_pyramid_scatter(const float *__restrict__ src, const int64_t *__restrict__ mv, int d, float *__restrict__ emb)
{
    const float *s = src + mv[2 * blockIdx.x] * d;
    float *o = emb + mv[2 * blockIdx.x + 1];
    for (int j = threadIdx.x; j < d; j += blockDim.x) o[j] = s[j];
}

// cv::saturate_cast<uchar>(lv * 255) (NeRFExecutor.h:826): cvRound is cvtss2si on x86 (round half to even; NaN and values outside int32 give INT_MIN), then a
// clamp to [0, 255]
__global__ void k_pyramid_gray(const float *__restrict__ rel, int64_t n, uint8_t *__restrict__ gray)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = rel[2 * i] * 255.0f;
    int iv = (v >= -2147483648.0f && v < 2147483648.0f) ? (int)rintf(v) : INT32_MIN;
    gray[i] = (uint8_t)(iv < 0 ? 0 : iv > 255 ? 255 : iv);
}

}  // namespace

struct nrf_pyramid {
    int d = 0, clip = 0, n_images = 0, max_zoom = 0, n_levels = 0;
    float overlap = 0.0f;
    std::vector<int> wh;                       // [n_images][2] = {W, H}
    std::vector<int> nw, nh, win;              // [n_images * n_levels]
    std::vector<int64_t> off;                  // block offset in floats, -1 = no grid at this level
    std::vector<int64_t> filled;               // distinct entries set per block
    std::vector<uint8_t> have;                 // per grid cell of every block
    std::vector<int64_t> cell0;                // first cell of each block in `have`
    int64_t elems = 0;
    nrf::DevBuf d_emb;                         // float [elems]
};

int nrf_pyramid_level_geometry(int img_w, int img_h, int clip, float overlap, int zoom, int *out)
{
    NRF_CHECK_ARG(out && img_w > 0 && img_h > 0 && clip > 0 && overlap >= 0.0f && overlap < 1.0f && zoom >= -1 && zoom <= 24,
                  "nrf_pyramid_level_geometry: bad argument (w %d, h %d, clip %d, overlap %g, zoom %d)", img_w, img_h, clip, (double)overlap, zoom);
    const int w = pyr_window(clip, zoom);
    NRF_CHECK_ARG(w > 0, "nrf_pyramid_level_geometry: empty window (clip %d, zoom %d)", clip, zoom);
    out[0] = w;
    out[1] = pyr_count(img_w, w, overlap);
    out[2] = pyr_count(img_h, w, overlap);
    return NRF_OK;
}

int nrf_pyramid_max_zoom_out(const int *wh, int n_images, int clip, int *out)
{
    NRF_CHECK_ARG(wh && out && n_images >= 1 && clip > 0, "nrf_pyramid_max_zoom_out: bad argument");
    int wmax = 0, hmax = 0;
    for (int i = 0; i < n_images; i++) {
        if (wh[2 * i + 1] > hmax) hmax = wh[2 * i + 1];
        if (wh[2 * i] > wmax) wmax = wh[2 * i];
    }
    // NeRFDataset.cpp:86, :178: integer quotients, log2f, the smaller of the two stored into an int
    NRF_CHECK_ARG(wmax / clip >= 1 && hmax / clip >= 1, "nrf_pyramid_max_zoom_out: the largest view (%d x %d) is smaller than the CLIP input size %d (log2f(0))",
                  wmax, hmax, clip);
    *out = (int)std::min(log2f((float)(wmax / clip)), log2f((float)(hmax / clip)));
    return NRF_OK;
}

int nrf_pyramid_create(int d, int clip_size, float overlap, int max_zoom_out, int n_images, const int *wh, nrf_pyramid **out)
{
    NRF_CHECK_ARG(out && wh, "nrf_pyramid_create: null pointer");
    *out = nullptr;
    NRF_CHECK_ARG(d >= 1 && clip_size >= 1 && overlap >= 0.0f && overlap < 1.0f && max_zoom_out >= -1 && max_zoom_out <= 24 && n_images >= 1,
                  "nrf_pyramid_create: bad argument (D %d, clip %d, overlap %g, max_zoom_out %d, images %d)", d, clip_size, (double)overlap, max_zoom_out, n_images);
    for (int i = 0; i < n_images; i++)
        NRF_CHECK_ARG(wh[2 * i] >= 1 && wh[2 * i + 1] >= 1, "nrf_pyramid_create: view %d has size %d x %d", i, wh[2 * i], wh[2 * i + 1]);
    std::unique_ptr<nrf_pyramid> p(new nrf_pyramid());
    p->d = d; p->clip = clip_size; p->overlap = overlap; p->max_zoom = max_zoom_out; p->n_images = n_images; p->n_levels = max_zoom_out + 2;
    p->wh.assign(wh, wh + 2 * n_images);
    const int nb = n_images * p->n_levels;
    p->nw.resize(nb); p->nh.resize(nb); p->win.resize(nb); p->off.resize(nb); p->filled.assign(nb, 0); p->cell0.resize(nb);
    int64_t cells = 0;
    for (int i = 0; i < n_images; i++) {
        for (int l = 0; l < p->n_levels; l++) {
            const int b = i * p->n_levels + l, w = pyr_window(clip_size, l - 1);
            const int nw = pyr_count(wh[2 * i], w, overlap), nh = pyr_count(wh[2 * i + 1], w, overlap);
            p->win[b] = w;
            p->cell0[b] = cells;
            if (w > 0 && nw > 0 && nh > 0) {
                p->nw[b] = nw; p->nh[b] = nh; p->off[b] = cells * d;
                cells += (int64_t)nw * nh;
            } else {
                p->nw[b] = p->nh[b] = 0; p->off[b] = -1;
            }
        }
    }
    p->have.assign((size_t)cells, 0);
    p->elems = cells * d;
    if (p->elems > 0) {
        NRF_TRY(p->d_emb.resize((size_t)p->elems * sizeof(float)));
        NRF_HIP(hipMemset(p->d_emb.as<float>(), 0, (size_t)p->elems * sizeof(float)));
    }
    *out = p.release();
    return NRF_OK;
}

int nrf_pyramid_destroy(nrf_pyramid *p)
{
    delete p;
    return NRF_OK;
}

int64_t nrf_pyramid_memory_bytes(const nrf_pyramid *p) { return p ? p->elems * (int64_t)sizeof(float) : 0; }

int nrf_pyramid_set_entries(nrf_pyramid *p, int64_t n, const int32_t *keys, const float *emb, int d, void *stream)
{
    NRF_CHECK_ARG(p && n >= 0, "nrf_pyramid_set_entries: bad argument");
    NRF_CHECK_ARG(d == p->d, "nrf_pyramid_set_entries: embeddings of %d floats for a pyramid of D = %d", d, p->d);
    if (n == 0) return NRF_OK;
    NRF_CHECK_ARG(keys && emb, "nrf_pyramid_set_entries: null pointer");
    std::vector<int64_t> cell((size_t)n), dst((size_t)n);
    for (int64_t k = 0; k < n; k++) {
        const int32_t *key = keys + 4 * k;              // {hor_pos_idx, vert_pos_idx, zoom_out_idx, data_img_id} (PyramidEmbedder.h:65)
        const int hor = key[0], vert = key[1], zoom = key[2], img = key[3];
        NRF_CHECK_ARG(img >= 0 && img < p->n_images && zoom >= -1 && zoom <= p->max_zoom,
                      "nrf_pyramid_set_entries: entry %lld {%d, %d, %d, %d}: image outside [0, %d) or level outside [-1, %d]", (long long)k, hor, vert, zoom, img,
                      p->n_images, p->max_zoom);
        const int b = img * p->n_levels + zoom + 1;
        NRF_CHECK_ARG(hor >= 0 && hor < p->nw[b] && vert >= 0 && vert < p->nh[b],
                      "nrf_pyramid_set_entries: entry %lld {%d, %d, %d, %d} lies outside that level's %d x %d grid", (long long)k, hor, vert, zoom, img, p->nw[b], p->nh[b]);
        const int64_t c = (int64_t)vert * p->nw[b] + hor;
        cell[k] = p->cell0[b] + c;
        dst[k] = p->off[b] + c * p->d;
    }
    // a key given twice: the later row wins, as a std::map assignment does (PyramidEmbedding::Load, PyramidEmbedder.cpp:221)
    std::vector<uint8_t> taken(p->have.size(), 0);
    std::vector<int64_t> mv;
    for (int64_t k = n - 1; k >= 0; k--) {
        if (taken[(size_t)cell[k]]) continue;
        taken[(size_t)cell[k]] = 1;
        mv.push_back(k); mv.push_back(dst[k]);
    }
    const int64_t m = (int64_t)mv.size() / 2;
    hipStream_t st = as_stream(stream);
    const size_t src_bytes = align_up((size_t)n * d * sizeof(float), 256), mv_bytes = mv.size() * sizeof(int64_t);
    DevBuf staging;
    NRF_TRY(staging.resize(src_bytes + mv_bytes));
    char *tmp = staging.as<char>();
    NRF_HIP(hipMemcpyAsync(tmp, emb, (size_t)n * d * sizeof(float), hipMemcpyHostToDevice, st));
    NRF_HIP(hipMemcpyAsync(tmp + src_bytes, mv.data(), mv_bytes, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_pyramid_scatter, dim3((unsigned)m), dim3(256), 0, st, reinterpret_cast<const float *>(tmp), reinterpret_cast<const int64_t *>(tmp + src_bytes), d,
                       p->d_emb.as<float>());
    NRF_LAUNCH_CHECK();
    NRF_HIP(hipStreamSynchronize(st));         // the host arrays and the staging buffer are released before returning
    staging.reset();
    for (int64_t k = 0; k < n; k++) {
        if (!p->have[(size_t)cell[k]]) {
            p->have[(size_t)cell[k]] = 1;
            p->filled[keys[4 * k + 3] * p->n_levels + keys[4 * k + 2] + 1]++;
        }
    }
    return NRF_OK;
}

namespace {

// The host half of GetNearestPatchIndicesMultiScale + GetPixelValue (PyramidEmbedder.cpp:97-113, :300-307) for one (image, scale): both levels must have
// every entry (the reference reads both; a missing map entry is an undefined tensor it throws on).
int pyr_plan(const nrf_pyramid *p, int img_id, float scale, const char *who, PyrCall *c)
{
    NRF_CHECK_ARG(p, "%s: null pyramid", who);
    NRF_CHECK_ARG(img_id >= 0 && img_id < p->n_images, "%s: image %d outside [0, %d)", who, img_id, p->n_images);
    NRF_CHECK_ARG(std::isfinite(scale) && scale > 0.0f, "%s: scale %g is not a positive finite number", who, (double)scale);
    const float zoom = log2f(scale);                             // std::log2(float)
    int z1 = (int)zoom;
    if (z1 < -1) z1 = -1;
    if (z1 > p->max_zoom) z1 = p->max_zoom;
    int z2 = z1 + 1;
    if (z2 < -1) z2 = -1;
    if (z2 > p->max_zoom) z2 = p->max_zoom;
    const int zs[2] = {z1, z2};
    for (int k = 0; k < 2; k++) {
        const int b = img_id * p->n_levels + zs[k] + 1;
        NRF_CHECK_ARG(p->off[b] >= 0 && p->filled[b] == (int64_t)p->nw[b] * p->nh[b],
                      "%s: scale %g needs level %d of image %d, which has %lld of its %d x %d entries", who, (double)scale, zs[k], img_id, (long long)p->filled[b], p->nw[b],
                      p->nh[b]);
        c->lv[k].emb = p->d_emb.as<float>() + p->off[b];
        c->lv[k].nw = p->nw[b]; c->lv[k].nh = p->nh[b]; c->lv[k].win = p->win[b];
    }
    const float zo1 = (float)z1, zo2 = (float)z2;
    c->use = zoom == zo2 ? 2 : zoom == zo1 ? 1 : 3;              // `result = e2` is assigned after `result = e1`
    c->dz = zo2 - zo1;
    c->tz = zoom - zo1;
    c->omo = 1.f - p->overlap;
    c->omo_d = 1. - p->overlap;
    c->d = p->d;
    return NRF_OK;
}

int pyr_launch(const PyrCall &c, const int64_t *xs, const int64_t *ys, int64_t n, int grid_w, int64_t q0, float *out, int64_t out_stride, hipStream_t st)
{
    const bool vec4 = c.d % 4 == 0 && out_stride % 4 == 0 && ((uintptr_t)out & 15) == 0;
    const dim3 grid((unsigned)ceil_div(n, PYR_WAVES)), block(64 * PYR_WAVES);
    if (vec4) hipLaunchKernelGGL(k_pyramid_pixels<4>, grid, block, 0, st, c, xs, ys, n, grid_w, q0, out, out_stride);
    else hipLaunchKernelGGL(k_pyramid_pixels<1>, grid, block, 0, st, c, xs, ys, n, grid_w, q0, out, out_stride);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

}  // namespace

int nrf_pyramid_pixel_values(const nrf_pyramid *p, int img_id, float scale, const int64_t *d_x, const int64_t *d_y, int64_t n, float *d_out, int64_t out_stride,
                             void *stream)
{
    PyrCall c;
    NRF_TRY(pyr_plan(p, img_id, scale, "nrf_pyramid_pixel_values", &c));
    NRF_CHECK_ARG(n >= 0 && n <= ((int64_t)1 << 32), "nrf_pyramid_pixel_values: bad pixel count %lld", (long long)n);
    NRF_CHECK_ARG(out_stride >= p->d, "nrf_pyramid_pixel_values: output stride %lld below D = %d", (long long)out_stride, p->d);
    if (n == 0) return NRF_OK;
    NRF_CHECK_ARG(d_x && d_y && d_out, "nrf_pyramid_pixel_values: null pointer");
    return pyr_launch(c, d_x, d_y, n, 1, 0, d_out, out_stride, as_stream(stream));
}

// the preview's workspace for `rows` image rows at a time: their embeddings and relevancies
struct PreviewWs { float *emb, *rel; };
static PreviewWs preview_layout(Bump &b, const nrf_pyramid *p, int w, int rows)
{
    PreviewWs ws;
    ws.emb = b.take<float>((size_t)rows * w * p->d);
    ws.rel = b.take<float>((size_t)rows * w * 2);
    return ws;
}
static size_t pyr_preview_bytes(const nrf_pyramid *p, int w, int rows) { return measure([&](Bump &b) { preview_layout(b, p, w, rows); }); }

size_t nrf_pyramid_relevancy_preview_workspace_bytes(const nrf_pyramid *p, int img_id, int rows)
{
    if (!p || img_id < 0 || img_id >= p->n_images || rows < 1) return 0;
    const int w = p->wh[2 * img_id], h = p->wh[2 * img_id + 1];
    if (rows > h) rows = h;
    return pyr_preview_bytes(p, w, rows);
}

int nrf_pyramid_relevancy_preview(const nrf_pyramid *p, int img_id, float scale, const float *d_positives, int n_pos, const float *d_negatives, int n_neg, int positive_id,
                                  uint8_t *d_gray, uint8_t *d_bgr, void *d_workspace, size_t workspace_bytes, void *stream)
{
    PyrCall c;
    NRF_TRY(pyr_plan(p, img_id, scale, "nrf_pyramid_relevancy_preview", &c));
    NRF_CHECK_ARG(d_positives && d_negatives && d_gray && d_workspace, "nrf_pyramid_relevancy_preview: null pointer");
    NRF_CHECK_ARG(n_pos >= 1 && n_neg >= 1 && positive_id >= 0 && positive_id < n_pos && (size_t)(1 + n_neg) * p->d * sizeof(float) <= 64 * 1024,
                  "nrf_pyramid_relevancy_preview: phrases as nrf_lerf_relevancy takes them (P %d, Q %d, id %d, D %d)", n_pos, n_neg, positive_id, p->d);
    const int w = p->wh[2 * img_id], h = p->wh[2 * img_id + 1];
    // the caller's bytes decide how many rows go at a time.  rows of one row's bytes each fit: align_up(rows * a, 256) <= rows * align_up(a, 256)
    const int rows = (int)std::min<size_t>((size_t)h, workspace_bytes / pyr_preview_bytes(p, w, 1));
    if (rows < 1) {
        set_error("nrf_pyramid_relevancy_preview: a workspace of %zu bytes holds no row (%zu bytes per row)", workspace_bytes, pyr_preview_bytes(p, w, 1));
        return NRF_ERR_WORKSPACE;
    }
    Bump bump(d_workspace, workspace_bytes);
    const PreviewWs ws = preview_layout(bump, p, w, rows);
    NRF_TRY(ws_check(bump, 0, "nrf_pyramid_relevancy_preview"));
    hipStream_t st = as_stream(stream);
    float *emb = ws.emb, *rel = ws.rel;
    // NeRFExecutor.h:809-827 pixel by pixel; here rows [r0, r0 + rows) at a time: GetPixelValue(i, j) -> Relevancy -> saturate_cast<uchar>(rel[0, 0] * 255)
    for (int r0 = 0; r0 < h; r0 += rows) {
        const int64_t m = (int64_t)std::min(rows, h - r0) * w;
        NRF_TRY(pyr_launch(c, nullptr, nullptr, m, w, (int64_t)r0 * w, emb, p->d, st));
        NRF_TRY(nrf_lerf_relevancy(emb, m, p->d, d_positives, n_pos, d_negatives, n_neg, positive_id, rel, stream));
        hipLaunchKernelGGL(k_pyramid_gray, dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, st, rel, m, d_gray + (int64_t)r0 * w);
        NRF_LAUNCH_CHECK();
    }
    if (d_bgr) NRF_TRY(nrf_colormap_jet_u8(d_gray, (int64_t)w * h, d_bgr, stream));      // cv::applyColorMap(COLORMAP_JET) (:830)
    return NRF_OK;
}
