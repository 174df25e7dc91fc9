// image_metrics.hip -- how good a rendered frame is: SSIM (Wang et al. 2004: 11-tap Gaussian window, sigma 1.5, the VALID region), its multi-scale form (Wang et al.
// 2003) and the mean squared error behind PSNR, on the device and in fp64.  No counterpart in the reference, whose only measure is the training loop's PSNR
// (NeRFExecutor.h:893).
//
// Why fp64: the variances E[x^2] - mu^2 cancel against c2 = 9e-4; in fp32 a flat pair (0.25 against 0.75) is off by 1.19e-4, the 4th digit of a number people quote to
// 3-4 digits.  Products of fp32 inputs are exact in fp64, every source-level op rounds once (-ffp-contract=off, no fused op is written here), and the order of the ops is
// part of the definition (include/nerfpp_hip.h), so a numpy float64 restatement equals the map bit for bit.
//
// k_ssim<T>: one workgroup of 256 lanes per 32 x 32 tile of the valid region of ONE channel of one image (grid: tiles x (b * c)).
//   1. the 42 x 42 input tiles of x and y (tile + 10-pixel apron; 0 beyond the image, which only masked outputs ever see) go to LDS once;
//   2. row pass: 42 rows x 32 columns of the five moments x, y, x*x, y*y, x*y, 11 taps each, into LDS as doubles (53.8 KB);
//   3. column pass from there, the SSIM formula, the optional map store, and the lane's sum of ssim and cs over its four outputs.
//   LDS: 14.1 KB + 53.8 KB = 67.9 KB with fp32 inputs (two workgroups per CU), 82.0 KB with fp64 inputs (the pooled scales of MS-SSIM: small grids).  A lane's 8-byte
//   accesses in both passes go to consecutive doubles across the 32 lanes of a tile row: 64 distinct banks per 32-lane group, conflict-free; the fp32 tile reads
//   are consecutive words of a 42-word row.
//   Sums: the lane's, then reduce.h's ordered block sum -> one fp64 pair per workgroup in the workspace; k_finish (one block per image channel) is reduce.h's ordered
//   finish pass over the pairs and divides by the count.  No atomics: two runs give the same bits, and an image's result does not depend on the batch it came in.
// k_pool2<T>: ((a00 + a01) + (a10 + a11)) * 0.25 in double, an odd trailing row / column dropped; the pooled planes are doubles in the workspace.
// k_mse: 4096 elements per block, lane t takes t, t + 256, ... in ascending order; the same partials and k_finish.
// k_ssim_loss<CT> / k_ssim_loss_finish: 1 - mean SSIM as a training loss and its gradient d loss / d x (nrf_ssim_loss); described where they stand.
#include "reduce.h"
#include "workspace.h"

#include <cmath>

namespace nrf {

namespace {

constexpr int IM_THREADS = 256;
constexpr int SS_TAPS = 11;
constexpr int SS_APRON = SS_TAPS - 1;
constexpr int SS_TILE = 32;                          // outputs per tile edge
constexpr int SS_IN = SS_TILE + SS_APRON;            // inputs per tile edge
constexpr int MSE_PER_BLOCK = 4096;
constexpr int MS_MAX_SCALES = 5;

struct SsimWindow {
    double g[SS_TAPS];
};

// g[k] = exp(-(k-5)^2 / 4.5) / sum, the sum added in order k = 0..10
SsimWindow ssim_window()
{
    SsimWindow w;
    for (int k = 0; k < SS_TAPS; k++) w.g[k] = std::exp(-(double)((k - 5) * (k - 5)) / 4.5);
    double sum = w.g[0];
    for (int k = 1; k < SS_TAPS; k++) sum = sum + w.g[k];
    for (int k = 0; k < SS_TAPS; k++) w.g[k] = w.g[k] / sum;
    return w;
}

template <class T>
__global__ void __launch_bounds__(IM_THREADS)
k_ssim(const T *__restrict__ x, const T *__restrict__ y, int h, int w, int c, int tiles_x, SsimWindow win, double c1, double c2, double *__restrict__ map,
       double *__restrict__ partials)
{
    __shared__ T s_x[SS_IN * SS_IN], s_y[SS_IN * SS_IN];
    __shared__ double s_m[5][SS_IN][SS_TILE];
    __shared__ double s_sum[2 * (IM_THREADS / 64)];
    const int t = threadIdx.x;
    const int ty0 = (int)(blockIdx.x / (unsigned)tiles_x) * SS_TILE, tx0 = (int)(blockIdx.x % (unsigned)tiles_x) * SS_TILE;
    const int img = (int)(blockIdx.y / (unsigned)c), ch = (int)(blockIdx.y % (unsigned)c);
    const int64_t base = (int64_t)img * h * w * c + ch;
    for (int e = t; e < SS_IN * SS_IN; e += IM_THREADS) {
        const int r = e / SS_IN, q = e - r * SS_IN;
        const int gy = ty0 + r, gx = tx0 + q;
        T a = (T)0, b = (T)0;
        if (gy < h && gx < w) {
            const int64_t at = base + ((int64_t)gy * w + gx) * c;
            a = x[at]; b = y[at];
        }
        s_x[e] = a; s_y[e] = b;
    }
    __syncthreads();
    for (int e = t; e < SS_IN * SS_TILE; e += IM_THREADS) {
        const int r = e / SS_TILE, q = e % SS_TILE;
        const T *ax = s_x + r * SS_IN + q, *ay = s_y + r * SS_IN + q;
        double a = (double)ax[0], b = (double)ay[0];
        double mx = win.g[0] * a, my = win.g[0] * b, exx = win.g[0] * (a * a), eyy = win.g[0] * (b * b), exy = win.g[0] * (a * b);
#pragma unroll
        for (int k = 1; k < SS_TAPS; k++) {
            a = (double)ax[k]; b = (double)ay[k];
            mx = mx + win.g[k] * a;
            my = my + win.g[k] * b;
            exx = exx + win.g[k] * (a * a);
            eyy = eyy + win.g[k] * (b * b);
            exy = exy + win.g[k] * (a * b);
        }
        s_m[0][r][q] = mx; s_m[1][r][q] = my; s_m[2][r][q] = exx; s_m[3][r][q] = eyy; s_m[4][r][q] = exy;
    }
    __syncthreads();
    const int oh = h - SS_APRON, ow = w - SS_APRON;
    double sum_ssim = 0.0, sum_cs = 0.0;
    for (int e = t; e < SS_TILE * SS_TILE; e += IM_THREADS) {
        const int r = e / SS_TILE, q = e % SS_TILE;
        const int oy = ty0 + r, ox = tx0 + q;
        if (oy < oh && ox < ow) {
            double mx = win.g[0] * s_m[0][r][q], my = win.g[0] * s_m[1][r][q], exx = win.g[0] * s_m[2][r][q], eyy = win.g[0] * s_m[3][r][q],
                   exy = win.g[0] * s_m[4][r][q];
#pragma unroll
            for (int k = 1; k < SS_TAPS; k++) {
                mx = mx + win.g[k] * s_m[0][r + k][q];
                my = my + win.g[k] * s_m[1][r + k][q];
                exx = exx + win.g[k] * s_m[2][r + k][q];
                eyy = eyy + win.g[k] * s_m[3][r + k][q];
                exy = exy + win.g[k] * s_m[4][r + k][q];
            }
            const double mxx = mx * mx, myy = my * my, mxy = mx * my;
            const double sxx = exx - mxx, syy = eyy - myy, sxy = exy - mxy;
            const double cs = (2.0 * sxy + c2) / ((sxx + syy) + c2);
            const double lum = (2.0 * mxy + c1) / ((mxx + myy) + c1);
            const double ssim = lum * cs;
            sum_ssim += ssim; sum_cs += cs;
            if (map) map[(((int64_t)img * oh + oy) * ow + ox) * c + ch] = ssim;
        }
    }
    double sums[2] = {sum_ssim, sum_cs};
    ordered_block_sum<IM_THREADS, 2>(sums, s_sum);
    if (t < 2) partials[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 + t] = t == 0 ? sums[0] : sums[1];
}

// out[i][v] = (the ordered sum over k of partials[i][k][v]) / count, v < NV: one block per i
template <int NV>
__global__ void __launch_bounds__(IM_THREADS) k_finish(int64_t per_image, const double *__restrict__ partials, double count, double *__restrict__ out)
{
    __shared__ double s_a[NV * IM_THREADS];
    double a[NV];
    ordered_finish<IM_THREADS, NV>(partials + (int64_t)blockIdx.x * per_image * NV, per_image, NV, 0, a, s_a);
    if (threadIdx.x < NV) out[(int64_t)blockIdx.x * NV + threadIdx.x] = (threadIdx.x == 0 ? a[0] : a[NV - 1]) / count;
}

// [b, h, w, c] -> [b, h / 2, w / 2, c] doubles, one lane per output element
template <class T> __global__ void __launch_bounds__(IM_THREADS) k_pool2(const T *__restrict__ in, int h, int w, int c, int64_t total, double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * IM_THREADS + threadIdx.x;
    if (i >= total) return;
    const int h2 = h >> 1, w2 = w >> 1;
    const int ch = (int)(i % c);
    int64_t r = i / c;
    const int px = (int)(r % w2); r /= w2;
    const int py = (int)(r % h2);
    const int64_t img = r / h2;
    const T *p = in + ((img * h + 2 * py) * w + 2 * px) * c + ch;
    const int64_t row = (int64_t)w * c;
    const double a00 = (double)p[0], a01 = (double)p[c], a10 = (double)p[row], a11 = (double)p[row + c];
    out[i] = ((a00 + a01) + (a10 + a11)) * 0.25;
}

__global__ void __launch_bounds__(IM_THREADS) k_mse(const float *__restrict__ x, const float *__restrict__ y, int64_t elems, double *__restrict__ partials)
{
    __shared__ double s_sum[IM_THREADS / 64];
    const int t = threadIdx.x;
    const int64_t img = blockIdx.y;
    const int64_t start = (int64_t)blockIdx.x * MSE_PER_BLOCK;
    const int64_t left = elems - start;
    const int cnt = left < MSE_PER_BLOCK ? (int)left : MSE_PER_BLOCK;
    const float *px = x + img * elems + start, *py = y + img * elems + start;
    double acc = 0.0;
    for (int e = t; e < cnt; e += IM_THREADS) {
        const double d = (double)px[e] - (double)py[e];
        acc += d * d;
    }
    acc = ordered_block_sum<IM_THREADS>(acc, s_sum);
    if (t == 0) partials[img * gridDim.x + blockIdx.x] = acc;
}

inline int64_t ssim_tiles(int h, int w) { return ceil_div(h - SS_APRON, SS_TILE) * ceil_div(w - SS_APRON, SS_TILE); }

// what every entry refuses about the images (the kernels index with these, so nothing is launched on a shape that fails here)
inline bool ssim_shape_ok(int b, int h, int w, int c)
{
    return b >= 1 && c >= 1 && c <= 4 && h >= SS_TAPS && w >= SS_TAPS && (int64_t)b * c <= 65535 && ssim_tiles(h, w) < ((int64_t)1 << 31) &&
           (int64_t)b * h * w * c < ((int64_t)1 << 40);
}

inline bool ms_shape_ok(int b, int h, int w, int c, int scales)
{
    return ssim_shape_ok(b, h, w, c) && scales >= 1 && scales <= MS_MAX_SCALES && ((h < w ? h : w) >> (scales - 1)) >= SS_TAPS;
}

struct SsimWs {
    double *partials;          // [b * c][tiles][2]
};

void ssim_layout(Bump &bp, int b, int h, int w, int c, SsimWs &ws) { ws.partials = bp.take<double>((size_t)b * c * ssim_tiles(h, w) * 2); }

struct MsSsimWs {
    double *px[MS_MAX_SCALES], *py[MS_MAX_SCALES];          // the pooled planes of scales 1 .. scales - 1 ([0] unused)
    SsimWs ssim;                                             // scale 0's partials; every further scale has fewer tiles and reuses them
};

void ms_ssim_layout(Bump &bp, int b, int h, int w, int c, int scales, MsSsimWs &ws)
{
    ws.px[0] = ws.py[0] = nullptr;
    for (int i = 1; i < MS_MAX_SCALES; i++) {
        if (i < scales) {
            const size_t n = (size_t)b * (h >> i) * (w >> i) * c;
            ws.px[i] = bp.take<double>(n);
            ws.py[i] = bp.take<double>(n);
        } else {
            ws.px[i] = ws.py[i] = nullptr;
        }
    }
    ssim_layout(bp, b, h, w, c, ws.ssim);
}

struct MseWs {
    double *partials;          // [b][blocks]
};

inline bool mse_shape_ok(int b, int64_t elems) { return b >= 1 && b <= 65535 && elems >= 1 && elems < ((int64_t)1 << 40); }

void mse_layout(Bump &bp, int b, int64_t elems, MseWs &ws) { ws.partials = bp.take<double>((size_t)b * ceil_div(elems, MSE_PER_BLOCK)); }

template <class T>
int ssim_launch(const T *x, const T *y, int b, int h, int w, int c, const SsimWindow &win, double c1, double c2, double *means, double *map, double *partials,
                hipStream_t st)
{
    const int tiles_x = (int)ceil_div(w - SS_APRON, SS_TILE);
    const int64_t tiles = ssim_tiles(h, w);
    hipLaunchKernelGGL(k_ssim<T>, dim3((unsigned)tiles, (unsigned)(b * c)), dim3(IM_THREADS), 0, st, x, y, h, w, c, tiles_x, win, c1, c2, map, partials);
    NRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_finish<2>, dim3((unsigned)(b * c)), dim3(IM_THREADS), 0, st, tiles, (const double *)partials,
                       (double)(h - SS_APRON) * (double)(w - SS_APRON), means);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

template <class T> int pool_launch(const T *in, int b, int h, int w, int c, double *out, hipStream_t st)
{
    const int64_t total = (int64_t)b * (h >> 1) * (w >> 1) * c;
    hipLaunchKernelGGL(k_pool2<T>, dim3((unsigned)ceil_div(total, IM_THREADS)), dim3(IM_THREADS), 0, st, in, h, w, c, total, out);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

inline bool range_ok(double data_range) { return std::isfinite(data_range) && data_range > 0.0; }

// ---- SSIM as a training loss: 1 - mean SSIM and its gradient with respect to x (nrf_ssim_loss; the operation order is in include/nerfpp_hip.h) ----
// k_ssim_loss<CT>: one workgroup of 256 lanes per 32 x 32 tile of the GRADIENT (= of the image) of one channel of one image, everything between the inputs and the
// gradient in LDS.  A gradient pixel p collects the coefficient maps at the valid pixels o = p - 10 .. p, and those need the inputs o .. o + 10: per axis the tile
// holds the coefficient pixels [max(g0 - 10, 0), min(g0 + 32, h - 10)) -- at most CT of them -- and 10 more input pixels.  Beyond that range the coefficient maps
// are the padded zeros of the definition: their taps are skipped (acc starts at 0.0 and takes the remaining taps in the order k = 0..10; 0.0 + a == a and a + 0.0 == a,
// so the values are the definition's).
//   CT = 42: the tiles of a large image (inputs 52 x 52).  LDS 21.6 KB inputs + 87.4 KB row-pass moments + 42.3 KB coefficient maps = 151.3 KB, one workgroup per CU.
//   CT = 22: a whole image of h, w <= 32 in one workgroup -- the training patches.  8.2 + 28.2 + 11.6 = 48.0 KB, three workgroups per CU.
//   1. inputs -> LDS;  2. row pass of the five moments (k_ssim's order);  3. column pass, the SSIM formula, A / B / Cc -> LDS, and the sum of ssim over the valid
//   pixels INSIDE the gradient tile (each valid pixel lies in exactly one);  4. transposed window along the column into the moments' LDS (dead by then);  5. along
//   the row, the combination with x and y, grad64 and the accumulation into g_x: one lane per element, no atomics.
//   The sums: the lane's, reduce.h's ordered block sum -> one fp64 partial per workgroup; k_ssim_loss_finish is the same finish pass as k_finish's.
constexpr int SL_CT_TILE = SS_TILE + SS_APRON, SL_CT_WHOLE = SS_TILE - SS_APRON;

inline int64_t ssim_loss_tiles(int h, int w) { return ceil_div(h, SS_TILE) * ceil_div(w, SS_TILE); }

inline bool ssim_loss_shape_ok(int b, int h, int w, int c) { return ssim_shape_ok(b, h, w, c) && ssim_loss_tiles(h, w) < ((int64_t)1 << 31); }

template <int CT>
__global__ void __launch_bounds__(IM_THREADS)
k_ssim_loss(const float *__restrict__ x, const float *__restrict__ y, int h, int w, int c, int tiles_x, SsimWindow win, double c1, double c2, double n_valid,
            double weight, float *__restrict__ g_x, double *__restrict__ grad64, double *__restrict__ partials)
{
    constexpr int IT = CT + SS_APRON, GT = SS_TILE;
    static_assert(3 * GT <= 5 * IT, "the column pass of the transposed window reuses the moments' LDS");
    __shared__ double s_m[5 * IT * CT];          // [5][IT][CT] moments after the row pass; from step 4 on [3][GT][CT]: T along the column
    __shared__ double s_c[3 * CT * CT];          // [3][CT][CT] A, B, Cc
    __shared__ float s_x[IT * IT], s_y[IT * IT];
    __shared__ double s_sum[IM_THREADS / 64];
    const int t = threadIdx.x;
    const int gy0 = (int)(blockIdx.x / (unsigned)tiles_x) * GT, gx0 = (int)(blockIdx.x % (unsigned)tiles_x) * GT;
    const int img = (int)(blockIdx.y / (unsigned)c), ch = (int)(blockIdx.y % (unsigned)c);
    const int64_t base = (int64_t)img * h * w * c + ch;
    const int oh = h - SS_APRON, ow = w - SS_APRON;
    const int cy0 = gy0 > SS_APRON ? gy0 - SS_APRON : 0, cx0 = gx0 > SS_APRON ? gx0 - SS_APRON : 0;
    const int n_cy = (gy0 + GT < oh ? gy0 + GT : oh) - cy0, n_cx = (gx0 + GT < ow ? gx0 + GT : ow) - cx0;          // 1 .. CT coefficient pixels per axis
    const int n_iy = n_cy + SS_APRON, n_ix = n_cx + SS_APRON;                                                      // input pixels: all inside the image
    const int n_gy = h - gy0 < GT ? h - gy0 : GT, n_gx = w - gx0 < GT ? w - gx0 : GT;
    for (int e = t; e < n_iy * n_ix; e += IM_THREADS) {
        const int r = e / n_ix, q = e - r * n_ix;
        const int64_t at = base + ((int64_t)(cy0 + r) * w + (cx0 + q)) * c;
        s_x[r * IT + q] = x[at]; s_y[r * IT + q] = y[at];
    }
    __syncthreads();
    for (int e = t; e < n_iy * n_cx; e += IM_THREADS) {
        const int r = e / n_cx, q = e - r * n_cx;
        const float *ax = s_x + r * IT + q, *ay = s_y + r * IT + q;
        double a = (double)ax[0], b = (double)ay[0];
        double mx = win.g[0] * a, my = win.g[0] * b, exx = win.g[0] * (a * a), eyy = win.g[0] * (b * b), exy = win.g[0] * (a * b);
#pragma unroll
        for (int k = 1; k < SS_TAPS; k++) {
            a = (double)ax[k]; b = (double)ay[k];
            mx = mx + win.g[k] * a;
            my = my + win.g[k] * b;
            exx = exx + win.g[k] * (a * a);
            eyy = eyy + win.g[k] * (b * b);
            exy = exy + win.g[k] * (a * b);
        }
        double *m = s_m + r * CT + q;
        m[0] = mx; m[IT * CT] = my; m[2 * IT * CT] = exx; m[3 * IT * CT] = eyy; m[4 * IT * CT] = exy;
    }
    __syncthreads();
    double sum_ssim = 0.0;
    for (int e = t; e < n_cy * n_cx; e += IM_THREADS) {
        const int r = e / n_cx, q = e - r * n_cx;
        const double *m = s_m + r * CT + q;
        double mx = win.g[0] * m[0], my = win.g[0] * m[IT * CT], exx = win.g[0] * m[2 * IT * CT], eyy = win.g[0] * m[3 * IT * CT], exy = win.g[0] * m[4 * IT * CT];
#pragma unroll
        for (int k = 1; k < SS_TAPS; k++) {
            mx = mx + win.g[k] * m[k * CT];
            my = my + win.g[k] * m[IT * CT + k * CT];
            exx = exx + win.g[k] * m[2 * IT * CT + k * CT];
            eyy = eyy + win.g[k] * m[3 * IT * CT + k * CT];
            exy = exy + win.g[k] * m[4 * IT * CT + k * CT];
        }
        const double mxx = mx * mx, myy = my * my, mxy = mx * my;
        const double sxx = exx - mxx, syy = eyy - myy, sxy = exy - mxy;
        const double cd = (sxx + syy) + c2, ld = (mxx + myy) + c1;
        const double cs = (2.0 * sxy + c2) / cd;
        const double lum = (2.0 * mxy + c1) / ld;
        const double ssim = lum * cs;
        if (cy0 + r >= gy0 && cx0 + q >= gx0) sum_ssim += ssim;
        double *co = s_c + r * CT + q;
        co[0] = cs * (2.0 * (my - lum * mx) / ld) + lum * (2.0 * (cs * mx - my) / cd);
        co[CT * CT] = -(ssim / cd);
        co[2 * CT * CT] = 2.0 * lum / cd;
    }
    sum_ssim = ordered_block_sum<IM_THREADS>(sum_ssim, s_sum);
    if (t == 0) partials[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = sum_ssim;
    for (int e = t; e < n_gy * n_cx; e += IM_THREADS) {
        const int gr = e / n_cx, q = e - gr * n_cx;
        const int r0 = gy0 + gr - cy0;          // the coefficient row of tap 0; tap k reads row r0 - k
        double ta = 0.0, tb = 0.0, tc = 0.0;
#pragma unroll
        for (int k = 0; k < SS_TAPS; k++) {
            const int r = r0 - k;
            if (r >= 0 && r < n_cy) {
                const double *co = s_c + r * CT + q;
                ta = ta + win.g[k] * co[0];
                tb = tb + win.g[k] * co[CT * CT];
                tc = tc + win.g[k] * co[2 * CT * CT];
            }
        }
        double *o = s_m + gr * CT + q;
        o[0] = ta; o[GT * CT] = tb; o[2 * GT * CT] = tc;
    }
    __syncthreads();
    for (int e = t; e < n_gy * n_gx; e += IM_THREADS) {
        const int gr = e / n_gx, gq = e - gr * n_gx;
        const int q0 = gx0 + gq - cx0;
        const double *row = s_m + gr * CT;
        double ta = 0.0, tb = 0.0, tc = 0.0;
#pragma unroll
        for (int k = 0; k < SS_TAPS; k++) {
            const int q = q0 - k;
            if (q >= 0 && q < n_cx) {
                ta = ta + win.g[k] * row[q];
                tb = tb + win.g[k] * row[GT * CT + q];
                tc = tc + win.g[k] * row[2 * GT * CT + q];
            }
        }
        const int li = (gy0 + gr - cy0) * IT + q0;
        const double xv = (double)s_x[li], yv = (double)s_y[li];
        const double g = -((ta + (2.0 * xv) * tb) + yv * tc) / n_valid;
        const int64_t at = base + ((int64_t)(gy0 + gr) * w + (gx0 + gq)) * c;
        if (grad64) grad64[at] = g;
        if (weight != 0.0) g_x[at] = g_x[at] + (float)(weight * g);
    }
}

// loss[1] = (the ordered sum of the partials) / n, loss[0] = 1 - loss[1]: one block
__global__ void __launch_bounds__(IM_THREADS) k_ssim_loss_finish(int64_t count, const double *__restrict__ partials, double n_valid, double *__restrict__ loss)
{
    __shared__ double s_a[IM_THREADS];
    const double total = ordered_finish<IM_THREADS>(partials, count, 1, 0, s_a);
    if (threadIdx.x == 0) {
        const double mean = total / n_valid;
        loss[1] = mean;
        loss[0] = 1.0 - mean;
    }
}

struct SsimLossWs {
    double *partials;          // [b * c][tiles]
};

void ssim_loss_layout(Bump &bp, int b, int h, int w, int c, SsimLossWs &ws) { ws.partials = bp.take<double>((size_t)b * c * ssim_loss_tiles(h, w)); }

}  // namespace

}  // namespace nrf

using namespace nrf;

extern "C" {

int nrf_ssim_window(double *out11)
{
    NRF_CHECK_ARG(out11, "nrf_ssim_window: null output");
    const SsimWindow w = ssim_window();
    for (int k = 0; k < SS_TAPS; k++) out11[k] = w.g[k];
    return NRF_OK;
}

size_t nrf_ssim_workspace_bytes(int b, int h, int w, int c)
{
    if (!ssim_shape_ok(b, h, w, c)) return 0;
    return measure([&](Bump &bp) { SsimWs ws; ssim_layout(bp, b, h, w, c, ws); });
}

int nrf_ssim(const float *d_x, const float *d_y, int b, int h, int w, int c, double data_range, double *d_means, double *d_map, void *d_workspace,
             size_t workspace_bytes, void *stream)
{
    NRF_CHECK_ARG(d_x && d_y && d_means && d_workspace, "nrf_ssim: null pointer");
    NRF_CHECK_ARG(ssim_shape_ok(b, h, w, c), "nrf_ssim: images [%d, %d, %d, %d]: b >= 1, h and w >= 11, c in 1..4, b * c <= 65535", b, h, w, c);
    NRF_CHECK_ARG(range_ok(data_range), "nrf_ssim: data_range must be finite and > 0");
    NRF_CHECK_ARG((reinterpret_cast<uintptr_t>(d_workspace) & 7) == 0, "nrf_ssim: the workspace must be 8-byte aligned");
    Bump bp(d_workspace, workspace_bytes);
    SsimWs ws;
    ssim_layout(bp, b, h, w, c, ws);
    NRF_TRY(ws_check(bp, nrf_ssim_workspace_bytes(b, h, w, c), "nrf_ssim"));
    const double k1 = 0.01 * data_range, k2 = 0.03 * data_range;
    return ssim_launch(d_x, d_y, b, h, w, c, ssim_window(), k1 * k1, k2 * k2, d_means, d_map, ws.partials, as_stream(stream));
}

size_t nrf_ssim_loss_workspace_bytes(int b, int h, int w, int c)
{
    if (!ssim_loss_shape_ok(b, h, w, c)) return 0;
    return measure([&](Bump &bp) { SsimLossWs ws; ssim_loss_layout(bp, b, h, w, c, ws); });
}

int nrf_ssim_loss(const float *d_x, const float *d_y, int b, int h, int w, int c, double data_range, double weight, double *d_loss, float *d_g_x, double *d_grad64,
                  void *d_workspace, size_t workspace_bytes, void *stream)
{
    NRF_CHECK_ARG(d_x && d_y && d_loss && d_g_x && d_workspace, "nrf_ssim_loss: null pointer");
    NRF_CHECK_ARG(ssim_loss_shape_ok(b, h, w, c), "nrf_ssim_loss: images [%d, %d, %d, %d]: b >= 1, h and w >= 11, c in 1..4, b * c <= 65535", b, h, w, c);
    NRF_CHECK_ARG(range_ok(data_range), "nrf_ssim_loss: data_range must be finite and > 0");
    NRF_CHECK_ARG(std::isfinite(weight) && weight >= 0.0, "nrf_ssim_loss: the weight must be finite and >= 0");
    NRF_CHECK_ARG((reinterpret_cast<uintptr_t>(d_workspace) & 7) == 0, "nrf_ssim_loss: the workspace must be 8-byte aligned");
    Bump bp(d_workspace, workspace_bytes);
    SsimLossWs ws;
    ssim_loss_layout(bp, b, h, w, c, ws);
    NRF_TRY(ws_check(bp, nrf_ssim_loss_workspace_bytes(b, h, w, c), "nrf_ssim_loss"));
    hipStream_t st = as_stream(stream);
    const double k1 = 0.01 * data_range, k2 = 0.03 * data_range;
    const double n_valid = (double)((int64_t)b * (h - SS_APRON) * (w - SS_APRON) * c);
    const SsimWindow win = ssim_window();
    const bool whole = h <= SS_TILE && w <= SS_TILE;          // one workgroup per image channel: the training patches
    const int tiles_x = whole ? 1 : (int)ceil_div(w, SS_TILE);
    const int64_t tiles = whole ? 1 : ssim_loss_tiles(h, w);
    if (whole)
        hipLaunchKernelGGL(k_ssim_loss<SL_CT_WHOLE>, dim3(1, (unsigned)(b * c)), dim3(IM_THREADS), 0, st, d_x, d_y, h, w, c, tiles_x, win, k1 * k1, k2 * k2, n_valid,
                           weight, d_g_x, d_grad64, ws.partials);
    else
        hipLaunchKernelGGL(k_ssim_loss<SL_CT_TILE>, dim3((unsigned)tiles, (unsigned)(b * c)), dim3(IM_THREADS), 0, st, d_x, d_y, h, w, c, tiles_x, win, k1 * k1,
                           k2 * k2, n_valid, weight, d_g_x, d_grad64, ws.partials);
    NRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ssim_loss_finish, dim3(1), dim3(IM_THREADS), 0, st, (int64_t)b * c * tiles, (const double *)ws.partials, n_valid, d_loss);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

size_t nrf_image_mse_workspace_bytes(int b, int64_t elems_per_image)
{
    if (!mse_shape_ok(b, elems_per_image)) return 0;
    return measure([&](Bump &bp) { MseWs ws; mse_layout(bp, b, elems_per_image, ws); });
}

int nrf_image_mse(const float *d_x, const float *d_y, int b, int64_t elems_per_image, double *d_mse, void *d_workspace, size_t workspace_bytes, void *stream)
{
    NRF_CHECK_ARG(d_x && d_y && d_mse && d_workspace, "nrf_image_mse: null pointer");
    NRF_CHECK_ARG(mse_shape_ok(b, elems_per_image), "nrf_image_mse: %d images of %lld elements: 1 <= b <= 65535, 1 <= elements < 2^40", b, (long long)elems_per_image);
    NRF_CHECK_ARG((reinterpret_cast<uintptr_t>(d_workspace) & 7) == 0, "nrf_image_mse: the workspace must be 8-byte aligned");
    Bump bp(d_workspace, workspace_bytes);
    MseWs ws;
    mse_layout(bp, b, elems_per_image, ws);
    NRF_TRY(ws_check(bp, nrf_image_mse_workspace_bytes(b, elems_per_image), "nrf_image_mse"));
    hipStream_t st = as_stream(stream);
    const int64_t blocks = ceil_div(elems_per_image, MSE_PER_BLOCK);
    hipLaunchKernelGGL(k_mse, dim3((unsigned)blocks, (unsigned)b), dim3(IM_THREADS), 0, st, d_x, d_y, elems_per_image, ws.partials);
    NRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_finish<1>, dim3((unsigned)b), dim3(IM_THREADS), 0, st, blocks, (const double *)ws.partials, (double)elems_per_image, d_mse);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

size_t nrf_ms_ssim_workspace_bytes(int b, int h, int w, int c, int scales)
{
    if (!ms_shape_ok(b, h, w, c, scales)) return 0;
    return measure([&](Bump &bp) { MsSsimWs ws; ms_ssim_layout(bp, b, h, w, c, scales, ws); });
}

int nrf_ms_ssim(const float *d_x, const float *d_y, int b, int h, int w, int c, double data_range, int scales, double *d_means, void *d_workspace,
                size_t workspace_bytes, void *stream)
{
    NRF_CHECK_ARG(d_x && d_y && d_means && d_workspace, "nrf_ms_ssim: null pointer");
    NRF_CHECK_ARG(ssim_shape_ok(b, h, w, c), "nrf_ms_ssim: images [%d, %d, %d, %d]: b >= 1, h and w >= 11, c in 1..4, b * c <= 65535", b, h, w, c);
    NRF_CHECK_ARG(ms_shape_ok(b, h, w, c, scales), "nrf_ms_ssim: %d scales of a %d x %d image: 1 <= scales <= 5 and min(h, w) >> (scales - 1) >= 11", scales, h, w);
    NRF_CHECK_ARG(range_ok(data_range), "nrf_ms_ssim: data_range must be finite and > 0");
    NRF_CHECK_ARG((reinterpret_cast<uintptr_t>(d_workspace) & 7) == 0, "nrf_ms_ssim: the workspace must be 8-byte aligned");
    Bump bp(d_workspace, workspace_bytes);
    MsSsimWs ws;
    ms_ssim_layout(bp, b, h, w, c, scales, ws);
    NRF_TRY(ws_check(bp, nrf_ms_ssim_workspace_bytes(b, h, w, c, scales), "nrf_ms_ssim"));
    hipStream_t st = as_stream(stream);
    const SsimWindow win = ssim_window();
    const double k1 = 0.01 * data_range, k2 = 0.03 * data_range;
    const double c1 = k1 * k1, c2 = k2 * k2;
    const int64_t per_scale = (int64_t)b * c * 2;
    NRF_TRY(ssim_launch(d_x, d_y, b, h, w, c, win, c1, c2, d_means, (double *)nullptr, ws.ssim.partials, st));
    for (int i = 1; i < scales; i++) {
        const int hp = h >> (i - 1), wp = w >> (i - 1);          // the size pooled FROM
        if (i == 1) {
            NRF_TRY(pool_launch(d_x, b, hp, wp, c, ws.px[1], st));
            NRF_TRY(pool_launch(d_y, b, hp, wp, c, ws.py[1], st));
        } else {
            NRF_TRY(pool_launch((const double *)ws.px[i - 1], b, hp, wp, c, ws.px[i], st));
            NRF_TRY(pool_launch((const double *)ws.py[i - 1], b, hp, wp, c, ws.py[i], st));
        }
        NRF_TRY(ssim_launch((const double *)ws.px[i], (const double *)ws.py[i], b, hp >> 1, wp >> 1, c, win, c1, c2, d_means + i * per_scale, (double *)nullptr,
                            ws.ssim.partials, st));
    }
    return NRF_OK;
}

}  // extern "C"
