// lerf_query.hip -- the LeRF relevancy in 3D: per point, lattice and (through the point entry) mesh vertex.  No counterpart in the reference, which reads the
// language field through rendered images only (LeRFRenderer::Render -> Relevancy); the formula is k_lerf_relevancy's (lerf_render.hip) on normalize(le(x)).
//
// NRF_PREC_F32: the composed path -- nrf_mlp_forward(F32) in chunks, the final normalise of RenderCLIPEmbedding, then the relevancy.  Any head.
// NRF_PREC_F16_SPLIT / F16_MFMA, per slab of points:
//   k_lattice_points (grid entry)            P(i, j, k) as nrf_density_grid
//   hash encode (CuHash L16 F8, level-major)  the language grid's fp16 features
//   sigma_le in EXACT fp32 (sigma_lerf_f32)  d_sigma (keep mask applied) and the (sigma, geo32) operand planes
//   k_lerf_query (mlp_lerf_split_mfma.hip)   LE0 -> a;  ||W a||^2 = a^T (W^T W) a (Gram layer);  d = U^T a;  relevancy in registers;  8 bytes per point
// The LeRF embedding layer W (256 -> 768) is bias-free, so q . (W a) = (W^T q) . a: U = W^T [positive; negatives] (256 x 32) is built in fp64 into the caller's
// workspace on EVERY call (prompts or weights changed since the last one are honoured; nothing is cached), scaled by a power of two into fp16 range and split
// hi / lo like k_lerf_fill.  The split image's LE0 and Gram fragments are copied beside it (480 KB): the kernel's weight stream walks one image.
#include "chunk_loop.h"
#include "mlp.h"
#include "mlp_lerf_net.h"
#include "reduce.h"
#include "stoch.h"

#include <cmath>

namespace nrf {

// lerf_render.hip: the parts of a LeRF renderer the query reads
void lerf_renderer_query_parts(const nrf_lerf_renderer *r, const nrf_hash **h, const nrf_mlp **m, const float **pos, int *n_pos, const float **neg, int *n_neg, int *embed_dim);

namespace {

using lerf::EMB;
using lerf::GEO;
using lerf::HID;
using lerf::IN;

constexpr int QSLOTS = 32;                                 // prompt slots of the U tile: the positive and up to 31 negatives
constexpr int64_t DEFAULT_SLAB = (int64_t)1 << 22;
constexpr int64_t MAX_SLAB = (int64_t)1 << 30;
constexpr int64_t MAX_LATTICE = (int64_t)1 << 36;
constexpr int64_t F32_CHUNK = (int64_t)1 << 14;            // points per nrf_mlp_forward(F32) call of the composed path ([chunk, 769] fp32 rows)
constexpr int64_t HEAD_SLAB = (int64_t)1 << 20;            // points per fused pass of the head entry (its feature planes live in the workspace)
constexpr size_t SPLIT_LE0_OFF = (size_t)2 * (8 * 8 + 2 * 16) * 1024;          // bytes of the split image before LE0 (sigma0, sigma1)
constexpr size_t SPLIT_COPY = (size_t)(lerf::QUERY_IMAGE_FRAGS - 2 * 16) * 1024; // LE0 + Gram fragments

// ---- the U tile ----
// U[j][k] = sum_o W[o][j] q_k[o] in double (four partial sums, as k_lerf_gram_f64); q_0 = positives[positive_id], q_k = negatives[k - 1] (k <= n_neg), 0 beyond
__global__ void __launch_bounds__(QSLOTS) k_query_proj_f64(const float *__restrict__ w3, const float *__restrict__ pos, const float *__restrict__ neg, int n_neg,
                                                            float *__restrict__ u, uint32_t *__restrict__ umax_bits)
{
    const int j = blockIdx.x, k = threadIdx.x;
    float v = 0.0f;
    if (k <= n_neg) {
        const float *q = k == 0 ? pos : neg + (size_t)(k - 1) * EMB;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        for (int o = 0; o + 4 <= EMB; o += 4) {
            s0 += (double)w3[(size_t)o * HID + j] * (double)q[o];
            s1 += (double)w3[(size_t)(o + 1) * HID + j] * (double)q[o + 1];
            s2 += (double)w3[(size_t)(o + 2) * HID + j] * (double)q[o + 2];
            s3 += (double)w3[(size_t)(o + 3) * HID + j] * (double)q[o + 3];
        }
        v = (float)((s0 + s1) + (s2 + s3));
    }
    u[(size_t)j * QSLOTS + k] = v;
    float mx = fabsf(v);
    mx = mx == mx ? mx : 0.0f;                             // a NaN entry does not decide the scale (it reaches the outputs through the image)
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 32));
    if (k == 0) atomicMax(umax_bits, __float_as_uint(mx));
}
static_assert(EMB % 4 == 0, "the projection's four partial sums cover EMB exactly");

// the U tile's 16 k-steps x (hi, lo) fragments: element (lane, j) of k-step ks multiplies chained operand index 32 (ks >> 1) + perm_row(ks & 1, lane >> 5, j) for prompt
// slot lane & 31 -- the Gram layer's operand order.  U is stored divided by 2^e, e chosen so that max|U| / 2^e lies in [512, 1024): no overflow, and the lo parts keep
// their bits above fp16's subnormal range for the small entries of a unit prompt.
__global__ void __launch_bounds__(512) k_query_fill(const float *__restrict__ u, const uint32_t *__restrict__ umax_bits, _Float16 *__restrict__ img, float *__restrict__ u_scale)
{
    const int f = blockIdx.x, e = threadIdx.x, lane = e >> 3, j = e & 7;
    const int ks = f >> 1, part = f & 1;
    const float gm = __uint_as_float(*umax_bits);
    int ex = 0;
    if (gm > 0.0f && gm <= 3.402823466e38f) (void)frexpf(gm / 1024.0f, &ex);
    const int row = 32 * (ks >> 1) + perm_row(ks & 1, lane >> 5, j);
    const float v = ldexpf(u[(size_t)row * QSLOTS + (lane & 31)], -ex);
    const _Float16 hv = (_Float16)v;
    img[(size_t)f * 512 + e] = part == 0 ? hv : (_Float16)(v - (float)hv);
    if (f == 0 && e == 0) *u_scale = ldexpf(1.0f, ex);
}

struct QueryImage {
    void *img;
    float *u, *u_scale;
    uint32_t *umax;
};

QueryImage take_image(Bump &b)
{
    QueryImage q;
    q.img = b.take<char>((size_t)lerf::QUERY_IMAGE_FRAGS * 1024);
    q.u = b.take<float>((size_t)HID * QSLOTS);
    q.umax = b.take<uint32_t>(1);
    q.u_scale = b.take<float>(1);
    return q;
}

int build_image(const nrf_mlp *m, const QueryImage &q, const float *pos, const float *neg, int n_neg, hipStream_t st)
{
    const float *w3 = m->params() + (size_t)HID * IN + (size_t)(1 + GEO) * HID + (size_t)HID * (GEO + IN);
    NRF_HIP(hipMemcpyAsync(q.img, m->d_packed_split.as<const char>() + SPLIT_LE0_OFF, SPLIT_COPY, hipMemcpyDeviceToDevice, st));
    NRF_HIP(hipMemsetAsync(q.umax, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_query_proj_f64, dim3(HID), dim3(QSLOTS), 0, st, w3, pos, neg, n_neg, q.u, q.umax);
    NRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_query_fill, dim3(32), dim3(512), 0, st, (const float *)q.u, (const uint32_t *)q.umax,
                       reinterpret_cast<_Float16 *>(static_cast<char *>(q.img) + SPLIT_COPY), q.u_scale);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

// ---- the composed F32 path ----
// k_lerf_relevancy's arithmetic (lerf_render.hip) with the phrases read from global memory: no bound on the number of negatives from an LDS phrase buffer
__global__ void __launch_bounds__(256) k_query_relevancy_f32(const float *__restrict__ emb, int64_t n, int e, const float *__restrict__ pos, const float *__restrict__ neg,
                                                           int q, float *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float *x = emb + row * (int64_t)e;
    float lp = 0.0f;
    for (int k = lane; k < e; k += 64) lp = __builtin_fmaf(x[k], pos[k], lp);
    lp = wave_sum(lp);
    float best0 = 0.0f, best1 = 0.0f;
    for (int j = 0; j < q; j++) {
        float ln = 0.0f;
        for (int k = lane; k < e; k += 64) ln = __builtin_fmaf(x[k], neg[(size_t)j * e + k], ln);
        ln = wave_sum(ln);
        const float a = 10.0f * lp, b = 10.0f * ln, m = fmaxf(a, b);
        const float ea = expf(a - m), eb = expf(b - m), sum = ea + eb;
        const float s0 = ea / sum, s1 = eb / sum;
        if (j == 0 || s0 < best0) { best0 = s0; best1 = s1; }
    }
    if (lane == 0) { out[row * 2 + 0] = best0; out[row * 2 + 1] = best1; }
}

// sigma_le = raw[:, col], 0 where the keep mask is false (LeRFRenderer.cpp:17-18)
__global__ void k_query_sigma_col(int64_t p, int stride, int col, const float *__restrict__ raw, const uint8_t *__restrict__ keep, float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p) return;
    out[i] = (keep && !keep[i]) ? 0.0f : raw[i * stride + col];
}

struct F32Bufs {
    float *raw, *emb, *ones, *x;
    uint8_t *keep;
    void *mws;
    size_t mws_bytes;
};
// rows: x_rows (head entry) or the features of points (point / grid entries: x == NULL here, encoded into bufs.x)
F32Bufs take_f32(const nrf_mlp *m, Bump &b, bool encode)
{
    F32Bufs f{};
    const int E = m->out_dims - 1;
    f.raw = b.take<float>((size_t)F32_CHUNK * m->out_dims);
    f.emb = b.take<float>((size_t)F32_CHUNK * E);
    f.ones = b.take<float>((size_t)F32_CHUNK);
    if (encode) { f.x = b.take<float>((size_t)F32_CHUNK * m->in_dims); f.keep = b.take<uint8_t>((size_t)F32_CHUNK); }
    f.mws_bytes = mlp_workspace_bytes(m, F32_CHUNK, NRF_PREC_F32);
    f.mws = b.take<char>(f.mws_bytes);
    return f;
}

// one chunk (<= F32_CHUNK rows) of the composed path: forward, sigma (optional), normalise + relevancy (optional)
int f32_chunk(const nrf_mlp *m, const float *x, const uint8_t *keep, int64_t c, const float *pos, const float *neg, int n_neg, float *sigma, float *rel,
              const F32Bufs &f, hipStream_t st)
{
    const int E = m->out_dims - 1, stride = m->out_dims;
    NRF_TRY(mlp_forward(m, x, m->in_dims, c, NRF_PREC_F32, f.raw, stride, f.mws, f.mws_bytes, st));
    if (sigma) {
        hipLaunchKernelGGL(k_query_sigma_col, dim3((unsigned)ceil_div(c, 256)), dim3(256), 0, st, c, stride, E, (const float *)f.raw, keep, sigma);
        NRF_LAUNCH_CHECK();
    }
    if (rel) {
        if (n_neg == 0) NRF_HIP(hipMemsetAsync(rel, 0, (size_t)c * 2 * sizeof(float), st));
        else {
            NRF_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(f.ones), 0x3f800000, (size_t)c, st));
            NRF_TRY(launch_clip_embedding(f.raw, stride, E, f.ones, c, 1, f.emb, st));          // normalize(le, eps 1e-8): RenderCLIPEmbedding's final step
            hipLaunchKernelGGL(k_query_relevancy_f32, dim3((unsigned)ceil_div(c, 4)), dim3(256), 0, st, (const float *)f.emb, c, E, pos, neg, n_neg, rel);
            NRF_LAUNCH_CHECK();
        }
    }
    return NRF_OK;
}

// ---- lattice ----
struct Grid {
    int nx, ny, nz;
    int64_t n;
    float bmin[3], step[3];
};
__global__ void k_query_lattice_points(Grid g, int64_t first, int64_t count, float *__restrict__ pts)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= count) return;
    const int64_t i = first + q, yz = i / g.nx;
    const int x = (int)(i - yz * g.nx), y = (int)(yz % g.ny), z = (int)(yz / g.ny);
    pts[q * 3 + 0] = g.bmin[0] + (float)x * g.step[0];          // nrf_density_grid's P = bmin + (float)i * step
    pts[q * 3 + 1] = g.bmin[1] + (float)y * g.step[1];
    pts[q * 3 + 2] = g.bmin[2] + (float)z * g.step[2];
}
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
        g.step[a] = (bbox[3 + a] - bbox[a]) / (float)(n[a] - 1);
    }
    return NRF_OK;
}

// head entry: fp32 feature rows -> level-major (hi, lo) fp16 planes [16][p][8] (feature 8 l + f of row i at (l * p + i) * 8 + f)
__global__ void k_query_rows_to_lm(int64_t p, const float *__restrict__ x, __half *__restrict__ hi, __half *__restrict__ lo)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= p * IN) return;
    const int64_t i = t / IN;
    const int c = (int)(t - i * IN), l = c >> 3, f = c & 7;
    const float v = x[t];
    const _Float16 h = (_Float16)v;
    const size_t o = ((size_t)l * p + i) * 8 + f;
    reinterpret_cast<_Float16 *>(hi)[o] = h;
    reinterpret_cast<_Float16 *>(lo)[o] = (_Float16)(v - (float)h);
}

bool fused_precision(int precision) { return precision == NRF_PREC_F16_SPLIT || precision == NRF_PREC_F16_MFMA; }

// the fused kernel's conditions (message names the call)
int fused_ok(const char *who, const nrf_mlp *m, int n_neg, bool need_exact)
{
    if (!lerf_split_available(m) || m->out_dims != EMB + 1) {
        set_error("%s: the fused query is built for the LeRF head of in 128 / hidden 256 / 2+2 layers / geo 32 / embedding 768 (NRF_PREC_F32 takes any head)", who);
        return NRF_ERR_UNSUPPORTED;
    }
    if (need_exact && !nrf_lerf_sigma_exact_available(m)) { set_error("%s: the exact-fp32 density pass is not available for this head (NRF_PREC_F32 takes any head)", who); return NRF_ERR_UNSUPPORTED; }
    if (1 + n_neg > QSLOTS) {
        set_error("%s: the fused query holds the positive and at most %d negatives in one 32-neuron tile (got %d negatives; NRF_PREC_F32 takes any number)", who, QSLOTS - 1, n_neg);
        return NRF_ERR_UNSUPPORTED;
    }
    return NRF_OK;
}

int64_t slab_of(int64_t slab_points, int64_t n)
{
    int64_t slab = slab_points > 0 ? slab_points : DEFAULT_SLAB;
    if (slab > MAX_SLAB) slab = MAX_SLAB;
    if (n > 0 && slab > n) slab = n;
    return slab < 1 ? 1 : slab;
}

// workspace of the point / grid entries for slabs of `slab` points
struct PointsWs {
    QueryImage qi;           // fused precisions: the prompt image, ...
    float *ptsb;             // a lattice's points (slab, or chunk of the composed path)
    __half *x;               // ... level-major fp16 features
    uint8_t *keep;
    float *sig;              // sigma_le (when the caller does not want it)
    void *geo;               // (sigma, geo32) planes
    F32Bufs f;               // NRF_PREC_F32: the composed path's buffers
};
PointsWs points_layout(Bump &b, const nrf_mlp *m, int precision, int64_t slab, bool lattice)
{
    PointsWs w{};
    if (fused_precision(precision)) {
        w.qi = take_image(b);
        if (lattice) w.ptsb = b.take<float>((size_t)slab * 3);
        w.x = b.take<__half>((size_t)slab * IN);
        w.keep = b.take<uint8_t>((size_t)slab);
        w.sig = b.take<float>((size_t)slab);
        w.geo = b.take<char>(nrf_lerf_geo_bytes(slab));
    } else {
        if (lattice) w.ptsb = b.take<float>((size_t)(slab < F32_CHUNK ? slab : F32_CHUNK) * 3);
        w.f = take_f32(m, b, true);
    }
    return w;
}
size_t points_ws(const nrf_mlp *m, int precision, int64_t slab, bool lattice)
{
    return measure([&](Bump &b) { points_layout(b, m, precision, slab, lattice); });
}

struct PointsCall {
    const nrf_hash *h;
    const nrf_mlp *m;
    const float *pos, *neg;
    int n_neg;
    int precision;
};

// the point pipeline over slabs; pts_of(first, cnt, buf) gives the slab's points (the caller's array, or the lattice written into buf)
template <class PtsOf>
int run_points(const char *who, const PointsCall &c, int64_t p, int64_t slab, bool lattice, PtsOf pts_of, float *d_sigma, float *d_rel, void *d_ws, size_t ws_bytes, hipStream_t st)
{
    Bump b(d_ws, ws_bytes);
    const PointsWs w = points_layout(b, c.m, c.precision, slab, lattice);
    NRF_TRY(ws_check(b, points_ws(c.m, c.precision, slab, lattice), who));
    float *const ptsb = w.ptsb;
    if (fused_precision(c.precision)) {
        const QueryImage &qi = w.qi;
        __half *x = w.x;
        uint8_t *keep = w.keep;
        float *sig_ws = w.sig;
        void *geo = w.geo;
        NRF_TRY(build_image(c.m, qi, c.pos, c.neg, c.n_neg, st));
        for (int64_t first = 0; first < p; first += slab) {
            const int64_t cnt = p - first < slab ? p - first : slab;
            const float *pts = pts_of(first, cnt, ptsb);
            if (!pts) return NRF_ERR_HIP;
            float *sig = d_sigma ? d_sigma + first : sig_ws;
            NRF_TRY(nrf_hash_encode_lm_f16_strided(c.h, pts, cnt, x, cnt, keep, st));
            NRF_TRY(nrf_lerf_sigma_exact_lm_strided(c.m, x, cnt, keep, cnt, sig, geo, cnt, st));
            lerf::QueryArgs a{};
            a.x_lm = x; a.x_lo = nullptr; a.pstride = cnt;
            a.geo = geo; a.geo_stride = cnt;
            a.u_scale = qi.u_scale; a.n_neg = c.n_neg; a.rel = d_rel + 2 * first;
            NRF_TRY(lerf_split_query(c.m, a, cnt, qi.img, c.precision == NRF_PREC_F16_SPLIT, st));
        }
        return NRF_OK;
    }
    const int64_t cs = slab < F32_CHUNK ? slab : F32_CHUNK;
    const F32Bufs &f = w.f;
    for (int64_t first = 0; first < p; first += cs) {
        const int64_t cnt = p - first < cs ? p - first : cs;
        const float *pts = pts_of(first, cnt, ptsb);
        if (!pts) return NRF_ERR_HIP;
        NRF_TRY(nrf_hash_encode(c.h, pts, cnt, f.x, f.keep, st));
        NRF_TRY(f32_chunk(c.m, f.x, f.keep, cnt, c.pos, c.neg, c.n_neg, d_sigma ? d_sigma + first : nullptr, d_rel + 2 * first, f, st));
    }
    return NRF_OK;
}

int renderer_prompts(const char *who, const nrf_lerf_renderer *r, int positive_id, PointsCall &c)
{
    int n_pos = 0, E = 0;
    lerf_renderer_query_parts(r, &c.h, &c.m, &c.pos, &n_pos, &c.neg, &c.n_neg, &E);
    NRF_CHECK_ARG(n_pos > 0, "%s: no prompts are set (nrf_lerf_set_prompts)", who);
    NRF_CHECK_ARG(positive_id >= 0 && positive_id < n_pos, "%s: positive_id %d outside the %d positive phrases", who, positive_id, n_pos);
    c.pos += (size_t)positive_id * E;
    return NRF_OK;
}

}  // namespace
}  // namespace nrf

using namespace nrf;

extern "C" {

namespace {
// workspace of the head entry: slabs of up to HEAD_SLAB rows in the fused precisions
struct HeadQueryWs {
    QueryImage qi;
    __half *xh, *xl;         // hi and lo feature planes
    float *sig_split;        // split sigma (discarded)
    void *geo;
    F32Bufs f;               // the composed path; in the fused precisions: sigma_le in fp32 (when wanted)
};
HeadQueryWs head_query_layout(Bump &b, const nrf_mlp *m, int64_t p, int precision)
{
    HeadQueryWs w{};
    if (fused_precision(precision)) {
        const int64_t hs = p < HEAD_SLAB ? p : HEAD_SLAB;
        w.qi = take_image(b);
        w.xh = b.take<__half>((size_t)hs * IN);
        w.xl = b.take<__half>((size_t)hs * IN);
        w.sig_split = b.take<float>((size_t)hs);
        w.geo = b.take<char>(nrf_lerf_geo_bytes(hs));
    }
    w.f = take_f32(m, b, false);
    return w;
}
}  // namespace

size_t nrf_lerf_head_relevancy_workspace_bytes(const nrf_mlp *m, int64_t p, int n_neg, int precision)
{
    (void)n_neg;
    if (!m || m->family != MLP_LERF || p <= 0) return 0;
    return measure([&](Bump &b) { head_query_layout(b, m, p, precision); });
}

int nrf_lerf_head_relevancy(const nrf_mlp *m, const float *d_x, int64_t p, const float *d_positives, int n_pos, const float *d_negatives, int n_neg, int positive_id,
                            int precision, float *d_sigma, float *d_relevancy, void *d_ws, size_t ws_bytes, void *stream)
{
    const char *who = "nrf_lerf_head_relevancy";
    NRF_CHECK_ARG(m && m->family == MLP_LERF, "%s: not a LeRF handle", who);
    NRF_CHECK_ARG(p >= 0 && n_neg >= 0 && n_pos >= 1 && positive_id >= 0 && positive_id < n_pos, "%s: need p >= 0, n_neg >= 0, 0 <= positive_id < n_pos (got p %lld, P %d, Q %d, id %d)",
                  who, (long long)p, n_pos, n_neg, positive_id);
    NRF_CHECK_ARG(d_relevancy, "%s: null relevancy output", who);
    NRF_CHECK_ARG(precision == NRF_PREC_F32 || fused_precision(precision), "%s: unknown precision %d", who, precision);
    if (fused_precision(precision)) NRF_TRY(fused_ok(who, m, n_neg, false));
    if (p == 0) return NRF_OK;
    NRF_CHECK_ARG(d_x && d_positives && (n_neg == 0 || d_negatives) && d_ws, "%s: null pointer", who);
    NRF_CHECK_ARG((reinterpret_cast<uintptr_t>(d_x) & 15) == 0, "%s: feature rows must be 16-byte aligned", who);
    Bump b(d_ws, ws_bytes);
    const HeadQueryWs w = head_query_layout(b, m, p, precision);
    NRF_TRY(ws_check(b, nrf_lerf_head_relevancy_workspace_bytes(m, p, n_neg, precision), who));
    hipStream_t st = as_stream(stream);
    const int E = m->out_dims - 1;
    const float *pos = d_positives + (size_t)positive_id * E;
    const F32Bufs &f = w.f;
    if (!fused_precision(precision)) {
        for (int64_t first = 0; first < p; first += F32_CHUNK) {
            const int64_t cnt = p - first < F32_CHUNK ? p - first : F32_CHUNK;
            NRF_TRY(f32_chunk(m, d_x + first * m->in_dims, nullptr, cnt, pos, d_negatives, n_neg, d_sigma ? d_sigma + first : nullptr, d_relevancy + 2 * first, f, st));
        }
        return NRF_OK;
    }
    const int64_t hs = p < HEAD_SLAB ? p : HEAD_SLAB;
    const QueryImage &qi = w.qi;
    __half *xh = w.xh, *xl = w.xl;
    float *sig_split = w.sig_split;
    void *geo = w.geo;
    NRF_TRY(build_image(m, qi, pos, d_negatives, n_neg, st));
    for (int64_t first = 0; first < p; first += hs) {
        const int64_t cnt = p - first < hs ? p - first : hs;
        const float *x = d_x + first * IN;
        hipLaunchKernelGGL(k_query_rows_to_lm, dim3((unsigned)ceil_div(cnt * IN, 256)), dim3(256), 0, st, cnt, x, xh, xl);
        NRF_LAUNCH_CHECK();
        // the (sigma, geo32) planes from fp32 rows: the split sigma net (kernel A); sigma_le itself comes from the F32 network below
        lerf::Args a{x, IN, nullptr, 0, nullptr, nullptr, sig_split, nullptr, 32};
        a.geo = geo; a.geo_stride = cnt;
        NRF_TRY(lerf_split_sigma(m, a, cnt, st));
        lerf::QueryArgs qa{};
        qa.x_lm = xh; qa.x_lo = xl; qa.pstride = cnt;
        qa.geo = geo; qa.geo_stride = cnt;
        qa.u_scale = qi.u_scale; qa.n_neg = n_neg; qa.rel = d_relevancy + 2 * first;
        NRF_TRY(lerf_split_query(m, qa, cnt, qi.img, precision == NRF_PREC_F16_SPLIT, st));
    }
    if (d_sigma)          // feature rows are not fp16 numbers in general: the exact-fp32 density pass (fp16 level-major input) does not apply; the F32 network does
        for (int64_t first = 0; first < p; first += F32_CHUNK) {
            const int64_t cnt = p - first < F32_CHUNK ? p - first : F32_CHUNK;
            NRF_TRY(f32_chunk(m, d_x + first * IN, nullptr, cnt, nullptr, nullptr, 0, d_sigma + first, nullptr, f, st));
        }
    return NRF_OK;
}

size_t nrf_lerf_point_relevancy_workspace_bytes(const nrf_lerf_renderer *r, int64_t p, int precision, int64_t slab_points)
{
    if (!r || p <= 0) return 0;
    PointsCall c{};
    int n_pos = 0, E = 0;
    lerf_renderer_query_parts(r, &c.h, &c.m, &c.pos, &n_pos, &c.neg, &c.n_neg, &E);
    return points_ws(c.m, precision, slab_of(slab_points, p), false);
}

int nrf_lerf_point_relevancy(const nrf_lerf_renderer *r, const float *d_pts, int64_t p, int positive_id, int precision, float *d_sigma, float *d_relevancy,
                             int64_t slab_points, void *d_ws, size_t ws_bytes, void *stream)
{
    const char *who = "nrf_lerf_point_relevancy";
    NRF_CHECK_ARG(r, "%s: null renderer", who);
    NRF_CHECK_ARG(p >= 0 && slab_points <= MAX_SLAB, "%s: need p >= 0 and slab_points <= 2^30", who);
    NRF_CHECK_ARG(precision == NRF_PREC_F32 || fused_precision(precision), "%s: unknown precision %d", who, precision);
    PointsCall c{};
    NRF_TRY(renderer_prompts(who, r, positive_id, c));
    NRF_CHECK_ARG(d_relevancy, "%s: null relevancy output", who);
    c.precision = precision;
    if (fused_precision(precision)) NRF_TRY(fused_ok(who, c.m, c.n_neg, true));
    if (p == 0) return NRF_OK;
    NRF_CHECK_ARG(d_pts && d_ws, "%s: null pointer", who);
    const int64_t slab = slab_of(slab_points, p);
    auto pts_of = [&](int64_t first, int64_t, float *) -> const float * { return d_pts + first * 3; };
    return run_points(who, c, p, slab, false, pts_of, d_sigma, d_relevancy, d_ws, ws_bytes, as_stream(stream));
}

size_t nrf_lerf_relevancy_grid_workspace_bytes(const nrf_lerf_renderer *r, int nx, int ny, int nz, int precision, int64_t slab_points)
{
    if (!r || nx < 2 || ny < 2 || nz < 2) return 0;
    PointsCall c{};
    int n_pos = 0, E = 0;
    lerf_renderer_query_parts(r, &c.h, &c.m, &c.pos, &n_pos, &c.neg, &c.n_neg, &E);
    return points_ws(c.m, precision, slab_of(slab_points, (int64_t)nx * ny * nz), true);
}

int nrf_lerf_relevancy_grid(const nrf_lerf_renderer *r, const float *bbox, int nx, int ny, int nz, int positive_id, int precision, float *d_sigma, float *d_relevancy,
                            int64_t slab_points, void *d_ws, size_t ws_bytes, void *stream)
{
    const char *who = "nrf_lerf_relevancy_grid";
    NRF_CHECK_ARG(r, "%s: null renderer", who);
    NRF_CHECK_ARG(slab_points <= MAX_SLAB, "%s: slab_points %lld above 2^30", who, (long long)slab_points);
    NRF_CHECK_ARG(precision == NRF_PREC_F32 || fused_precision(precision), "%s: unknown precision %d", who, precision);
    PointsCall c{};
    NRF_TRY(renderer_prompts(who, r, positive_id, c));
    NRF_CHECK_ARG(d_relevancy, "%s: null relevancy output", who);
    c.precision = precision;
    Grid g;
    NRF_TRY(make_grid(who, bbox, nx, ny, nz, g));
    if (fused_precision(precision)) NRF_TRY(fused_ok(who, c.m, c.n_neg, true));
    NRF_CHECK_ARG(d_ws, "%s: null workspace", who);
    const int64_t slab = slab_of(slab_points, g.n);
    hipStream_t st = as_stream(stream);
    auto pts_of = [&](int64_t first, int64_t cnt, float *buf) -> const float * {
        hipLaunchKernelGGL(k_query_lattice_points, dim3((unsigned)ceil_div(cnt, 256)), dim3(256), 0, st, g, first, cnt, buf);
        if (hipGetLastError() != hipSuccess) { set_error("%s: k_query_lattice_points launch failed", who); return nullptr; }
        return buf;
    };
    return run_points(who, c, g.n, slab, true, pts_of, d_sigma, d_relevancy, d_ws, ws_bytes, st);
}

}  // extern "C"
