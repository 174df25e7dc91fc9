// normals.hip -- surface normals from the analytic gradient of the density field: d sigma / d x of a hash grid (either encoder) followed by NeRFSmall's sigma net,
// and the per-ray compositing of density and predicted normals.  The reference meant to add them (NeRFExecutorParams::calculate_normals / use_pred_normal,
// NeRFRenderer.h's commented RenderedNormals) and never did; the contract is stated in include/nerfpp_hip.h (nrf_density_grad, nrf_render_normals).
//
// k_density_grad: one lane per point, forward mode.
//   Encoder: per level, the cell the forward pass chooses (floorf of the fp32 scaled position, formed as k_hash_cu / k_hash_ngp form it), the features of that
//   lookup -- CuHashEmbedder: the fp32 blend of cu_blend rounded once to fp16, HashEmbedder: k_hash_ngp's fp32 interpolation -- and their position derivative, the
//   derivative of the UNROUNDED fp32 blend: per axis the fp32 differences of the corner features times the other two weights, times d(weight)/dx.  CuHash:
//   mul_l / (max - min), 0 on an axis the clamp moved (CuHashEmbedder.cpp:92-94); NGP: 1 / (vmax - vmin) (NeRF.cpp:311 interpolates with the unclamped x; floor
//   contributes nothing), what torch autograd of HashEmbedderImpl::forward gives.
//   Sigma net: the primal in the arithmetic of NRF_PREC_F32 (mlp.hip k_linear: an fmaf chain in ascending k from 0, ReLU as v < 0 ? 0 : v), so sigma, every ReLU
//   mask and the keep mask equal NRF_PREC_F32's bit for bit; the tangent runs beside it through the same weights as a second fmaf chain, zeroed where the primal's
//   pre-activation is <= 0 (torch's relu backward).  grad = row 0 of the last layer applied to the tangents.  Sigma is replaced by 0 (and its gradient with it)
//   where k_mask_sigma would do it: outside the box with a 4-column net (the mask writes column -1; a 7-column net with the predicted-normals head keeps sigma).
//   The three tangents go one axis per pass beside a recomputed primal (the same chain, the same bits): a (primal, tangent) pair per neuron is one v_pk_fma_f32 with
//   a broadcast weight, and the hidden layer of a pass -- 64 pairs -- stays in registers.  The features' derivatives wait in LDS between passes (384 B per lane).
//   Weights are read as wave-uniform scalars from the network's fp32 blob.
// k_normals_composite: one lane per ray, sum_i w_i * safe_normalize(v_i) (v / max(|v|, 1e-8) in fp32, NeRFRenderer.h:311) in ascending sample order, summed in
//   fp64 and rounded once; a sample with w_i == 0 is skipped (it contributes exactly 0).
#include "encode.h"
#include "mlp.h"

namespace nrf {

namespace {

constexpr int NG_THREADS = 128;
constexpr int NG_IN = 32;          // input_ch of the built family (levels x features)
constexpr int NG_HID = 64;

typedef float ng_f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ ng_f2 pk_fma(float w, ng_f2 x, ng_f2 acc) { return __builtin_elementwise_fma(ng_f2{w, w}, x, acc); }

// features of level l and their derivatives (df[j][a] = d feature j / d x_a), the encoders' own arithmetic for the features
template <int F, bool CU>
__device__ __forceinline__ void level_grad(const HashParams &hp, int l, const float x[3], float f[F], float df[F][3])
{
    float wt[3], dw[3];
    float v[8][F];
    if constexpr (CU) {
        uint32_t pos[3];
        const float mul = hp.level_scale[l];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const float c = fmaxf(fminf(x[a], hp.bbox.mx[a]), hp.bbox.mn[a]);
            const float ext = hp.bbox.mx[a] - hp.bbox.mn[a];
            float q = (c - hp.bbox.mn[a]) / ext * mul;
            q = q + hp.bias[l * 3 + a];
            const float fl = floorf(q);
            pos[a] = (uint32_t)fl;
            wt[a] = q - fl;
            dw[a] = x[a] == c ? mul / ext : 0.0f;
        }
        const uint32_t pa = hp.primes[l * 3 + 0], pb = hp.primes[l * 3 + 1], pc = hp.primes[l * 3 + 2];
        const uint32_t lsz = hp.local_size[l];
        const bool pow2 = (lsz & (lsz - 1u)) == 0u;
        const __half *fp = reinterpret_cast<const __half *>(hp.table) + hp.local_idx[l];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t hv = (pos[0] + ((k >> 2) & 1u)) * pa ^ (pos[1] + ((k >> 1) & 1u)) * pb ^ (pos[2] + (k & 1u)) * pc;
            const uint32_t e = pow2 ? (hv & (lsz - 1u)) : (hv % lsz);
#pragma unroll
            for (int j = 0; j < F; j++) v[k][j] = __half2float(fp[(size_t)e * F + j]);
        }
        // cu_blend: three-factor weights, fp32 sum of products in corner order, one fp16 rounding
        const float a = wt[0], b = wt[1], c = wt[2], oma = 1.0f - a, omb = 1.0f - b, omc = 1.0f - c;
        float ws[8];
#pragma unroll
        for (int k = 0; k < 8; k++) ws[k] = ((k & 4) ? a : oma) * ((k & 2) ? b : omb) * ((k & 1) ? c : omc);
#pragma unroll
        for (int j = 0; j < F; j++) {
            float s = ws[0] * v[0][j];
#pragma unroll
            for (int k = 1; k < 8; k++) s = s + ws[k] * v[k][j];
            f[j] = __half2float(__float2half_rn(s));
            const float gx = omb * omc * (v[4][j] - v[0][j]) + omb * c * (v[5][j] - v[1][j]) + b * omc * (v[6][j] - v[2][j]) + b * c * (v[7][j] - v[3][j]);
            const float gy = oma * omc * (v[2][j] - v[0][j]) + oma * c * (v[3][j] - v[1][j]) + a * omc * (v[6][j] - v[4][j]) + a * c * (v[7][j] - v[5][j]);
            const float gz = oma * omb * (v[1][j] - v[0][j]) + oma * b * (v[3][j] - v[2][j]) + a * omb * (v[5][j] - v[4][j]) + a * b * (v[7][j] - v[6][j]);
            df[j][0] = gx * dw[0]; df[j][1] = gy * dw[1]; df[j][2] = gz * dw[2];
        }
    } else {
        int32_t idx[3];
        const float res = hp.level_scale[l];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const float c = fmaxf(fminf(x[a], hp.bbox.mx[a]), hp.bbox.mn[a]);
            const float grid = (hp.bbox.mx[a] - hp.bbox.mn[a]) / res;
            const float fl = floorf((c - hp.bbox.mn[a]) / grid);
            idx[a] = (int32_t)fl;
            const float vmin = fl * grid + hp.bbox.mn[a];
            const float vmax = vmin + grid;
            wt[a] = (x[a] - vmin) / (vmax - vmin);
            dw[a] = 1.0f / (vmax - vmin);
        }
        const float *tl = reinterpret_cast<const float *>(hp.table) + (int64_t)l * ((int64_t)1 << hp.log2_t) * F;
        const uint32_t hmask = (1u << hp.log2_t) - 1u;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t cx = (uint32_t)idx[0] + ((k >> 2) & 1), cy = (uint32_t)idx[1] + ((k >> 1) & 1), cz = (uint32_t)idx[2] + (k & 1);
            const uint32_t h = (cx ^ (cy * 2654435761u) ^ (cz * 805459861u)) & hmask;
#pragma unroll
            for (int j = 0; j < F; j++) v[k][j] = tl[(int64_t)h * F + j];
        }
        const float wx = wt[0], wy = wt[1], wz = wt[2], omx = 1.0f - wx, omy = 1.0f - wy, omz = 1.0f - wz;
#pragma unroll
        for (int j = 0; j < F; j++) {
            const float c00 = v[0][j] * omx + v[4][j] * wx, c01 = v[1][j] * omx + v[5][j] * wx;
            const float c10 = v[2][j] * omx + v[6][j] * wx, c11 = v[3][j] * omx + v[7][j] * wx;
            const float c0 = c00 * omy + c10 * wy, c1 = c01 * omy + c11 * wy;
            f[j] = c0 * omz + c1 * wz;
            const float gx = ((v[4][j] - v[0][j]) * omy + (v[6][j] - v[2][j]) * wy) * omz + ((v[5][j] - v[1][j]) * omy + (v[7][j] - v[3][j]) * wy) * wz;
            const float gy = (c10 - c00) * omz + (c11 - c01) * wz;
            const float gz = c1 - c0;
            df[j][0] = gx * dw[0]; df[j][1] = gy * dw[1]; df[j][2] = gz * dw[2];
        }
    }
}

// w0 [64][32], w1 [64][64] (NL == 3), wl: row 0 of the last layer [64] -- the blob's [out][in] blocks
template <int F, bool CU, int NL>
__global__ void __launch_bounds__(NG_THREADS) k_density_grad(HashParams hp, PointSource ps, int64_t p, const float *__restrict__ wsel, const float *__restrict__ w0,
                                                             const float *__restrict__ w1, const float *__restrict__ wl, int mask_keep, float *__restrict__ sigma,
                                                             float *__restrict__ grad)
{
    __shared__ float sdf[NG_IN * 3 * NG_THREADS];          // [k][axis][lane]: the features' derivatives between the passes
    const int t = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * NG_THREADS + t;
    if (i >= p) return;
    if (wsel && wsel[i] == 0.0f) return;                    // a render's zero-weight sample: nothing reads its gradient
    const F3 pt = load_point(ps, i);
    const float x[3] = {pt.x, pt.y, pt.z};
    bool kp = true;
#pragma unroll
    for (int a = 0; a < 3; a++) kp = kp && (x[a] == fmaxf(fminf(x[a], hp.bbox.mx[a]), hp.bbox.mn[a]));
    float f[NG_IN];
    constexpr int L = NG_IN / F;
#pragma unroll
    for (int l = 0; l < L; l++) {
        float fl[F], dfl[F][3];
        level_grad<F, CU>(hp, l, x, fl, dfl);
#pragma unroll
        for (int j = 0; j < F; j++) {
            f[l * F + j] = fl[j];
#pragma unroll
            for (int a = 0; a < 3; a++) sdf[((l * F + j) * 3 + a) * NG_THREADS + t] = dfl[j][a];
        }
    }
    const bool zero = mask_keep && !kp;                     // NeRFRenderer.h:187-188 on a 4-column net
    float sig = 0.0f;
#pragma unroll 1
    for (int a = 0; a < 3; a++) {
        ng_f2 in[NG_IN];
#pragma unroll
        for (int k = 0; k < NG_IN; k++) in[k] = ng_f2{f[k], sdf[(k * 3 + a) * NG_THREADS + t]};
        ng_f2 out = {0.0f, 0.0f};
        auto relu2 = [](ng_f2 z) -> ng_f2 { return ng_f2{z.x < 0.0f ? 0.0f : z.x, z.x > 0.0f ? z.y : 0.0f}; };
        if constexpr (NL == 2) {
#pragma unroll 4
            for (int o = 0; o < NG_HID; o++) {
                ng_f2 z = {0.0f, 0.0f};
#pragma unroll
                for (int k = 0; k < NG_IN; k++) z = pk_fma(w0[o * NG_IN + k], in[k], z);
                out = pk_fma(wl[o], relu2(z), out);
            }
        } else {
            ng_f2 h[NG_HID];
#pragma unroll
            for (int o = 0; o < NG_HID; o++) {
                ng_f2 z = {0.0f, 0.0f};
#pragma unroll
                for (int k = 0; k < NG_IN; k++) z = pk_fma(w0[o * NG_IN + k], in[k], z);
                h[o] = relu2(z);
            }
#pragma unroll 2
            for (int j = 0; j < NG_HID; j++) {
                ng_f2 z = {0.0f, 0.0f};
#pragma unroll
                for (int o = 0; o < NG_HID; o++) z = pk_fma(w1[j * NG_HID + o], h[o], z);
                out = pk_fma(wl[j], relu2(z), out);
            }
        }
        if (a == 0) sig = out.x;
        if (grad) grad[i * 3 + a] = zero ? 0.0f : out.y;
    }
    if (sigma) sigma[i] = zero ? 0.0f : sig;
}

template <int F, bool CU>
int launch_grad_f(const nrf_hash *h, const nrf_mlp *m, const PointSource &ps, int64_t p, const float *wsel, float *sigma, float *grad, hipStream_t st)
{
    const int nl = m->small.num_layers;
    const float *w0 = m->params() + m->layers[0].w_off;
    const float *w1 = nl == 3 ? m->params() + m->layers[1].w_off : nullptr;
    const float *wl = m->params() + m->layers[nl - 1].w_off;
    const int mask_keep = m->out_dims == 4 ? 1 : 0;
    // bounded launches: a grid of at most 2^24 blocks per launch
    const int64_t slab = (int64_t)NG_THREADS << 24;
    for (int64_t p0 = 0; p0 < p; p0 += slab) {
        const int64_t c = p - p0 < slab ? p - p0 : slab;
        PointSource q = ps;
        const float *ws = wsel ? wsel + p0 : nullptr;
        float *sg = sigma ? sigma + p0 : nullptr, *gr = grad ? grad + p0 * 3 : nullptr;
        if (q.pts) q.pts += p0 * 3;
        else if (p0) { set_error("internal: density gradient over ray samples in more than one launch"); return NRF_ERR_INVALID_ARG; }
        const dim3 grid((unsigned)ceil_div(c, NG_THREADS));
        if (nl == 3) hipLaunchKernelGGL((k_density_grad<F, CU, 3>), grid, dim3(NG_THREADS), 0, st, h->params, q, c, ws, w0, w1, wl, mask_keep, sg, gr);
        else hipLaunchKernelGGL((k_density_grad<F, CU, 2>), grid, dim3(NG_THREADS), 0, st, h->params, q, c, ws, w0, w1, wl, mask_keep, sg, gr);
        NRF_LAUNCH_CHECK();
    }
    return NRF_OK;
}

__global__ void k_normals_composite(int64_t n, int s, const float *__restrict__ v, int v_stride, int v_col, const int32_t *__restrict__ src, float sign,
                                    const float *__restrict__ weights, float *__restrict__ out)
{
    const int64_t ray = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ray >= n) return;
    double ax = 0.0, ay = 0.0, az = 0.0;          // fp64 sum: the result is the exact composite of the fp32 unit vectors, rounded once
    for (int j = 0; j < s; j++) {
        const int64_t i = ray * s + j;
        const float w = weights[i];
        if (w == 0.0f) continue;
        const float *q = v + (src ? (int64_t)src[i] : i) * v_stride + v_col;
        const float x = q[0], y = q[1], z = q[2];
        const float d = fmaxf(sqrtf(x * x + y * y + z * z), 1e-8f);
        ax = ax + (double)w * (double)(sign * x / d);
        ay = ay + (double)w * (double)(sign * y / d);
        az = az + (double)w * (double)(sign * z / d);
    }
    out[ray * 3 + 0] = (float)ax; out[ray * 3 + 1] = (float)ay; out[ray * 3 + 2] = (float)az;
}

}  // namespace

const char *density_grad_unsupported(const nrf_hash *h, const nrf_mlp *m)
{
    if (!h) return "density gradients are built for hash-grid renderers (CuHashEmbedder / HashEmbedder + NeRFSmall); this renderer has a sinusoidal position encoder";
    if (!m || m->family != MLP_SMALL) return "density gradients are built for NeRFSmall networks; this renderer's network is another family";
    const auto &d = m->small;
    if (d.input_ch != NG_IN || h->desc.n_levels * h->desc.n_features != NG_IN || d.hidden_dim != NG_HID || (d.num_layers != 2 && d.num_layers != 3))
        return "density gradients are built for NeRFSmall with 32 hash features, hidden_dim 64 and 2 or 3 sigma-net layers";
    return nullptr;
}

int density_grad_launch(const nrf_hash *h, const nrf_mlp *m, const PointSource &ps, int64_t p, const float *wsel, float *sigma, float *grad, hipStream_t st)
{
    if (const char *why = density_grad_unsupported(h, m)) { set_error("%s", why); return NRF_ERR_UNSUPPORTED; }
    if (p <= 0) return NRF_OK;
    if (!h->table_set) { set_error("hash grid: table not uploaded (nrf_hash_set_table)"); return NRF_ERR_INVALID_ARG; }
    if (h->desc.mode == NRF_HASH_CU && !h->primes_set) { set_error("hash grid (CU mode): primes not set (nrf_hash_set_primes)"); return NRF_ERR_INVALID_ARG; }
    const bool cu = h->desc.mode == NRF_HASH_CU;
    switch (h->desc.n_features) {
        case 1: return cu ? launch_grad_f<1, true>(h, m, ps, p, wsel, sigma, grad, st) : launch_grad_f<1, false>(h, m, ps, p, wsel, sigma, grad, st);
        case 2: return cu ? launch_grad_f<2, true>(h, m, ps, p, wsel, sigma, grad, st) : launch_grad_f<2, false>(h, m, ps, p, wsel, sigma, grad, st);
        case 4: return cu ? launch_grad_f<4, true>(h, m, ps, p, wsel, sigma, grad, st) : launch_grad_f<4, false>(h, m, ps, p, wsel, sigma, grad, st);
        default: return cu ? launch_grad_f<8, true>(h, m, ps, p, wsel, sigma, grad, st) : launch_grad_f<8, false>(h, m, ps, p, wsel, sigma, grad, st);
    }
}

int normals_composite(int64_t n, int s, const float *v, int v_stride, int v_col, const int32_t *src, float sign, const float *weights, float *out, hipStream_t st)
{
    if (n <= 0) return NRF_OK;
    hipLaunchKernelGGL(k_normals_composite, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, n, s, v, v_stride, v_col, src, sign, weights, out);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

}  // namespace nrf
