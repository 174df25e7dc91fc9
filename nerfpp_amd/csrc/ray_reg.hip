// ray_reg.hip -- two regularisers on how density is distributed along a ray, added to the training step's d loss / d raw[..., 3]:
//   the distortion loss of mip-NeRF 360 (Barron et al. 2022, eq. 15) on the render's weights, and the reference's SigmaSparsityLoss (NeRF.h:302-306: a Cauchy loss
//   log(1 + 2 sigma^2) summed along the ray, declared there and never called).  Both are functions of one ray's (sigma_i, w_i, z_i) only.
//
// k_ray_reg: one wave per ray, four rays per block (k_raw2outputs_bwd's shape), 64-sample blocks walked forwards and then backwards.
//   Forward quantities: alpha_i, T_i, w_i are recomputed from raw, z, |d| and the optional noise draws exactly as k_raw2outputs<false> / k_raw2outputs_bwd do (nrf_expf /
//   nrf_logf, the double wave scan of log(max(1 - alpha, 1e-10)) rounded to fp32 per prefix, last interval 1e10): weights_out, when given, is the render's Weights bit for bit.
//   Normalised depths t_i = (z_i - z_0) / (z_{s-1} - z_0); sample i owns [t_i, t_{i+1}] (what its alpha integrates over): m_i = (t_i + t_{i+1}) / 2, dl_i = t_{i+1} - t_i;
//   the last sample (the 1e10 tail has no finite extent) m = t_{s-1}, dl = 0.  A ray whose span is not > 0 (a missed ray, s == 1) is skipped: no loss, no store.
//     L_dist   = mean over rays of [ sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 dl_i ]
//              = mean of [ 2 sum_i w_i (M_{>i} - m_i W_{>i}) + ... ]   (m ascends with z; W, M: sums of w and of w m over the samples after / before i)
//     dL/dw_i  = 2 (m_i W_{<i} - M_{<i} + M_{>i} - m_i W_{>i}) + (2/3) w_i dl_i                (z carries no gradient: z_samples are detached, NeRFRenderer.h:429)
//     L_sparse = mean over rays of sum_i log(1 + 2 sp_i^2), sp_i = max(raw[i,3], 0) (the density compositing uses, without the noise draw); d/d raw = 4 sp / (1 + 2 sp^2)
//   W_{>i}, M_{>i} come from a reverse wave scan in fp64 per block (blocks walked last to first, as the chain below needs them anyway); W_{<i} = W_total - w_i - W_{>i} in
//   fp64 with the totals of the forward walk: the two halves of dL/dw_i cancel where the weight sits in a few neighbouring samples, and fp64 keeps that difference exact to
//   fp32's eye, which an fp32 prefix row read back from memory would not.  So the per-ray scratch row holds the exclusive log-transmittance only (4 B per sample).
//   Chain dL/dw -> raw[..., 3]: k_raw2outputs_bwd's, with gw_i := distortion_weight * dL_dist/dw_i / n -- TruncExp's clamped derivatives, the 1 - alpha >= 1e-10 guard,
//   the relu mask on sigma + noise, the reverse suffix scan of g_L.  The sparsity term is added to it and the sum is ADDED to g_raw[..., 3]; no other column is read or written.
//   Sums: per lane fp64, reduce.h's ordered block sum -> one fp64 pair per block; its k_finish_loss_pair (one block) is the ordered finish pass over the pairs.  No
//   atomics: two runs give the same bits.
#include "reduce.h"

#include <cmath>

namespace nrf {

namespace {

constexpr int RR_RAYS = 4;          // waves (rays) per block
constexpr int RR_FIN = 256;

__global__ void __launch_bounds__(64 * RR_RAYS)
k_ray_reg(int64_t n, int s, int c, const float *__restrict__ raw, const float *__restrict__ z, const float *__restrict__ dirs, int d_stride, const float *__restrict__ noise,
          float noise_std, float k_dist /* distortion_weight / n */, float k_sparse /* sparsity_weight / n */, int terms /* bit 0: distortion, bit 1: sparsity */, float *__restrict__ g_raw,
          float *__restrict__ weights_out, float *__restrict__ lt_scratch /* [n, s] exclusive log-transmittance */, double *__restrict__ partials /* [blocks][2] */)
{
    __shared__ double s_sum[2 * RR_RAYS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t ray = (int64_t)blockIdx.x * RR_RAYS + wv;
    double l_dist = 0.0, l_sparse = 0.0;
    if (ray < n) {                                                    // (wave-uniform; no early return: the block meets at the barrier below)
        const float *zr = z + ray * s;
        const float z0 = zr[0];
        const float span = zr[s - 1] - z0;
        const bool on = span > 0.0f;                                  // a missed ray (far = near + 1e-6 rounds to near) or s == 1: contributes nothing
        const bool dist_on = on && (terms & 1), sparse_on = on && (terms & 2);
        float nrm = 0.0f;
        double w_tot = 0.0, m_tot = 0.0;
        float *lt = lt_scratch + ray * s;
        if (dist_on || weights_out) {
            const float *dv = dirs + ray * d_stride;
            float nn = dv[0] * dv[0]; nn = nn + dv[1] * dv[1]; nn = nn + dv[2] * dv[2];
            nrm = sqrtf(nn);
            // walk 1 (forward order): exclusive prefix of log(clamp_min(1 - alpha, 1e-10)) rounded to fp32 like torch::cumsum's output; the weights; the totals of w and w m
            double carry = 0.0;
            for (int base = 0; base < s; base += 64) {
                const int j = base + lane;
                const bool live = j < s;
                float lg = 0.0f, alpha = 0.0f, mj = 0.0f;
                if (live) {
                    const float zj = zr[j], zn = (j + 1 < s) ? zr[j + 1] : zj;
                    float dist = (j + 1 < s) ? (zn - zj) : 1e10f;
                    dist = dist * nrm;
                    float sr = raw[(ray * s + j) * c + 3];
                    if (noise) sr = sr + noise[ray * s + j] * noise_std;
                    const float sig = sr > 0.0f ? sr : 0.0f;
                    alpha = -nrf_expf(-sig * dist) + 1.0f;
                    const float om = 1.0f - alpha;
                    lg = nrf_logf(om > 1e-10f ? om : 1e-10f);
                    if (dist_on) mj = 0.5f * ((zj - z0) / span + (zn - z0) / span);          // (the last sample: zn = zj, m = t_{s-1})
                }
                const double incl = wave_incl_scan((double)lg, lane);
                const float excl = (float)(carry + (incl - (double)lg));
                carry += __shfl(incl, 63);
                if (live) {
                    lt[j] = excl;
                    const float w = alpha * nrf_expf(excl);
                    if (weights_out) weights_out[ray * s + j] = w;
                    w_tot += (double)w; m_tot += (double)w * (double)mj;
                }
            }
            w_tot = wave_sum(w_tot); m_tot = wave_sum(m_tot);
            wave_sync();                                              // the wave reads its own lt row back below
        }
        if (dist_on || sparse_on) {
            // walk 2 (reverse order): sums over LATER samples = later blocks' totals + (this block's total - its inclusive prefix)
            double w_suf = 0.0, m_suf = 0.0, gl_suf = 0.0;
            const int nblk = (s + 63) / 64;
            for (int blk = nblk - 1; blk >= 0; blk--) {
                const int j = blk * 64 + lane;
                const bool live = j < s;
                float sraw = 0.0f, sp = 0.0f, dist = 0.0f, x = 0.0f, alpha = 0.0f, trans = 0.0f, w = 0.0f, mj = 0.0f, dl = 0.0f, cl = 0.0f;
                if (live) {
                    sraw = raw[(ray * s + j) * c + 3];
                    sp = sraw > 0.0f ? sraw : 0.0f;
                    if (dist_on) {
                        const float zj = zr[j], zn = (j + 1 < s) ? zr[j + 1] : zj;
                        dist = (j + 1 < s) ? (zn - zj) : 1e10f;
                        dist = dist * nrm;
                        if (noise) sraw = sraw + noise[ray * s + j] * noise_std;
                        const float sig = sraw > 0.0f ? sraw : 0.0f;
                        x = -sig * dist;
                        alpha = -nrf_expf(x) + 1.0f;
                        const float l = lt[j];
                        trans = nrf_expf(l);
                        cl = fminf(fmaxf(l, -100.0f), 5.0f);
                        w = alpha * trans;
                        const float tj = (zj - z0) / span, tn = (zn - z0) / span;
                        mj = 0.5f * (tj + tn);
                        dl = tn - tj;
                    }
                }
                float g_sigma = 0.0f;
                if (dist_on) {
                    const double wd = (double)w, wm = (double)w * (double)mj;
                    const double w_incl = wave_incl_scan(wd, lane), m_incl = wave_incl_scan(wm, lane);
                    const double w_blk = __shfl(w_incl, 63), m_blk = __shfl(m_incl, 63);
                    const double w_after = w_suf + (w_blk - w_incl), m_after = m_suf + (m_blk - m_incl);
                    w_suf += w_blk; m_suf += m_blk;
                    const double w_before = w_tot - wd - w_after, m_before = m_tot - wm - m_after;
                    const double after = m_after - (double)mj * w_after;          // sum over j > i of w_j (m_j - m_i)
                    const double before = (double)mj * w_before - m_before;       // sum over j < i of w_j (m_i - m_j)
                    const double self = wd * (double)dl;
                    l_dist += wd * (2.0 * after + self * (1.0 / 3.0));
                    const float gw = live ? k_dist * (float)(2.0 * (before + after) + self * (2.0 / 3.0)) : 0.0f;
                    // k_raw2outputs_bwd's chain from g_w
                    const float gL = gw * alpha * nrf_expf(cl);                   // g_T * dT/dL with TruncExp's clamped derivative
                    const double g_incl = wave_incl_scan((double)gL, lane);
                    const double g_blk = __shfl(g_incl, 63);
                    const double later = gl_suf + (g_blk - g_incl);
                    gl_suf += g_blk;
                    float g_alpha = gw * trans;
                    const float om = 1.0f - alpha;
                    if (om >= 1e-10f) g_alpha -= (float)later / om;
                    const float cx = fminf(fmaxf(x, -100.0f), 5.0f);
                    const float g_x = -g_alpha * nrf_expf(cx);
                    g_sigma = (sraw > 0.0f) ? -g_x * dist : 0.0f;
                }
                if (sparse_on && live) {
                    const float q = 1.0f + 2.0f * (sp * sp);
                    l_sparse += (double)nrf_logf(q);
                    g_sigma = g_sigma + k_sparse * (4.0f * sp / q);
                }
                if (live) {
                    float *g = g_raw + (ray * s + j) * c + 3;
                    *g = *g + g_sigma;
                }
            }
        }
    }
    double sums[2] = {l_dist, l_sparse};
    ordered_block_sum<64 * RR_RAYS, 2>(sums, s_sum);
    if (threadIdx.x < 2) partials[(int64_t)blockIdx.x * 2 + threadIdx.x] = threadIdx.x == 0 ? sums[0] : sums[1];
}

inline size_t rr_row_bytes(int64_t n, int s) { return align_up((size_t)n * (size_t)s * sizeof(float), 8); }

}  // namespace

}  // namespace nrf

using namespace nrf;

extern "C" {

size_t nrf_ray_regularizers_workspace_bytes(int64_t n, int s)
{
    if (n <= 0 || s <= 0) return 0;
    return rr_row_bytes(n, s) + (size_t)ceil_div(n, RR_RAYS) * 2 * sizeof(double);
}

int nrf_ray_regularizers(const float *d_raw, const float *d_z, const float *d_dirs, int d_stride, int64_t n, int s, int c, const float *d_noise, float noise_std,
                         float distortion_weight, float sparsity_weight, float *d_g_raw, float *d_losses, float *d_weights_out, void *d_workspace, size_t workspace_bytes,
                         void *stream)
{
    NRF_CHECK_ARG(d_raw && d_z && d_dirs && d_g_raw && d_losses && n >= 0 && s >= 1 && d_stride >= 3, "nrf_ray_regularizers: bad argument");
    if (c != 4 && c != 7) { set_error("nrf_ray_regularizers: raw rows of %d columns (4, or 7 with the predicted-normals head)", c); return NRF_ERR_UNSUPPORTED; }
    NRF_CHECK_ARG(std::isfinite(distortion_weight) && distortion_weight >= 0.0f && std::isfinite(sparsity_weight) && sparsity_weight >= 0.0f,
                  "nrf_ray_regularizers: the weights must be finite and >= 0");
    NRF_CHECK_ARG(n < ((int64_t)1 << 31), "nrf_ray_regularizers: batch too large");          // (four rays per block: the grid stays below 2^31 blocks)
    hipStream_t st = as_stream(stream);
    if (n == 0 || (distortion_weight == 0.0f && sparsity_weight == 0.0f)) {          // nothing to add: no kernel runs, d_g_raw (and d_weights_out) stay as they are
        NRF_HIP(hipMemsetAsync(d_losses, 0, 2 * sizeof(float), st));
        return NRF_OK;
    }
    const size_t need = nrf_ray_regularizers_workspace_bytes(n, s);
    if (!d_workspace || workspace_bytes < need) {
        set_error("nrf_ray_regularizers: workspace %zu < %zu bytes", workspace_bytes, need);
        return NRF_ERR_WORKSPACE;
    }
    NRF_CHECK_ARG((reinterpret_cast<uintptr_t>(d_workspace) & 7) == 0, "nrf_ray_regularizers: the workspace must be 8-byte aligned");
    float *lt = static_cast<float *>(d_workspace);
    double *partials = reinterpret_cast<double *>(static_cast<char *>(d_workspace) + rr_row_bytes(n, s));
    const int64_t blocks = ceil_div(n, RR_RAYS);
    const float k_dist = (float)((double)distortion_weight / (double)n), k_sparse = (float)((double)sparsity_weight / (double)n);
    const int terms = (distortion_weight != 0.0f ? 1 : 0) | (sparsity_weight != 0.0f ? 2 : 0);
    hipLaunchKernelGGL(k_ray_reg, dim3((unsigned)blocks), dim3(64 * RR_RAYS), 0, st, n, s, c, d_raw, d_z, d_dirs, d_stride, d_noise, noise_std, k_dist, k_sparse, terms, d_g_raw,
                       d_weights_out, lt, partials);
    NRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_finish_loss_pair<RR_FIN>, dim3(1), dim3(RR_FIN), 0, st, blocks, (const double *)partials, (double)n, (double)n, d_losses);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

}  // extern "C"
