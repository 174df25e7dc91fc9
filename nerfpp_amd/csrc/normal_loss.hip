// normal_loss.hip -- training the predicted-normals head of NeRFSmall (use_pred_normal, NeRF.cpp:343-347, :393-407) against the density normals: the two losses the
// reference defines (NeRF.h:308-326) and whose call site it left commented out (NeRFExecutor.h:929-952), and the C entry of the 7-column network backward.
//
// k_normal_losses: one lane per sample, one launch over the n * s samples of a batch.
//   w (the render's weight) and nrm = -g / max(|g|, 1e-8) (g = nrf_density_grad at the sample; nrf_render_normals' definition, normals.hip) are constants of the
//   step; pred = raw[4:7] as the network gave it (the reference normalises nowhere in the loss).
//     PredNormalLoss  = mean over n * s * 3 of (w pred - w nrm)^2                                  (torch::mse_loss, NeRF.h:324)
//     OrientationLoss = mean over rays of sum_i w_i min(0, pred_i . (-rays_d))^2                   (NeRF.h:309-316, torch::mean NeRFExecutor.h:938)
//   Written: d (pn_weight L_pn + or_weight L_or) / d pred into columns 4:7 of the raw gradient (columns 0:4 belong to nrf_raw2outputs_backward and are not touched).
//   A sample with w == 0 contributes exactly 0 to both sums and gets a zero gradient whatever pred and g hold (0 * inf never forms).
//   Memory: a block's 256 raw rows (7 floats each) and gradient rows (3 floats) are contiguous: they are staged through LDS with 16-byte loads, a lane then reads its
//   row from LDS (row strides 7 and 3 words are odd: conflict-free).  The gradient columns are three 4-byte stores per lane into 28-byte rows.
//   Sums: per lane in fp64, reduce.h's ordered block sum -> one fp64 partial pair per block; its k_finish_loss_pair (one block) is the ordered finish pass over the
//   pairs.  No atomics: two runs give the same bits.
#include "mlp.h"
#include "reduce.h"

namespace nrf {

namespace {

constexpr int NL_THREADS = 256;
constexpr int NL_C = 7;            // columns of a raw row with the head: rgb, sigma, normal xyz

// rows [base, base + cnt) of a row-major [total][W] fp32 array into LDS; `vec`: the array starts 16-byte aligned (a block's first row then does too: 256 W words)
template <int W>
__device__ __forceinline__ void stage_rows(const float *__restrict__ src, int64_t base, int cnt, bool vec, float *dst)
{
    const float *p = src + base * W;
    if (vec && cnt == NL_THREADS) {
        const float4 *p4 = reinterpret_cast<const float4 *>(p);
        float4 *d4 = reinterpret_cast<float4 *>(dst);
        for (int e = threadIdx.x; e < NL_THREADS * W / 4; e += NL_THREADS) d4[e] = p4[e];
    } else {
        for (int e = threadIdx.x; e < cnt * W; e += NL_THREADS) dst[e] = p[e];
    }
}

__global__ void __launch_bounds__(NL_THREADS)
k_normal_losses(int64_t total, int s, const float *__restrict__ w, const float *__restrict__ grad, const float *__restrict__ raw, const float *__restrict__ dirs, int d_stride,
                float k_pn /* pn_weight * 2 / (n s 3) */, float k_or /* or_weight * 2 / n */, int vec, float *__restrict__ g_raw, double *__restrict__ partials)
{
    __shared__ __attribute__((aligned(16))) float s_raw[NL_THREADS * NL_C];
    __shared__ __attribute__((aligned(16))) float s_g[NL_THREADS * 3];
    __shared__ double s_sum[2 * (NL_THREADS / 64)];
    const int t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * NL_THREADS;
    const int64_t left = total - base;
    const int cnt = left < NL_THREADS ? (int)left : NL_THREADS;          // (the grid covers `total`: cnt >= 1)
    stage_rows<NL_C>(raw, base, cnt, vec != 0, s_raw);
    stage_rows<3>(grad, base, cnt, vec != 0, s_g);
    __syncthreads();
    double l_pn = 0.0, l_or = 0.0;
    if (t < cnt) {
        const int64_t i = base + t;
        const float wi = w[i];
        float gx = 0.0f, gy = 0.0f, gz = 0.0f;
        if (wi != 0.0f) {
            const float px = s_raw[t * NL_C + 4], py = s_raw[t * NL_C + 5], pz = s_raw[t * NL_C + 6];
            const float dx = s_g[t * 3], dy = s_g[t * 3 + 1], dz = s_g[t * 3 + 2];
            const float len = fmaxf(sqrtf(dx * dx + dy * dy + dz * dz), 1e-8f);          // k_normals_composite's safe_normalize
            const float nx = -dx / len, ny = -dy / len, nz = -dz / len;
            // PredNormalLoss: the two products are formed apart, as the reference writes them (w * pred, w * nrm)
            const float ex = wi * px - wi * nx, ey = wi * py - wi * ny, ez = wi * pz - wi * nz;
            l_pn = (double)ex * (double)ex + (double)ey * (double)ey + (double)ez * (double)ez;
            const float cw = k_pn * wi;
            gx = cw * ex; gy = cw * ey; gz = cw * ez;
            // OrientationLoss: v = -rays_d as the batch holds it
            const int64_t ray = (i >> 31) == 0 ? (int64_t)((uint32_t)i / (uint32_t)s) : i / s;
            const float *dv = dirs + ray * d_stride;
            const float vx = -dv[0], vy = -dv[1], vz = -dv[2];
            float dot = px * vx; dot = dot + py * vy; dot = dot + pz * vz;
            if (dot < 0.0f) {
                l_or = (double)wi * ((double)dot * (double)dot);
                const float co = k_or * wi * dot;
                gx = gx + co * vx; gy = gy + co * vy; gz = gz + co * vz;
            }
        }
        float *o = g_raw + i * NL_C + 4;
        o[0] = gx; o[1] = gy; o[2] = gz;
    }
    double sums[2] = {l_pn, l_or};
    ordered_block_sum<NL_THREADS, 2>(sums, s_sum);
    if (t < 2) partials[(int64_t)blockIdx.x * 2 + t] = t == 0 ? sums[0] : sums[1];
}

}  // namespace

}  // namespace nrf

using namespace nrf;

extern "C" {

size_t nrf_normal_losses_workspace_bytes(int64_t n, int s)
{
    if (n <= 0 || s <= 0) return 0;
    return (size_t)ceil_div(n * s, NL_THREADS) * 2 * sizeof(double);
}

int nrf_normal_losses(const float *d_weights, const float *d_density_grad, const float *d_raw, int c, const float *d_dirs, int d_stride, int64_t n, int s,
                      float pred_normal_weight, float orientation_weight, float *d_g_raw, float *d_losses, void *d_workspace, size_t workspace_bytes, void *stream)
{
    NRF_CHECK_ARG(d_weights && d_density_grad && d_raw && d_dirs && d_g_raw && d_losses && n >= 0 && s >= 1 && d_stride >= 3, "nrf_normal_losses: bad argument");
    if (c != NL_C) { set_error("nrf_normal_losses: raw rows of %d columns; the predicted normals are columns 4:7 of a 7-column NeRFSmall output (use_pred_normal)", c); return NRF_ERR_UNSUPPORTED; }
    NRF_CHECK_ARG(n <= ((int64_t)1 << 38) / s, "nrf_normal_losses: batch too large");          // (2^38 samples / 256 per block: the grid stays below 2^31 blocks)
    hipStream_t st = as_stream(stream);
    const int64_t total = n * s;
    if (total == 0) { NRF_HIP(hipMemsetAsync(d_losses, 0, 2 * sizeof(float), st)); return NRF_OK; }
    const int64_t blocks = ceil_div(total, NL_THREADS);
    if (!d_workspace || workspace_bytes < nrf_normal_losses_workspace_bytes(n, s)) {
        set_error("nrf_normal_losses: workspace %zu < %zu bytes", workspace_bytes, nrf_normal_losses_workspace_bytes(n, s));
        return NRF_ERR_WORKSPACE;
    }
    NRF_CHECK_ARG((reinterpret_cast<uintptr_t>(d_workspace) & 7) == 0, "nrf_normal_losses: the workspace must be 8-byte aligned");
    const double cnt_pn = (double)total * 3.0, cnt_or = (double)n;
    const float k_pn = (float)((double)pred_normal_weight * 2.0 / cnt_pn), k_or = (float)((double)orientation_weight * 2.0 / cnt_or);
    const int vec = ((reinterpret_cast<uintptr_t>(d_raw) | reinterpret_cast<uintptr_t>(d_density_grad)) & 15) == 0 ? 1 : 0;
    double *partials = reinterpret_cast<double *>(d_workspace);
    hipLaunchKernelGGL(k_normal_losses, dim3((unsigned)blocks), dim3(NL_THREADS), 0, st, total, s, d_weights, d_density_grad, d_raw, d_dirs, d_stride, k_pn, k_or, vec, d_g_raw,
                       partials);
    NRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_finish_loss_pair<NL_THREADS>, dim3(1), dim3(NL_THREADS), 0, st, blocks, (const double *)partials, cnt_pn, cnt_or, d_losses);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

size_t nrf_mlp_backward_pn_workspace_bytes(const nrf_mlp *m, int64_t p)
{
    if (!m || m->family != MLP_SMALL || !m->small.use_pred_normal) return 0;
    return mlp_backward_workspace_bytes(m, p);          // one row buffer per layer + 3: the head's hidden outputs and its input gradient take the head's own layers' share
}

int nrf_mlp_backward_pn(const nrf_mlp *m, const float *d_x, const float *d_g_out, int64_t p, float *d_g_params, float *d_g_x, void *d_workspace, size_t workspace_bytes,
                        void *stream)
{
    NRF_CHECK_ARG(m && d_x && d_g_out && d_g_params && d_workspace && p >= 0, "nrf_mlp_backward_pn: bad argument");
    if (m->family != MLP_SMALL || !m->small.use_pred_normal) {
        set_error("nrf_mlp_backward_pn: needs a NeRFSmall with the predicted-normals head (use_pred_normal)");
        return NRF_ERR_UNSUPPORTED;
    }
    if (p == 0) return NRF_OK;
    return mlp_small_backward(m, d_x, m->in_dims, d_g_out, m->out_dims, p, d_g_params, d_g_x, m->small.input_ch, d_workspace, workspace_bytes, as_stream(stream), true);
}

}  // extern "C"
