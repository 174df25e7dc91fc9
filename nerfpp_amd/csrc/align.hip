// align.hip -- registering one surface onto another: the pose (nrf_align_state_init), moving points through it (nrf_align_apply), the normal-equation sums of an
// ICP iteration over given pairs (nrf_align_sums) and the small solve that updates the pose on the device (nrf_align_solve).  The reference has none of it; the
// contract is stated in include/nerfpp_hip.h ("Registration") and restated in numpy by tests/align_ref.py, which the GPU tests compare with bit for bit.
//
// Pose.  Eight doubles: a unit quaternion (w, x, y, z), a scale s, a translation t; x -> s R x + t.  quat_rot is the one place R is formed.
// Sums.  k_align_sums<MODE>: ALIGN_TILE pairs per block, lane t takes t, t + 256, ... in ascending order into one fp64 accumulator per column; reduce.h's ordered
//   block sum, one row of NV partials per block.  No atomics on a sum; the drop counters are integers.  The pairs come from nrf_closest_on_mesh (or a gather after
//   nrf_nearest_points) as they are: the query is NOT fused in, because its far-list fallback finishes queries in an order the scheduling decides.
// Solve.  k_align_solve: one workgroup; reduce.h's finish pass per column, then thread 0 alone: Horn's closed form through a cyclic Jacobi iteration of the 4x4
//   matrix (point mode) or a Cholesky factorisation of the 6x6 / 7x7 normal equations (plane mode), in fp64 with + - * / sqrt only, the update composed into the
//   state and one row of the history.  Nothing returns to the host: a whole ICP run is a chain of launches on one stream.
// Every loop is bounded by a count; no kernel waits on another workgroup.
#include "reduce.h"
#include "scan.h"
#include "workspace.h"
#include "face_grid.h"

#include <climits>
#include <cmath>

namespace nrf {

namespace {

constexpr int ALIGN_BLOCK = 256;
constexpr int ALIGN_TILE = NRF_ALIGN_TILE;          // pairs per block of k_align_sums
constexpr int NV_POINT = NRF_ALIGN_POINT_COLUMNS, NV_PLANE = NRF_ALIGN_PLANE_COLUMNS;
constexpr int JACOBI_SWEEPS = NRF_ALIGN_JACOBI_SWEEPS;

struct Pose {
    double v[8];
};

struct AlignWs {
    double *partials;          // [blocks][NV]
};

inline int align_nv(int mode) { return mode == NRF_ALIGN_POINT ? NV_POINT : NV_PLANE; }
inline int64_t align_blocks(int64_t n) { return n > 0 ? ceil_div(n, ALIGN_TILE) : 1; }
inline bool align_shape_ok(int64_t n, int mode) { return n >= 0 && n <= INT32_MAX && (mode == NRF_ALIGN_POINT || mode == NRF_ALIGN_PLANE); }

AlignWs align_layout(Bump &b, int64_t n, int mode)
{
    AlignWs s;
    s.partials = b.take<double>((size_t)align_blocks(n) * align_nv(mode));
    return s;
}

// R of a unit quaternion (w, x, y, z), row-major, in the header's order
__device__ __forceinline__ void quat_rot(double w, double x, double y, double z, double R[9])
{
    R[0] = 1.0 - 2.0 * (y * y + z * z);
    R[1] = 2.0 * (x * y - w * z);
    R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);
    R[4] = 1.0 - 2.0 * (x * x + z * z);
    R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);
    R[7] = 2.0 * (y * z + w * x);
    R[8] = 1.0 - 2.0 * (x * x + y * y);
}

__device__ __forceinline__ double dot3(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__global__ void k_align_state_set(Pose p, double *__restrict__ state)
{
    if (threadIdx.x < 8) state[threadIdx.x] = p.v[threadIdx.x];
}

__global__ void __launch_bounds__(ALIGN_BLOCK) k_align_apply(const float *points, int64_t n, const double *__restrict__ state, int rotate_only, float *out)
{
    const int64_t i = (int64_t)blockIdx.x * ALIGN_BLOCK + threadIdx.x;
    if (i >= n) return;
    double M[9];
    quat_rot(state[0], state[1], state[2], state[3], M);
    double t[3] = {0.0, 0.0, 0.0};
    if (!rotate_only) {
        const double s = state[4];
#pragma unroll
        for (int k = 0; k < 9; k++) M[k] = s * M[k];
        t[0] = state[5]; t[1] = state[6]; t[2] = state[7];
    }
    const double x0 = (double)points[i * 3 + 0], x1 = (double)points[i * 3 + 1], x2 = (double)points[i * 3 + 2];          // all three read before the first write: in place
    float y[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double r = (M[a * 3 + 0] * x0 + M[a * 3 + 1] * x1) + M[a * 3 + 2] * x2;
        y[a] = rotate_only ? (float)r : (float)(r + t[a]);
    }
    out[i * 3 + 0] = y[0];
    out[i * 3 + 1] = y[1];
    out[i * 3 + 2] = y[2];
}

// GIVEN (plane mode only): the normal of pair i is verts[i] -- the caller's d_n, one per pair -- not the cross product of face[i]'s corners; face is any index whose
// sign says whether there is a pair (nrf_align_sums_normals)
template <int MODE, bool GIVEN = false>
__global__ void __launch_bounds__(ALIGN_BLOCK) k_align_sums(const float *__restrict__ ym, const float *__restrict__ pm, const int32_t *__restrict__ face, int64_t n,
                                                            const float *__restrict__ verts, int32_t n_verts, const int32_t *__restrict__ faces, int64_t n_faces,
                                                            double *__restrict__ partials, uint32_t *__restrict__ stats)
{
    constexpr int NV = MODE == NRF_ALIGN_POINT ? NV_POINT : NV_PLANE;
    __shared__ double s_wave[NV * (ALIGN_BLOCK / 64)];
    __shared__ int sh[ALIGN_BLOCK / 64];
    const int t = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * ALIGN_TILE;
    const int64_t left = n - first;
    const int cnt = left < ALIGN_TILE ? (int)(left > 0 ? left : 0) : ALIGN_TILE;
    double acc[NV];
#pragma unroll
    for (int c = 0; c < NV; c++) acc[c] = 0.0;
    int drop[4] = {0, 0, 0, 0};          // no pair, a non-finite coordinate, a bad or non-finite face, a face without a normal
    for (int e = t; e < cnt; e += ALIGN_BLOCK) {
        const int64_t i = first + e;
        const int32_t f = face[i];
        if (f < 0) { drop[0]++; continue; }
        const float yf[3] = {ym[i * 3 + 0], ym[i * 3 + 1], ym[i * 3 + 2]}, pf[3] = {pm[i * 3 + 0], pm[i * 3 + 1], pm[i * 3 + 2]};
        if (!finite3(yf) || !finite3(pf)) { drop[1]++; continue; }
        const double y[3] = {(double)yf[0], (double)yf[1], (double)yf[2]}, p[3] = {(double)pf[0], (double)pf[1], (double)pf[2]};
        const double d[3] = {p[0] - y[0], p[1] - y[1], p[2] - y[2]};
        if (MODE == NRF_ALIGN_POINT) {
            acc[0] += 1.0;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                acc[1 + a] += y[a];
                acc[4 + a] += p[a];
#pragma unroll
                for (int b = 0; b < 3; b++) acc[7 + a * 3 + b] += y[a] * p[b];
            }
            acc[16] += dot3(y, y);
            acc[17] += dot3(p, p);
            acc[18] += dot3(d, d);
        } else {
            double cx, cy, cz;
            if (GIVEN) {
                cx = (double)verts[i * 3 + 0]; cy = (double)verts[i * 3 + 1]; cz = (double)verts[i * 3 + 2];
            } else {
                float fa[3], fb[3], fc[3];
                if (cm_face(verts, n_verts, faces, n_faces, f, fa, fb, fc) != 0) { drop[2]++; continue; }
                const double e1[3] = {(double)fb[0] - (double)fa[0], (double)fb[1] - (double)fa[1], (double)fb[2] - (double)fa[2]};
                const double e2[3] = {(double)fc[0] - (double)fa[0], (double)fc[1] - (double)fa[1], (double)fc[2] - (double)fa[2]};
                cx = e1[1] * e2[2] - e1[2] * e2[1]; cy = e1[2] * e2[0] - e1[0] * e2[2]; cz = e1[0] * e2[1] - e1[1] * e2[0];
            }
            const double len2 = (cx * cx + cy * cy) + cz * cz;
            if (!(len2 > 0.0) || (GIVEN && !isfinite(len2))) { drop[3]++; continue; }
            const double len = sqrt(len2);
            const double nn[3] = {cx / len, cy / len, cz / len};
            const double r = dot3(nn, d);
            const double row[7] = {y[1] * nn[2] - y[2] * nn[1], y[2] * nn[0] - y[0] * nn[2], y[0] * nn[1] - y[1] * nn[0], nn[0], nn[1], nn[2], dot3(nn, y)};
            int c = 0;
#pragma unroll
            for (int a = 0; a < 7; a++) {
#pragma unroll
                for (int b = a; b < 7; b++) acc[c++] += row[a] * row[b];
            }
#pragma unroll
            for (int a = 0; a < 7; a++) acc[28 + a] += row[a] * r;
            acc[35] += 1.0;
            acc[36] += r * r;
        }
    }
    ordered_block_sum<ALIGN_BLOCK, NV>(acc, s_wave);
    if (t == 0) {
#pragma unroll
        for (int c = 0; c < NV; c++) partials[(int64_t)blockIdx.x * NV + c] = acc[c];
    }
    if (!stats) return;          // uniform
#pragma unroll
    for (int k = 0; k < 4; k++) {          // counts: their values do not depend on the order of the additions
        const int total = block_sum<int, ALIGN_BLOCK>(drop[k], sh);
        if (t == 0 && total) atomicAdd(stats + k, (uint32_t)total);
    }
}

// the update (dq, ds, dt) of point mode from the totals T[NV_POINT]; returns the flag
__device__ int solve_point(const double *T, bool scale, double dq[4], double &ds, double dt[3])
{
    const double cnt = T[0];
    if (!(cnt >= 3.0)) return NRF_ALIGN_FLAG_FEW_PAIRS;
    const double sy[3] = {T[1], T[2], T[3]}, sp[3] = {T[4], T[5], T[6]};
    double yb[3], pb[3], S[9];
    for (int a = 0; a < 3; a++) { yb[a] = sy[a] / cnt; pb[a] = sp[a] / cnt; }
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) S[a * 3 + b] = T[7 + a * 3 + b] - (sy[a] * sp[b]) / cnt;
    const double vy = T[16] - dot3(sy, sy) / cnt;
    if (!(vy > 0.0)) return NRF_ALIGN_FLAG_NO_SPREAD;
    const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
    double A[4][4], V[4][4];
    A[0][0] = (Sxx + Syy) + Szz;
    A[1][1] = (Sxx - Syy) - Szz;
    A[2][2] = (Syy - Sxx) - Szz;
    A[3][3] = (Szz - Sxx) - Syy;
    A[0][1] = A[1][0] = Syz - Szy;
    A[0][2] = A[2][0] = Szx - Sxz;
    A[0][3] = A[3][0] = Sxy - Syx;
    A[1][2] = A[2][1] = Sxy + Syx;
    A[1][3] = A[3][1] = Szx + Sxz;
    A[2][3] = A[3][2] = Syz + Szy;
    for (int a = 0; a < 4; a++)
        for (int b = 0; b < 4; b++) V[a][b] = a == b ? 1.0 : 0.0;
    for (int sweep = 0; sweep < JACOBI_SWEEPS; sweep++) {
        for (int p = 0; p < 3; p++) {
            for (int q = p + 1; q < 4; q++) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double th = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double ath = fabs(th);
                double tt;
                if (ath > NRF_ALIGN_JACOBI_BIG_THETA) tt = 0.5 / th;          // th * th would overflow
                else tt = (th >= 0.0 ? 1.0 : -1.0) / (ath + sqrt(th * th + 1.0));
                const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
                for (int k = 0; k < 4; k++) {          // A <- A J
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 4; k++) {          // A <- J^T A
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 4; k++) {          // V <- V J
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
        }
    }
    int best = 0;
    for (int k = 1; k < 4; k++)
        if (A[k][k] > A[best][best]) best = k;
    double q[4] = {V[0][best], V[1][best], V[2][best], V[3][best]};
    if (q[0] < 0.0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
    const double nrm = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    if (!(nrm > 0.0) || !isfinite(nrm)) return NRF_ALIGN_FLAG_BAD_ROTATION;
    for (int k = 0; k < 4; k++) dq[k] = q[k] / nrm;
    double R[9];
    quat_rot(dq[0], dq[1], dq[2], dq[3], R);
    ds = 1.0;
    if (scale) {
        double num = 0.0;
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) {
                const double term = R[a * 3 + b] * S[b * 3 + a];
                num = (a == 0 && b == 0) ? term : num + term;
            }
        ds = num / vy;
        if (!(ds > 0.0) || !isfinite(ds)) return NRF_ALIGN_FLAG_BAD_SCALE;
    }
    for (int a = 0; a < 3; a++) dt[a] = pb[a] - ds * ((R[a * 3 + 0] * yb[0] + R[a * 3 + 1] * yb[1]) + R[a * 3 + 2] * yb[2]);
    return NRF_ALIGN_FLAG_OK;
}

// the update of plane mode from the totals T[NV_PLANE]
__device__ int solve_plane(const double *T, bool scale, double dq[4], double &ds, double dt[3])
{
    const int m = scale ? 7 : 6;
    if (!(T[35] >= (double)m)) return NRF_ALIGN_FLAG_FEW_PAIRS;
    double H[7][7], Lc[7][7], g[7], z[7], x[7];
    int c = 0;
    for (int a = 0; a < 7; a++)
        for (int b = a; b < 7; b++) { H[a][b] = T[c]; H[b][a] = T[c]; c++; }
    for (int a = 0; a < 7; a++) g[a] = T[28 + a];
    for (int j = 0; j < m; j++) {
        double d = H[j][j];
        for (int k = 0; k < j; k++) d = d - Lc[j][k] * Lc[j][k];
        if (!(d > 0.0) || !isfinite(d)) return NRF_ALIGN_FLAG_BAD_PIVOT;
        const double l = sqrt(d);
        Lc[j][j] = l;
        for (int i = j + 1; i < m; i++) {
            double v = H[i][j];
            for (int k = 0; k < j; k++) v = v - Lc[i][k] * Lc[j][k];
            Lc[i][j] = v / l;
        }
    }
    for (int i = 0; i < m; i++) {
        double v = g[i];
        for (int k = 0; k < i; k++) v = v - Lc[i][k] * z[k];
        z[i] = v / Lc[i][i];
    }
    for (int i = m - 1; i >= 0; i--) {
        double v = z[i];
        for (int k = i + 1; k < m; k++) v = v - Lc[k][i] * x[k];
        x[i] = v / Lc[i][i];
    }
    for (int i = 0; i < m; i++)
        if (!isfinite(x[i])) return NRF_ALIGN_FLAG_BAD_PIVOT;
    const double qa = x[0] / 2.0, qb = x[1] / 2.0, qc = x[2] / 2.0;
    const double nrm = sqrt(((1.0 + qa * qa) + qb * qb) + qc * qc);
    if (!isfinite(nrm)) return NRF_ALIGN_FLAG_BAD_ROTATION;
    dq[0] = 1.0 / nrm; dq[1] = qa / nrm; dq[2] = qb / nrm; dq[3] = qc / nrm;
    ds = scale ? 1.0 + x[6] : 1.0;
    if (!(ds > 0.0) || !isfinite(ds)) return NRF_ALIGN_FLAG_BAD_SCALE;
    dt[0] = x[3]; dt[1] = x[4]; dt[2] = x[5];
    return NRF_ALIGN_FLAG_OK;
}

__global__ void __launch_bounds__(ALIGN_BLOCK) k_align_solve(int64_t blocks, int mode, int scale, const double *__restrict__ partials, double *__restrict__ state,
                                                             double *__restrict__ history_row)
{
    __shared__ double s_a[ALIGN_BLOCK];
    __shared__ double s_tot[NV_PLANE];
    const int nv = mode == NRF_ALIGN_POINT ? NV_POINT : NV_PLANE;
    for (int v = 0; v < nv; v++) {          // one column at a time, as k_geo_finish: 37 columns at once would not fit the LDS
        const double a = ordered_finish<ALIGN_BLOCK>(partials, blocks, nv, v, s_a);
        if (threadIdx.x == 0) s_tot[v] = a;
    }
    if (threadIdx.x != 0) return;
    double dq[4] = {1.0, 0.0, 0.0, 0.0}, ds = 1.0, dt[3] = {0.0, 0.0, 0.0};
    const int flag = mode == NRF_ALIGN_POINT ? solve_point(s_tot, scale != 0, dq, ds, dt) : solve_plane(s_tot, scale != 0, dq, ds, dt);
    double s_new = state[4];
    if (flag == NRF_ALIGN_FLAG_OK) {
        const double w = state[0], x = state[1], y = state[2], z = state[3];
        const double t[3] = {state[5], state[6], state[7]};
        double q[4];
        q[0] = ((dq[0] * w - dq[1] * x) - dq[2] * y) - dq[3] * z;
        q[1] = ((dq[0] * x + dq[1] * w) + dq[2] * z) - dq[3] * y;
        q[2] = ((dq[0] * y - dq[1] * z) + dq[2] * w) + dq[3] * x;
        q[3] = ((dq[0] * z + dq[1] * y) - dq[2] * x) + dq[3] * w;
        const double nrm = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
        double R[9];
        quat_rot(dq[0], dq[1], dq[2], dq[3], R);
        for (int k = 0; k < 4; k++) state[k] = q[k] / nrm;
        s_new = ds * s_new;
        state[4] = s_new;
        for (int a = 0; a < 3; a++) state[5 + a] = ds * ((R[a * 3 + 0] * t[0] + R[a * 3 + 1] * t[1]) + R[a * 3 + 2] * t[2]) + dt[a];
    } else {          // the identity update: the state keeps its bits
        dq[0] = 1.0; dq[1] = dq[2] = dq[3] = 0.0;
        ds = 1.0;
        dt[0] = dt[1] = dt[2] = 0.0;
    }
    if (!history_row) return;
    history_row[0] = mode == NRF_ALIGN_POINT ? s_tot[0] : s_tot[35];
    history_row[1] = mode == NRF_ALIGN_POINT ? s_tot[18] : s_tot[36];
    history_row[2] = (double)flag;
    history_row[3] = 2.0 * sqrt((dq[1] * dq[1] + dq[2] * dq[2]) + dq[3] * dq[3]);
    history_row[4] = sqrt((dt[0] * dt[0] + dt[1] * dt[1]) + dt[2] * dt[2]);
    history_row[5] = ds;
    history_row[6] = s_new;
    history_row[7] = 0.0;
}

inline bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

}  // namespace nrf

using namespace nrf;

extern "C" {

int nrf_align_state_init(const double *pose, double *d_state, void *stream)
{
    NRF_CHECK_ARG(d_state && aligned_to(d_state, 8), "nrf_align_state_init: d_state must be non-null and 8-byte aligned");
    Pose p{{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0}};
    if (pose) {
        for (int k = 0; k < 8; k++) NRF_CHECK_ARG(std::isfinite(pose[k]), "nrf_align_state_init: pose[%d] is not finite", k);
        const double nrm = std::sqrt(((pose[0] * pose[0] + pose[1] * pose[1]) + pose[2] * pose[2]) + pose[3] * pose[3]);
        NRF_CHECK_ARG(nrm > 0.0 && std::isfinite(nrm), "nrf_align_state_init: the quaternion has no direction (norm %g)", nrm);
        NRF_CHECK_ARG(pose[4] > 0.0, "nrf_align_state_init: the scale must be > 0 (got %g)", pose[4]);
        for (int k = 0; k < 4; k++) p.v[k] = pose[k] / nrm;
        for (int k = 4; k < 8; k++) p.v[k] = pose[k];
    }
    hipLaunchKernelGGL(k_align_state_set, dim3(1), dim3(64), 0, as_stream(stream), p, d_state);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

int nrf_align_apply(const float *d_points, int64_t n, const double *d_state, int rotate_only, float *d_out, void *stream)
{
    NRF_CHECK_ARG(n >= 0 && n <= INT32_MAX, "nrf_align_apply: %lld points (0 .. 2^31 - 1)", (long long)n);
    NRF_CHECK_ARG(rotate_only == 0 || rotate_only == 1, "nrf_align_apply: rotate_only must be 0 or 1 (got %d)", rotate_only);
    NRF_CHECK_ARG(d_state && aligned_to(d_state, 8), "nrf_align_apply: d_state must be non-null and 8-byte aligned");
    NRF_CHECK_ARG(n == 0 || (d_points && d_out), "nrf_align_apply: null d_points or d_out");
    NRF_CHECK_ARG(aligned_to(d_points, 4) && aligned_to(d_out, 4), "nrf_align_apply: d_points and d_out must be 4-byte aligned");
    if (n == 0) return NRF_OK;
    hipLaunchKernelGGL(k_align_apply, dim3((unsigned)ceil_div(n, ALIGN_BLOCK)), dim3(ALIGN_BLOCK), 0, as_stream(stream), d_points, n, d_state, rotate_only, d_out);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

size_t nrf_align_workspace_bytes(int64_t n, int mode)
{
    if (!align_shape_ok(n, mode)) return 0;
    return measure([&](Bump &b) { align_layout(b, n, mode); });
}

int nrf_align_sums(const float *d_y, const float *d_p, const int32_t *d_face, int64_t n, int mode, const float *d_verts, int64_t n_verts, const int32_t *d_faces,
                   int64_t n_faces, uint32_t *d_stats, void *d_workspace, size_t workspace_bytes, void *stream)
{
    NRF_CHECK_ARG(mode == NRF_ALIGN_POINT || mode == NRF_ALIGN_PLANE, "nrf_align_sums: mode %d is neither NRF_ALIGN_POINT nor NRF_ALIGN_PLANE", mode);
    NRF_CHECK_ARG(n >= 0 && n <= INT32_MAX, "nrf_align_sums: %lld pairs (0 .. 2^31 - 1)", (long long)n);
    NRF_CHECK_ARG(n == 0 || (d_y && d_p && d_face), "nrf_align_sums: null d_y, d_p or d_face");
    NRF_CHECK_ARG(aligned_to(d_y, 4) && aligned_to(d_p, 4) && aligned_to(d_face, 4) && aligned_to(d_stats, 4), "nrf_align_sums: d_y, d_p, d_face and d_stats must be 4-byte aligned");
    if (mode == NRF_ALIGN_PLANE) {
        NRF_CHECK_ARG(sample_shape_ok(n_verts, n_faces), "nrf_align_sums: %lld vertices, %lld faces (both 0 .. 2^31 - 1)", (long long)n_verts, (long long)n_faces);
        NRF_CHECK_ARG(d_faces && d_verts, "nrf_align_sums: NRF_ALIGN_PLANE needs the target mesh (null d_verts or d_faces)");
        NRF_CHECK_ARG(aligned_to(d_verts, 4) && aligned_to(d_faces, 4), "nrf_align_sums: d_verts and d_faces must be 4-byte aligned");
    }
    NRF_CHECK_ARG(d_workspace && aligned_to(d_workspace, 8), "nrf_align_sums: the workspace must be non-null and 8-byte aligned");
    Bump bump(d_workspace, workspace_bytes);
    const AlignWs ws = align_layout(bump, n, mode);
    NRF_TRY(ws_check(bump, nrf_align_workspace_bytes(n, mode), "nrf_align_sums"));
    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)align_blocks(n));          // n == 0: one block writes a row of zeros, so the solve sees no pairs
    if (mode == NRF_ALIGN_POINT)
        hipLaunchKernelGGL(k_align_sums<NRF_ALIGN_POINT>, grid, dim3(ALIGN_BLOCK), 0, st, d_y, d_p, d_face, n, (const float *)nullptr, 0, (const int32_t *)nullptr,
                           (int64_t)0, ws.partials, d_stats);
    else
        hipLaunchKernelGGL(k_align_sums<NRF_ALIGN_PLANE>, grid, dim3(ALIGN_BLOCK), 0, st, d_y, d_p, d_face, n, d_verts, (int32_t)n_verts, d_faces, n_faces, ws.partials,
                           d_stats);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

int nrf_align_sums_normals(const float *d_y, const float *d_p, const float *d_n, const int32_t *d_index, int64_t n, uint32_t *d_stats, void *d_workspace,
                           size_t workspace_bytes, void *stream)
{
    NRF_CHECK_ARG(n >= 0 && n <= INT32_MAX, "nrf_align_sums_normals: %lld pairs (0 .. 2^31 - 1)", (long long)n);
    NRF_CHECK_ARG(n == 0 || (d_y && d_p && d_n && d_index), "nrf_align_sums_normals: null d_y, d_p, d_n or d_index");
    NRF_CHECK_ARG(aligned_to(d_y, 4) && aligned_to(d_p, 4) && aligned_to(d_n, 4) && aligned_to(d_index, 4) && aligned_to(d_stats, 4),
                  "nrf_align_sums_normals: d_y, d_p, d_n, d_index and d_stats must be 4-byte aligned");
    NRF_CHECK_ARG(d_workspace && aligned_to(d_workspace, 8), "nrf_align_sums_normals: the workspace must be non-null and 8-byte aligned");
    Bump bump(d_workspace, workspace_bytes);
    const AlignWs ws = align_layout(bump, n, NRF_ALIGN_PLANE);
    NRF_TRY(ws_check(bump, nrf_align_workspace_bytes(n, NRF_ALIGN_PLANE), "nrf_align_sums_normals"));
    hipLaunchKernelGGL((k_align_sums<NRF_ALIGN_PLANE, true>), dim3((unsigned)align_blocks(n)), dim3(ALIGN_BLOCK), 0, as_stream(stream), d_y, d_p, d_index, n, d_n, 0,
                       (const int32_t *)nullptr, (int64_t)0, ws.partials, d_stats);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

int nrf_align_solve(int64_t n, int mode, int scale, int iteration, int n_history, double *d_state, double *d_history, void *d_workspace, size_t workspace_bytes,
                    void *stream)
{
    NRF_CHECK_ARG(mode == NRF_ALIGN_POINT || mode == NRF_ALIGN_PLANE, "nrf_align_solve: mode %d is neither NRF_ALIGN_POINT nor NRF_ALIGN_PLANE", mode);
    NRF_CHECK_ARG(n >= 0 && n <= INT32_MAX, "nrf_align_solve: %lld pairs (0 .. 2^31 - 1)", (long long)n);
    NRF_CHECK_ARG(scale == 0 || scale == 1, "nrf_align_solve: scale must be 0 or 1 (got %d)", scale);
    NRF_CHECK_ARG(d_state && aligned_to(d_state, 8), "nrf_align_solve: d_state must be non-null and 8-byte aligned");
    NRF_CHECK_ARG(aligned_to(d_history, 8), "nrf_align_solve: d_history must be 8-byte aligned");
    NRF_CHECK_ARG(!d_history || (n_history >= 1 && iteration >= 0 && iteration < n_history), "nrf_align_solve: iteration %d outside the history's %d rows", iteration,
                  n_history);
    NRF_CHECK_ARG(d_workspace && aligned_to(d_workspace, 8), "nrf_align_solve: the workspace must be non-null and 8-byte aligned");
    Bump bump(d_workspace, workspace_bytes);
    const AlignWs ws = align_layout(bump, n, mode);
    NRF_TRY(ws_check(bump, nrf_align_workspace_bytes(n, mode), "nrf_align_solve"));
    hipLaunchKernelGGL(k_align_solve, dim3(1), dim3(ALIGN_BLOCK), 0, as_stream(stream), align_blocks(n), mode, scale, (const double *)ws.partials, d_state,
                       d_history ? d_history + (size_t)iteration * 8 : nullptr);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

}  // extern "C"
