// points.hip -- the point-cloud half of the geometry tools: a BVH over the points of a cloud (nrf_point_bvh_build: bvh.hip's build with the point itself as the
// leaf), the k nearest neighbours of every query through it (nrf_bvh_knn), normals and local shape from those neighbours (nrf_points_normals), outlier scores
// (nrf_knn_mean_distance) and the ordered statistics a threshold is formed from (nrf_value_stats).  The contract is stated in include/nerfpp_hip.h ("Point clouds");
// tests/points_ref.py restates every output in numpy and the GPU tests compare bit for bit.
//
// kNN.  One lane per query, k_bvh_closest's traversal (a private stack of NRF_BVH_MAX_DEPTH node indices, the nearer child first).  The list of the k best packed keys
//   lives in REGISTERS: KnnList<KL> for KL = 1, 8, 16, 32 holds KL keys in DESCENDING order, every index a compile-time constant, so the bound of the pruning test
//   -- the k-th best -- is always v[0].  Slots k .. KL - 1 start at key 0, below or equal to every candidate, and are never displaced; an accepted candidate drops
//   v[0] and is shifted into place by KL unrolled compare-and-select steps, no branch and no indexed access.  A point leaf's box is the point, so the box bound of a
//   leaf child IS its d2 (header: WHY IT IS EXACT) and no coordinate is fetched for a candidate; only the n_valid == 1 tree, which has no node, reads d_points.
// Normals.  One lane per point, everything fp64 in the header's order; the 3x3 Jacobi iteration is align.hip's rotation with every index unrolled.
// Every loop is bounded by a count or the tree's size; no kernel waits on another workgroup; no sum goes through an atomic.
#include "reduce.h"
#include "scan.h"
#include "workspace.h"
#include "face_grid.h"
#include "bvh.h"

#include <climits>
#include <cmath>

namespace nrf {

namespace {

static_assert(NRF_KNN_MAX_K == 32, "the list sizes of k_bvh_knn are written for k <= 32");
constexpr int PSTATS_TILE = 4096;          // entries per block of k_value_stats: nrf_distance_stats's
constexpr int PSTATS_VALUES = 4;           // count, sum, sum of squares, max

struct PtTree {
    const long long *head;
    const int32_t *leaf;
    const BvhNode *node;
    int64_t n;
};

// KL packed keys, descending: v[0] is the worst key held, the bound of the search
template <int KL>
struct KnnList {
    unsigned long long v[KL];

    __device__ __forceinline__ void init(int k)
    {
#pragma unroll
        for (int i = 0; i < KL; i++) v[i] = i < k ? NN_NONE : 0ull;
    }
    __device__ __forceinline__ float bound() const { return key_value(v[0]); }
    // c < v[0]: v[0] leaves, c goes in front of the first key that is not above it
    __device__ __forceinline__ void insert(unsigned long long c)
    {
        bool above = true;          // v[i] > c, as it was before this call; true for i = 0
#pragma unroll
        for (int i = 0; i < KL; i++) {
            const unsigned long long next = i + 1 < KL ? v[i + 1] : 0ull;
            const bool next_above = i + 1 < KL && next > c;
            v[i] = next_above ? next : (above ? c : v[i]);
            above = next_above;
        }
    }
    __device__ __forceinline__ void take(int64_t self, int32_t j, float d2, float md2)
    {
        if ((int64_t)j == self) return;
        const unsigned long long c = key_pack(d2, (uint32_t)j);
        if (d2 <= md2 && c < v[0]) insert(c);
    }
};

template <int KL>
__global__ void __launch_bounds__(GEO_BLOCK) k_bvh_knn(const float *__restrict__ query, int64_t nq, const int32_t *__restrict__ order, const float *__restrict__ points,
                                                       PtTree m, int k, float md2, int exclude_self, float *__restrict__ dist2, int32_t *__restrict__ index,
                                                       int32_t *__restrict__ count, uint32_t *__restrict__ stats)
{
    __shared__ int sh[GEO_BLOCK / 64];
    BvhTree t;
    if (!bvh_head_read(m.head, m.n, t, PBVH_MAGIC)) return;          // uniform: not a buffer built for these points; nothing more of it is read, nothing written
    const int64_t lane_i = (int64_t)blockIdx.x * GEO_BLOCK + threadIdx.x;
    int64_t qi = lane_i;
    if (order && lane_i < nq) qi = order[lane_i];
    const bool live = lane_i < nq && qi >= 0 && qi < nq;
    float q[3] = {0.0f, 0.0f, 0.0f};
    if (live) { q[0] = query[qi * 3 + 0]; q[1] = query[qi * 3 + 1]; q[2] = query[qi * 3 + 2]; }
    const bool finite = live && finite3(q);
    const int64_t self = exclude_self ? qi : -1;
    KnnList<KL> best;
    best.init(k);
    if (finite && t.n_valid == 1) {
        const int32_t j = m.leaf[0];
        best.take(self, j, nn_d2(q[0], q[1], q[2], make_float4(points[(int64_t)j * 3 + 0], points[(int64_t)j * 3 + 1], points[(int64_t)j * 3 + 2], 0.0f)), md2);
    }
    if (finite && t.n_valid > 1) {
        int32_t stack[NRF_BVH_MAX_DEPTH];
        int sp = 0;
        int32_t at = 0;
        for (;;) {          // every node is visited at most once: the tree's size bounds the loop
            BvhNode n;
            bvh_node_load(m.node, at, n);
            const float b0 = bvh_box_d2(q, n.lo0, n.hi0), b1 = bvh_box_d2(q, n.lo1, n.hi1);
            const bool swap = b1 < b0;          // the nearer child first
            const int32_t ca = swap ? n.child[1] : n.child[0], cb = swap ? n.child[0] : n.child[1];
            const float ba = swap ? b1 : b0, bb = swap ? b0 : b1;
            int32_t next = -1;
            // skipped iff the bound lies strictly above what can still enter the list or tie its last key
            if (!(ba > fminf(best.bound(), md2))) {
                if (ca < 0) best.take(self, m.leaf[-(ca + 1)], ba, md2);          // a leaf's bound is its d2
                else next = ca;
            }
            if (!(bb > fminf(best.bound(), md2))) {
                if (cb < 0) best.take(self, m.leaf[-(cb + 1)], bb, md2);
                else if (next < 0) next = cb;
                else if (sp < NRF_BVH_MAX_DEPTH) stack[sp++] = cb;          // always, for a tree of the build: its height is at most 62
            }
            if (next < 0) {
                if (sp == 0) break;
                next = stack[--sp];
            }
            at = next;
        }
    }
    if (live) {
        int filled = 0;
#pragma unroll
        for (int i = 0; i < KL; i++) {
            if (i < k) {          // slot k - 1 - i, ascending
                dist2[qi * k + (k - 1 - i)] = key_value(best.v[i]);
                index[qi * k + (k - 1 - i)] = key_index(best.v[i]);
                filled += best.v[i] != NN_NONE;
            }
        }
        if (count) count[qi] = filled;
    }
    if (!stats) return;          // uniform
    const int total = block_count<GEO_BLOCK>(live && !finite, sh);
    if (threadIdx.x == 0 && total) atomicAdd(stats + 0, (uint32_t)total);
}

// one Jacobi rotation of the symmetric 3x3 A on the pair (P, Q), V's columns as A's: align.hip's formula, every index a constant
template <int P, int Q>
__device__ __forceinline__ void jacobi3(double A[3][3], double V[3][3])
{
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double th = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double ath = fabs(th);
    double tt;
    if (ath > NRF_ALIGN_JACOBI_BIG_THETA) tt = 0.5 / th;          // th * th would overflow
    else tt = (th >= 0.0 ? 1.0 : -1.0) / (ath + sqrt(th * th + 1.0));
    const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
#pragma unroll
    for (int k = 0; k < 3; k++) {          // A <- A J
        const double akp = A[k][P], akq = A[k][Q];
        A[k][P] = c * akp - s * akq;
        A[k][Q] = s * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {          // A <- J^T A
        const double apk = A[P][k], aqk = A[Q][k];
        A[P][k] = c * apk - s * aqk;
        A[Q][k] = s * apk + c * aqk;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {          // V <- V J
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - s * vkq;
        V[k][Q] = s * vkp + c * vkq;
    }
}

__device__ __forceinline__ double sel3(const double v[3], int k) { return k == 0 ? v[0] : (k == 1 ? v[1] : v[2]); }

__global__ void __launch_bounds__(GEO_BLOCK) k_points_normals(const float *__restrict__ points, int64_t n, const int32_t *__restrict__ index, int k,
                                                              const float *__restrict__ toward, int toward_stride, float *__restrict__ normals, float *__restrict__ eigen,
                                                              uint32_t *__restrict__ stats)
{
    __shared__ int sh[GEO_BLOCK / 64];
    const int64_t i = (int64_t)blockIdx.x * GEO_BLOCK + threadIdx.x;
    const bool live = i < n;
    bool good = false;
    float out_n[3] = {0.0f, 0.0f, 0.0f}, out_e[3] = {0.0f, 0.0f, 0.0f};
    if (live) {
        const float pf[3] = {points[i * 3 + 0], points[i * 3 + 1], points[i * 3 + 2]};
        const double p[3] = {(double)pf[0], (double)pf[1], (double)pf[2]};
        bool fin = finite3(pf);
        int m = 1;
        double sum[3] = {p[0], p[1], p[2]};
        for (int s = 0; s < k; s++) {
            const int32_t j = index[i * k + s];
            if (j < 0 || j >= n) continue;          // an empty slot (an index outside the cloud reads nothing)
            const float xf[3] = {points[(int64_t)j * 3 + 0], points[(int64_t)j * 3 + 1], points[(int64_t)j * 3 + 2]};
            fin = fin && finite3(xf);
            sum[0] += (double)xf[0]; sum[1] += (double)xf[1]; sum[2] += (double)xf[2];
            m++;
        }
        if (fin && m >= 3) {
            const double dm = (double)m;
            const double mean[3] = {sum[0] / dm, sum[1] / dm, sum[2] / dm};
            double d[3] = {p[0] - mean[0], p[1] - mean[1], p[2] - mean[2]};
            double cxx = d[0] * d[0], cxy = d[0] * d[1], cxz = d[0] * d[2], cyy = d[1] * d[1], cyz = d[1] * d[2], czz = d[2] * d[2];
            for (int s = 0; s < k; s++) {
                const int32_t j = index[i * k + s];
                if (j < 0 || j >= n) continue;
                d[0] = (double)points[(int64_t)j * 3 + 0] - mean[0];
                d[1] = (double)points[(int64_t)j * 3 + 1] - mean[1];
                d[2] = (double)points[(int64_t)j * 3 + 2] - mean[2];
                cxx += d[0] * d[0]; cxy += d[0] * d[1]; cxz += d[0] * d[2];
                cyy += d[1] * d[1]; cyz += d[1] * d[2]; czz += d[2] * d[2];
            }
            double A[3][3] = {{cxx, cxy, cxz}, {cxy, cyy, cyz}, {cxz, cyz, czz}};
            double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
            for (int sweep = 0; sweep < NRF_POINTS_JACOBI_SWEEPS; sweep++) {
                jacobi3<0, 1>(A, V);
                jacobi3<0, 2>(A, V);
                jacobi3<1, 2>(A, V);
            }
            const double ev[3] = {A[0][0], A[1][1], A[2][2]};
            // ascending, the lowest column first on a tie: the rank of column c is the number of columns that come before it
            int at[3] = {0, 0, 0};
#pragma unroll
            for (int c = 0; c < 3; c++) {
                int rank = 0;
#pragma unroll
                for (int o = 0; o < 3; o++) rank += (ev[o] < ev[c] || (ev[o] == ev[c] && o < c)) ? 1 : 0;
#pragma unroll
                for (int r = 0; r < 3; r++) at[r] = rank == r ? c : at[r];
            }
            const double l0 = sel3(ev, at[0]), l1 = sel3(ev, at[1]), l2 = sel3(ev, at[2]);
            const double col[3] = {at[0] == 0 ? V[0][0] : (at[0] == 1 ? V[0][1] : V[0][2]), at[0] == 0 ? V[1][0] : (at[0] == 1 ? V[1][1] : V[1][2]),
                                   at[0] == 0 ? V[2][0] : (at[0] == 1 ? V[2][1] : V[2][2])};
            const double nrm = sqrt((col[0] * col[0] + col[1] * col[1]) + col[2] * col[2]);
            if (isfinite(l0) && isfinite(l1) && isfinite(l2) && l1 > 0.0 && nrm > 0.0 && isfinite(nrm)) {
                double nn[3] = {col[0] / nrm, col[1] / nrm, col[2] / nrm};
                bool flip;
                if (toward) {
                    const float *tw = toward + (toward_stride ? i * toward_stride : 0);
                    const double w[3] = {(double)tw[0] - p[0], (double)tw[1] - p[1], (double)tw[2] - p[2]};
                    flip = ((nn[0] * w[0] + nn[1] * w[1]) + nn[2] * w[2]) < 0.0;          // a NaN viewpoint flips nothing
                } else {
                    int big = 0;
                    if (fabs(nn[1]) > fabs(nn[big])) big = 1;
                    if (fabs(nn[2]) > fabs(sel3(nn, big))) big = 2;
                    flip = sel3(nn, big) < 0.0;
                }
#pragma unroll
                for (int a = 0; a < 3; a++) out_n[a] = (float)(flip ? -nn[a] : nn[a]);
                out_e[0] = (float)l0; out_e[1] = (float)l1; out_e[2] = (float)l2;
                good = true;
            }
        }
        normals[i * 3 + 0] = out_n[0]; normals[i * 3 + 1] = out_n[1]; normals[i * 3 + 2] = out_n[2];
        if (eigen) { eigen[i * 3 + 0] = out_e[0]; eigen[i * 3 + 1] = out_e[1]; eigen[i * 3 + 2] = out_e[2]; }
    }
    if (!stats) return;          // uniform
    const int total = block_count<GEO_BLOCK>(live && !good, sh);
    if (threadIdx.x == 0 && total) atomicAdd(stats + 0, (uint32_t)total);
}

__global__ void __launch_bounds__(GEO_BLOCK) k_knn_mean_distance(const float *__restrict__ dist2, int64_t n, int k, float *__restrict__ score)
{
    const int64_t i = (int64_t)blockIdx.x * GEO_BLOCK + threadIdx.x;
    if (i >= n) return;
    float sum = 0.0f;
    int m = 0;
    for (int s = 0; s < k; s++) {
        const float v = dist2[i * k + s];
        if (!(v < INFINITY)) continue;          // an empty slot (+inf), or a NaN
        sum += sqrtf(v);
        m++;
    }
    score[i] = m ? sum / (float)m : INFINITY;
}

inline int64_t pstats_blocks(int64_t n) { return n > 0 ? ceil_div(n, PSTATS_TILE) : 1; }

struct PStatsWs {
    double *partials;          // [blocks][4]
};

PStatsWs pstats_layout(Bump &b, int64_t n)
{
    PStatsWs s;
    s.partials = b.take<double>((size_t)pstats_blocks(n) * PSTATS_VALUES);
    return s;
}

__global__ void __launch_bounds__(GEO_BLOCK) k_value_stats(const float *__restrict__ values, int64_t n, double *__restrict__ partials)
{
    __shared__ double s_wave[GEO_BLOCK / 64];
    const int t = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * PSTATS_TILE;
    const int64_t left = n - first;
    const int cnt = left < PSTATS_TILE ? (int)(left > 0 ? left : 0) : PSTATS_TILE;
    double acc[PSTATS_VALUES] = {0.0, 0.0, 0.0, 0.0};
    for (int e = t; e < cnt; e += GEO_BLOCK) {
        const float v = values[first + e];
        if (!isfinite(v)) continue;
        const double x = (double)v;
        acc[0] += 1.0;
        acc[1] += x;
        acc[2] += x * x;
        acc[3] = fmax(acc[3], x);
    }
#pragma unroll
    for (int v = 0; v < PSTATS_VALUES; v++) {
        const double a = v == 3 ? ordered_block_max<GEO_BLOCK>(acc[3], s_wave) : ordered_block_sum<GEO_BLOCK>(acc[v], s_wave);
        if (t == 0) partials[(int64_t)blockIdx.x * PSTATS_VALUES + v] = a;
        __syncthreads();          // the next column goes through the same words
    }
}

__global__ void __launch_bounds__(GEO_BLOCK) k_value_stats_finish(int64_t count, const double *__restrict__ partials, double *__restrict__ out)
{
    __shared__ double s_a[GEO_BLOCK];
    for (int v = 0; v < PSTATS_VALUES; v++) {
        const double a = v == 3 ? ordered_finish<GEO_BLOCK, true>(partials, count, PSTATS_VALUES, v, s_a) : ordered_finish<GEO_BLOCK>(partials, count, PSTATS_VALUES, v, s_a);
        if (threadIdx.x == 0) out[v] = a;
    }
}

inline bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

}  // namespace nrf

using namespace nrf;

extern "C" {

size_t nrf_point_bvh_bytes(int64_t n)
{
    if (n < 0 || n > INT32_MAX) return 0;
    return measure([&](Bump &b) { bvh_layout(b, n); });
}

size_t nrf_point_bvh_workspace_bytes(int64_t n) { return bvh_build_workspace_bytes(n); }

// the checks every entry over a cloud and its BVH buffer makes
#define NRF_PBVH_CHECK(who)                                                                                                                                                \
    NRF_CHECK_ARG(n >= 0 && n <= INT32_MAX, who ": %lld points (0 .. 2^31 - 1)", (long long)n);                                                                           \
    NRF_CHECK_ARG((d_points || n == 0) && aligned_to(d_points, 4), who ": d_points must be non-null and 4-byte aligned");                                                 \
    NRF_CHECK_ARG(d_bvh && aligned_to(d_bvh, 64), who ": the BVH buffer must be non-null and 64-byte aligned");                                                           \
    NRF_CHECK_ARG(bvh_bytes == nrf_point_bvh_bytes(n), who ": a BVH buffer of %zu bytes was not built for %lld points (nrf_point_bvh_bytes gives %zu)", bvh_bytes,        \
                  (long long)n, nrf_point_bvh_bytes(n))

int nrf_point_bvh_build(const float *d_points, int64_t n, void *d_bvh, size_t bvh_bytes, uint32_t *d_stats, void *d_workspace, size_t workspace_bytes, void *stream)
{
    NRF_PBVH_CHECK("nrf_point_bvh_build");
    NRF_CHECK_ARG(aligned_to(d_stats, 4), "nrf_point_bvh_build: d_stats must be 4-byte aligned");
    NRF_CHECK_ARG(d_workspace && aligned_to(d_workspace, 8), "nrf_point_bvh_build: the workspace must be non-null and 8-byte aligned");
    return bvh_build_launch(true, d_points, n, nullptr, n, d_bvh, bvh_bytes, d_stats, d_workspace, workspace_bytes, as_stream(stream), "nrf_point_bvh_build");
}

int nrf_point_bvh_codes(const float *d_query, int64_t nq, int stride, const void *d_bvh, size_t bvh_bytes, int64_t n, uint32_t *d_codes, void *stream)
{
    NRF_CHECK_ARG(nq >= 0 && nq <= INT32_MAX, "nrf_point_bvh_codes: %lld points (0 .. 2^31 - 1)", (long long)nq);
    NRF_CHECK_ARG(stride >= 3 && stride <= NRF_RC_MAX_STRIDE, "nrf_point_bvh_codes: a stride of %d floats (3 .. %d)", stride, NRF_RC_MAX_STRIDE);
    NRF_CHECK_ARG(n >= 0 && n <= INT32_MAX, "nrf_point_bvh_codes: a cloud of %lld points (0 .. 2^31 - 1)", (long long)n);
    NRF_CHECK_ARG(d_bvh && aligned_to(d_bvh, 64), "nrf_point_bvh_codes: the BVH buffer must be non-null and 64-byte aligned");
    NRF_CHECK_ARG(bvh_bytes == nrf_point_bvh_bytes(n), "nrf_point_bvh_codes: a BVH buffer of %zu bytes was not built for %lld points (nrf_point_bvh_bytes gives %zu)",
                  bvh_bytes, (long long)n, nrf_point_bvh_bytes(n));
    NRF_CHECK_ARG(nq == 0 || (d_query && d_codes), "nrf_point_bvh_codes: null d_query or d_codes");
    NRF_CHECK_ARG(aligned_to(d_query, 4) && aligned_to(d_codes, 4), "nrf_point_bvh_codes: d_query and d_codes must be 4-byte aligned");
    if (nq == 0) return NRF_OK;
    return bvh_point_codes_launch(d_query, nq, stride, d_bvh, n, PBVH_MAGIC, d_codes, as_stream(stream));
}

int nrf_bvh_knn(const float *d_query, int64_t nq, const float *d_points, int64_t n, const void *d_bvh, size_t bvh_bytes, const int32_t *d_order, int k, float max_dist,
                int exclude_self, float *d_dist2, int32_t *d_index, int32_t *d_count, uint32_t *d_stats, void *d_workspace, size_t workspace_bytes, void *stream)
{
    (void)d_workspace;
    (void)workspace_bytes;          // nrf_bvh_query_workspace_bytes is 0: the list and the stack live in the lane; any pair is accepted
    NRF_CHECK_ARG(nq >= 0 && nq <= INT32_MAX, "nrf_bvh_knn: %lld queries (0 .. 2^31 - 1)", (long long)nq);
    NRF_CHECK_ARG(k >= 1 && k <= NRF_KNN_MAX_K, "nrf_bvh_knn: k = %d (1 .. %d)", k, NRF_KNN_MAX_K);
    NRF_PBVH_CHECK("nrf_bvh_knn");
    NRF_CHECK_ARG(exclude_self == 0 || exclude_self == 1, "nrf_bvh_knn: exclude_self must be 0 or 1 (got %d)", exclude_self);
    NRF_CHECK_ARG(nq == 0 || (d_query && d_dist2 && d_index), "nrf_bvh_knn: null d_query, d_dist2 or d_index");
    NRF_CHECK_ARG(aligned_to(d_query, 4) && aligned_to(d_dist2, 4) && aligned_to(d_index, 4) && aligned_to(d_count, 4) && aligned_to(d_order, 4) && aligned_to(d_stats, 4),
                  "nrf_bvh_knn: d_query, d_order, d_dist2, d_index, d_count and d_stats must be 4-byte aligned");
    NRF_CHECK_ARG(max_dist >= 0.0f, "nrf_bvh_knn: max_dist must be >= 0 or +inf (got %g)", (double)max_dist);          // NaN fails
    if (nq == 0) return NRF_OK;
    Bump bb(const_cast<void *>(d_bvh), bvh_bytes);
    const BvhBuf buf = bvh_layout(bb, n);
    const PtTree m = {buf.head, buf.leaf_face, buf.node, n};
    const dim3 grid((unsigned)ceil_div(nq, GEO_BLOCK)), block(GEO_BLOCK);
    const float md2 = max_dist * max_dist;
    hipStream_t st = as_stream(stream);
#define NRF_KNN_LAUNCH(KL) \
    hipLaunchKernelGGL(k_bvh_knn<KL>, grid, block, 0, st, d_query, nq, d_order, d_points, m, k, md2, exclude_self, d_dist2, d_index, d_count, d_stats)
    if (k == 1) NRF_KNN_LAUNCH(1);
    else if (k <= 8) NRF_KNN_LAUNCH(8);
    else if (k <= 16) NRF_KNN_LAUNCH(16);
    else NRF_KNN_LAUNCH(32);
#undef NRF_KNN_LAUNCH
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

int nrf_points_normals(const float *d_points, int64_t n, const int32_t *d_index, int k, const float *d_toward, int toward_stride, float *d_normals, float *d_eigen,
                       uint32_t *d_stats, void *stream)
{
    NRF_CHECK_ARG(n >= 0 && n <= INT32_MAX, "nrf_points_normals: %lld points (0 .. 2^31 - 1)", (long long)n);
    NRF_CHECK_ARG(k >= 1 && k <= NRF_KNN_MAX_K, "nrf_points_normals: k = %d (1 .. %d)", k, NRF_KNN_MAX_K);
    NRF_CHECK_ARG(toward_stride == 0 || toward_stride == 3, "nrf_points_normals: toward_stride must be 0 (one viewpoint) or 3 (one per point), got %d", toward_stride);
    NRF_CHECK_ARG(n == 0 || (d_points && d_index && d_normals), "nrf_points_normals: null d_points, d_index or d_normals");
    NRF_CHECK_ARG(aligned_to(d_points, 4) && aligned_to(d_index, 4) && aligned_to(d_toward, 4) && aligned_to(d_normals, 4) && aligned_to(d_eigen, 4) && aligned_to(d_stats, 4),
                  "nrf_points_normals: every pointer must be 4-byte aligned");
    NRF_CHECK_ARG(d_normals != d_points || n == 0, "nrf_points_normals: d_normals must not be d_points");
    if (n == 0) return NRF_OK;
    hipLaunchKernelGGL(k_points_normals, dim3((unsigned)ceil_div(n, GEO_BLOCK)), dim3(GEO_BLOCK), 0, as_stream(stream), d_points, n, d_index, k, d_toward, toward_stride,
                       d_normals, d_eigen, d_stats);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

int nrf_knn_mean_distance(const float *d_dist2, int64_t n, int k, float *d_score, void *stream)
{
    NRF_CHECK_ARG(n >= 0 && n <= INT32_MAX, "nrf_knn_mean_distance: %lld rows (0 .. 2^31 - 1)", (long long)n);
    NRF_CHECK_ARG(k >= 1 && k <= NRF_KNN_MAX_K, "nrf_knn_mean_distance: k = %d (1 .. %d)", k, NRF_KNN_MAX_K);
    NRF_CHECK_ARG(n == 0 || (d_dist2 && d_score), "nrf_knn_mean_distance: null d_dist2 or d_score");
    NRF_CHECK_ARG(aligned_to(d_dist2, 4) && aligned_to(d_score, 4), "nrf_knn_mean_distance: d_dist2 and d_score must be 4-byte aligned");
    if (n == 0) return NRF_OK;
    hipLaunchKernelGGL(k_knn_mean_distance, dim3((unsigned)ceil_div(n, GEO_BLOCK)), dim3(GEO_BLOCK), 0, as_stream(stream), d_dist2, n, k, d_score);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

size_t nrf_value_stats_workspace_bytes(int64_t n)
{
    if (n < 0 || n >= ((int64_t)1 << 40)) return 0;
    return measure([&](Bump &b) { pstats_layout(b, n); });
}

int nrf_value_stats(const float *d_values, int64_t n, double *d_out, void *d_workspace, size_t workspace_bytes, void *stream)
{
    NRF_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 40), "nrf_value_stats: %lld entries (0 .. 2^40 - 1)", (long long)n);
    NRF_CHECK_ARG(d_out && aligned_to(d_out, 8) && (d_values || n == 0) && aligned_to(d_values, 4), "nrf_value_stats: null or misaligned d_out or d_values");
    NRF_CHECK_ARG(d_workspace && aligned_to(d_workspace, 8), "nrf_value_stats: the workspace must be non-null and 8-byte aligned");
    Bump bump(d_workspace, workspace_bytes);
    const PStatsWs ws = pstats_layout(bump, n);
    NRF_TRY(ws_check(bump, nrf_value_stats_workspace_bytes(n), "nrf_value_stats"));
    hipStream_t st = as_stream(stream);
    const int64_t nb = pstats_blocks(n);
    hipLaunchKernelGGL(k_value_stats, dim3((unsigned)nb), dim3(GEO_BLOCK), 0, st, d_values, n, ws.partials);
    NRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_value_stats_finish, dim3(1), dim3(GEO_BLOCK), 0, st, nb, (const double *)ws.partials, d_out);
    NRF_LAUNCH_CHECK();
    return NRF_OK;
}

}  // extern "C"
