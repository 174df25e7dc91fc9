// raycast.h -- a (ray, face) pair judged in one place, for every structure that finds the pairs: the face grid's walk and its fallback (raycast.hip) and the BVH
// (bvh.hip).  The packed ray row, the header's INVALID rule, Moeller-Trumbore in the header's operation order with the consistency of t and P (rc_candidate), a face
// as a candidate of a ray (rc_take) and the outputs of a ray from its key (rc_write).  One copy: the two structures return the same bits because it is one function.
#pragma once

#include "reduce.h"
#include "face_grid.h"

namespace nrf {

constexpr float RC_TAU = 1.0f / 4096.0f;           // 2^NRF_RC_TAU_LOG2
static_assert(NRF_RC_TAU_LOG2 == -12, "RC_TAU is written out for -12");

struct RcRay {
    float o[3], d[3], lo, hi;          // lo = max(near, 0), hi = far
    float o_inf;                       // |o|_inf
};

struct RcHit {
    float t, v, w, p[3];
};

// the header's INVALID: a non-finite o or d, d == 0 on all axes, a NaN near or far
__device__ __forceinline__ bool rc_ray_valid(const RcRay &r, float near, float far)
{
    return finite3(r.o) && finite3(r.d) && (r.d[0] != 0.0f || r.d[1] != 0.0f || r.d[2] != 0.0f) && near == near && far == far;
}

__device__ __forceinline__ void rc_ray_finish(RcRay &r, float near, float far)
{
    r.lo = near > 0.0f ? near : 0.0f;
    r.hi = far;
    r.o_inf = fmaxf(fmaxf(fabsf(r.o[0]), fabsf(r.o[1])), fabsf(r.o[2]));
}

__device__ __forceinline__ void rc_cross(const float x[3], const float y[3], float out[3])
{
    out[0] = x[1] * y[2] - x[2] * y[1];
    out[1] = x[2] * y[0] - x[0] * y[2];
    out[2] = x[0] * y[1] - x[1] * y[0];
}

// the one place a candidate is formed and judged (the header's steps); cull: 0 none, 1 back (det > 0 accepted), 2 front (det < 0 accepted)
__device__ __forceinline__ bool rc_candidate(const RcRay &r, const float a[3], const float b[3], const float c[3], int cull, RcHit &h)
{
    float ab[3], ac[3], tv[3], p[3], q[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        ab[k] = b[k] - a[k];
        ac[k] = c[k] - a[k];
        tv[k] = r.o[k] - a[k];
    }
    rc_cross(r.d, ac, p);
    const float det = cm_dot(ab, p);
    const float inv = 1.0f / det;
    const float v = cm_dot(tv, p) * inv;
    rc_cross(tv, ab, q);
    const float w = cm_dot(r.d, q) * inv;
    const float t = cm_dot(ac, q) * inv + 0.0f;          // -0.0f becomes +0.0f: the key of -0.0f lies above every positive t
    bool ok = det != 0.0f && (cull == 0 || (cull == 1 ? det > 0.0f : det < 0.0f));
    ok = ok && v >= 0.0f && w >= 0.0f && v + w <= 1.0f && t >= r.lo && t <= r.hi && t < INFINITY;          // a NaN fails every comparison
    float raw[3];
#pragma unroll
    for (int k = 0; k < 3; k++) raw[k] = (a[k] + ab[k] * v) + ac[k] * w;
    cm_clamp_to_face(raw, a, b, c, h.p);
    float m = r.o_inf, e = 0.0f;
    bool cmp = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float pu = r.o[k] + t * r.d[k];
        const float ak = fabsf(pu), ek = fabsf(pu - h.p[k]);
        m = ak > m ? ak : m;
        cmp = cmp && ek == ek;          // a NaN difference fails
        e = ek > e ? ek : e;
    }
    ok = ok && cmp && e <= RC_TAU * m;
    h.t = t;
    h.v = v;
    h.w = w;
    return ok;
}

// face f as a candidate of ray r; best: the running key minimum
__device__ __forceinline__ void rc_take(const RcRay &r, const float *__restrict__ verts, int32_t n_verts, const int32_t *__restrict__ faces, int64_t n_faces, int64_t f,
                                        int cull, unsigned long long &best)
{
    float a[3], b[3], c[3];
    if (cm_face(verts, n_verts, faces, n_faces, f, a, b, c) != 0) return;
    RcHit h;
    if (!rc_candidate(r, a, b, c, cull, h)) return;
    const unsigned long long k = key_pack(h.t, (uint32_t)f);
    if (k < best) best = k;
}

// the outputs of ray i from its key: (v, w) and P are those of the winning face, formed once more by the same function
__device__ __forceinline__ void rc_write(const RcRay &r, int64_t i, unsigned long long best, const float *__restrict__ verts, int32_t n_verts,
                                         const int32_t *__restrict__ faces, int64_t n_faces, int cull, float *__restrict__ out_t, int32_t *__restrict__ face,
                                         float *__restrict__ uv, float *__restrict__ point, uint8_t *__restrict__ hit)
{
    const int32_t f = key_index(best);
    if (out_t) out_t[i] = key_value(best);
    if (face) face[i] = f;
    if (hit) hit[i] = f >= 0 ? 1 : 0;
    if (!uv && !point) return;
    RcHit h;
    h.v = h.w = h.p[0] = h.p[1] = h.p[2] = 0.0f;
    float a[3], b[3], c[3];
    if (f >= 0 && cm_face(verts, n_verts, faces, n_faces, f, a, b, c) == 0) (void)rc_candidate(r, a, b, c, cull, h);
    if (uv) { uv[i * 2 + 0] = h.v; uv[i * 2 + 1] = h.w; }
    if (point) { point[i * 3 + 0] = h.p[0]; point[i * 3 + 1] = h.p[1]; point[i * 3 + 2] = h.p[2]; }
}

__device__ __forceinline__ bool rc_load_ray(const float *__restrict__ rays, int64_t i, int stride, RcRay &r)
{
    const float *row = rays + i * stride;
#pragma unroll
    for (int k = 0; k < 3; k++) { r.o[k] = row[k]; r.d[k] = row[3 + k]; }
    const float near = row[6], far = row[7];
    rc_ray_finish(r, near, far);
    return rc_ray_valid(r, near, far);
}

}  // namespace nrf
