"""numpy restatement of the closest-point-on-a-mesh contract (include/nerfpp_hip.h: nrf_face_grid_count / _build, nrf_closest_on_mesh): one numpy fp32 operation per
source operation and brute force over all (query, face) pairs; it knows nothing of grids, cell boxes, large lists or rings.  The GPU tests compare with it bit for
bit.  Also the inputs the host and GPU tests share.  Imports nothing of the package."""
import numpy as np

import geometry_ref as G

F32 = np.float32
FG_MAX_FACE_CELLS = 64
REGIONS = ("A", "B", "AB", "C", "AC", "BC", "interior")          # the order the header tests them in
NONE = (G.INF_BITS << np.uint64(32)) | np.uint64(0xFFFFFFFF)


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def closest_on_triangle(q, a, b, c):
    """The header's closest point, q / a / b / c [..., 3] f32 (broadcast against each other) -> dict(d2, v, w, p [..., 3], region (index into REGIONS), raw: P before
    the clamp)"""
    q, a, b, c = (np.asarray(x, F32) for x in (q, a, b, c))
    one, zero = F32(1), F32(0)
    with np.errstate(all="ignore"):
        ab, ac, ap, bp, cp = b - a, c - a, q - a, q - b, q - c
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6), (vb <= 0) & (d2 >= 0) & (d6 <= 0),
                 (va <= 0) & (e43 >= 0) & (e56 >= 0)]
        region = np.select(conds, list(range(6)), 6)
        v_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = e43 / (e43 + e56)
        denom = one / ((va + vb) + vc)
        v_in, w_in = vb * denom, vc * denom
        full = np.broadcast(region, zero).shape
        z, o = np.zeros(full, F32), np.ones(full, F32)
        v = np.select([region == k for k in range(6)], [z, o, v_ab, z, z, one - w_bc], v_in).astype(F32)
        w = np.select([region == k for k in range(6)], [z, z, z, o, w_ac, w_bc], w_in).astype(F32)
        shape = full + (3,)
        cands = [np.broadcast_to(a, shape), np.broadcast_to(b, shape), a + v_ab[..., None] * ab, np.broadcast_to(c, shape), a + w_ac[..., None] * ac,
                 b + w_bc[..., None] * (c - b), (a + ab * v_in[..., None]) + ac * w_in[..., None]]
        raw = np.select([(region == k)[..., None] for k in range(6)], cands[:6], cands[6]).astype(F32)
        lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
        p = np.where(raw < lo, lo, np.where(raw > hi, hi, raw)).astype(F32)
        dx, dy, dz = q[..., 0] - p[..., 0], q[..., 1] - p[..., 1], q[..., 2] - p[..., 2]
        dd = (dx * dx + dy * dy) + dz * dz
    for x in (v, w, raw, p, dd, v_ab, w_bc, denom):
        assert x.dtype == F32
    return dict(d2=dd, v=v, w=w, p=p, region=region, raw=raw)


def face_classes(verts, faces):
    """-> (cls [F]: 0 a face, 1 bad (a corner outside [0, V)), 2 non-finite (a non-finite vertex coordinate); a, b, c [F, 3] f32, zeros where cls != 0)"""
    P = np.asarray(verts, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    bad = ((f < 0) | (f >= len(P))).any(-1) if len(P) else np.ones(len(f), bool)
    g = np.where(bad[:, None], 0, f)
    if len(P) == 0:
        P = np.zeros((1, 3), F32)
    tri = P[g]
    nonfinite = ~bad & ~np.isfinite(tri).all(axis=(1, 2))
    cls = np.where(bad, 1, np.where(nonfinite, 2, 0))
    tri = np.where((cls == 0)[:, None, None], tri, F32(0))
    return cls, tri[:, 0], tri[:, 1], tri[:, 2]


def closest(query, verts, faces, max_dist=np.inf, chunk=128):
    """All pairs -> dict(d2 [nq] f32, face [nq] i32, uv [nq, 2] f32, point [nq, 3] f32, stats [4] u32: non-finite queries, bad faces, non-finite faces, 0)"""
    q = np.asarray(query, F32).reshape(-1, 3)
    cls, a, b, c = face_classes(verts, faces)
    valid = cls == 0
    qf = np.isfinite(q).all(-1)
    with np.errstate(all="ignore"):
        md2 = F32(max_dist) * F32(max_dist)
    best = np.full(len(q), NONE, np.uint64)
    idx = np.arange(len(cls), dtype=np.uint64)
    if len(cls):
        for c0 in range(0, len(q), chunk):
            r = closest_on_triangle(q[c0:c0 + chunk, None, :], a[None], b[None], c[None])
            key = (r["d2"].view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx[None]
            ok = valid[None] & qf[c0:c0 + chunk, None] & (r["d2"] <= md2)          # a NaN d2 fails the comparison
            best[c0:c0 + chunk] = np.where(ok, key, NONE).min(1)
    d2 = (best >> np.uint64(32)).astype(np.uint32).view(F32)
    face = (best & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    uv, point = np.zeros((len(q), 2), F32), np.zeros((len(q), 3), F32)
    hit = face >= 0
    if hit.any():
        r = closest_on_triangle(q[hit], a[face[hit]], b[face[hit]], c[face[hit]])
        uv[hit] = np.stack([r["v"], r["w"]], -1)
        point[hit] = r["p"]
        assert np.array_equal(r["d2"].view(np.uint32), d2[hit].view(np.uint32))
    stats = np.array([(~qf).sum(), (cls == 1).sum(), (cls == 2).sum(), 0], np.uint32)
    return dict(d2=d2, face=face, uv=uv, point=point, stats=stats)


def interpolate(attr, faces, face, uv):
    """InterpolateAttributes in fp32: (1 - u - v) a0 + u a1 + v a2 of each row's face, zeros where face < 0"""
    a = np.asarray(attr, F32).reshape(len(attr), -1)
    f = np.asarray(faces, np.int64)[np.maximum(face, 0)]
    u, v = uv[:, :1].astype(F32), uv[:, 1:].astype(F32)
    out = (F32(1) - u - v) * a[f[:, 0]] + u * a[f[:, 1]] + v * a[f[:, 2]]
    assert out.dtype == F32
    return np.where((face >= 0)[:, None], out, F32(0))


# ---- the inputs of the tests ----
TRIANGLE = (np.array([0, 0, 0], F32), np.array([1, 0, 0], F32), np.array([0, 1, 0], F32))
REGION_QUERIES = np.array([[-1, -1, 0.5], [2, -0.5, 0.3], [0.5, -1, 0.2], [-0.5, 2, -0.4], [-1, 0.5, 0.1], [1, 1, -0.2], [0.25, 0.25, 1],          # one per region, in order
                           [-0.1, -0.2, 0], [1.5, 0.2, 0], [0.3, -0.01, 3], [-0.2, 1.3, 0], [-0.01, 0.4, -2], [0.6, 0.6, 0.1], [0.1, 0.7, -0.5]], F32)


def mesh_queries(verts, faces, seed, n_random=300, n_surface=300):
    """Queries of every kind around a mesh of valid faces: random points in and around the box, surface samples, vertices, edge midpoints, centroids, points along
    the face normals on both sides, and rows with a NaN or an infinity -> [n, 3] f32"""
    rng = np.random.default_rng(seed)
    V = np.asarray(verts, F32)
    tri = V[np.asarray(faces, np.int64)]
    lo, hi = V.min(0).astype(np.float64), V.max(0).astype(np.float64)
    ext = hi - lo
    rnd = rng.uniform(lo - 0.5 * ext, hi + 0.5 * ext, (n_random, 3)).astype(F32)
    f = rng.integers(0, len(tri), n_surface)
    u, v = rng.uniform(0, 1, n_surface), rng.uniform(0, 1, n_surface)
    flip = u + v > 1
    u, v = np.where(flip, 1 - u, u)[:, None], np.where(flip, 1 - v, v)[:, None]
    t64 = tri.astype(np.float64)
    surf = ((1 - u - v) * t64[f, 0] + u * t64[f, 1] + v * t64[f, 2]).astype(F32)
    mids = np.concatenate([F32(0.5) * (tri[:, 0] + tri[:, 1]), F32(0.5) * (tri[:, 1] + tri[:, 2]), F32(0.5) * (tri[:, 2] + tri[:, 0])])
    cen = t64.mean(1)
    n = np.cross(t64[:, 1] - t64[:, 0], t64[:, 2] - t64[:, 0])
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)
    along = np.concatenate([cen + s * ext.max() * n for s in (0.05, -0.05, 0.6)]).astype(F32)
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan]], F32)
    return np.concatenate([rnd, surf, V, mids, cen.astype(F32), along, bad]).astype(F32)


def search_clamp_cases(seed=0, n=100000):
    """A bounded random search for (triangle, query) pairs whose UNCLAMPED P leaves the face's coordinate box -> (a, b, c, q [k, 3] each, region [k]).  It looks where
    the rounding can do it: queries beyond edge AB that project very near b, so that v = d1 / (d1 - d3) is just below 1 and a + v * fl(b - a) can round past b."""
    rng = np.random.default_rng(seed)
    a, b, c = (rng.uniform(-1, 1, (n, 3)).astype(F32) for _ in range(3))
    a = (a * 10.0 ** rng.uniform(-3, 0, (n, 1))).astype(F32)
    a64, b64, c64 = (x.astype(np.float64) for x in (a, b, c))
    t = 1.0 - 10.0 ** rng.uniform(-9, -1, (n, 1))
    nrm = np.cross(b64 - a64, c64 - a64)
    outward = np.cross(nrm, b64 - a64)                                   # in the face's plane, across AB
    outward *= np.sign((outward * (a64 - c64)).sum(-1, keepdims=True))          # away from c
    q = (a64 + t * (b64 - a64) + 1e-3 * outward).astype(F32)
    r = closest_on_triangle(q, a, b, c)
    lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
    out = ((r["raw"] < lo) | (r["raw"] > hi)).any(-1)
    return a[out], b[out], c[out], q[out], r["region"][out]
