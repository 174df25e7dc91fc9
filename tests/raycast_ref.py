"""numpy restatement of the ray-casting contract (include/nerfpp_hip.h: nrf_ray_cast_mesh, nrf_hemisphere_dirs, nrf_mesh_ambient_occlusion): one numpy fp32
operation per source operation and brute force over all (ray, face) pairs; it knows nothing of grids, clipping, steps or fallbacks.  The GPU tests compare with it bit
for bit.  Also the ray sets the host and GPU tests share.  Imports nothing of the package."""
import numpy as np

import closest_ref as CR
import geometry_ref as G

F32 = np.float32
CLOSEST, ANY = 0, 1
CULL_NONE, CULL_BACK, CULL_FRONT = 0, 1, 2
TAU_LOG2, MAX_STEPS, MAX_STRIDE = -12, 1024, 64
HEMI_ATTEMPTS, HEMI_MAX_K, HEMI_MAX_INDEX, HEMI_MIN_LEN2 = 8, 65536, 1 << 40, F32(2.0 ** -20)
RNG_HEMI_DIR = 12
NONE = CR.NONE
INF = F32(np.inf)


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def _cross(x, y):
    return np.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1], x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2], x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], -1)


def ray_parts(rays):
    """rays [n, >= 8] -> (o, d [n, 3], lo, hi [n], valid [n]): the header's range and INVALID rule"""
    r = np.asarray(rays, F32)
    o, d, near, far = r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7]
    valid = np.isfinite(o).all(-1) & np.isfinite(d).all(-1) & (d != 0).any(-1) & ~np.isnan(near) & ~np.isnan(far)
    lo = np.where(near > 0, near, F32(0)).astype(F32)
    return o, d, lo, far, valid


def candidate(o, d, lo, hi, a, b, c, cull=CULL_NONE, tau_log2=TAU_LOG2):
    """The header's candidate; o, d [..., 3], lo, hi [...], a, b, c [..., 3] broadcast against each other -> dict(ok, t, v, w, p, ratio: |Pu - P|_inf /
    max(|o|_inf, |Pu|_inf) in float64, before: accepted but for the consistency rule)"""
    o, d, a, b, c = (np.asarray(x, F32) for x in (o, d, a, b, c))
    with np.errstate(all="ignore"):
        ab, ac = b - a, c - a
        p = _cross(np.broadcast_to(d, np.broadcast(d, ac).shape), ac)
        det = _dot(ab, p)
        inv = F32(1) / det
        tv = o - a
        v = _dot(tv, p) * inv
        q = _cross(tv, ab)
        w = _dot(np.broadcast_to(d, q.shape), q) * inv
        t = _dot(ac, q) * inv + F32(0)
        ok = det != 0
        if cull == CULL_BACK:
            ok = ok & (det > 0)
        elif cull == CULL_FRONT:
            ok = ok & (det < 0)
        ok = ok & (v >= 0) & (w >= 0) & (v + w <= F32(1)) & (t >= lo) & (t <= hi) & (t < INF)
        raw = (a + ab * v[..., None]) + ac * w[..., None]
        lo3, hi3 = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
        P = np.where(raw < lo3, lo3, np.where(raw > hi3, hi3, raw)).astype(F32)
        tf = np.where(np.isfinite(t), t, F32(0))[..., None]          # a t that is not finite is rejected above; keep the arithmetic below free of inf * 0
        Pu = o + tf * d
        m = np.maximum(np.abs(o).max(-1), np.abs(Pu).max(-1))
        e = np.abs(Pu - P)
        emax = e.max(-1)          # NaN propagates: a NaN difference fails the comparison
        tau = F32(2.0 ** tau_log2) * m
        before = ok
        ok = ok & (emax <= tau)
        ratio = emax.astype(np.float64) / np.maximum(m.astype(np.float64), 1e-300)
    for x in (t, v, w, P, Pu, tau, det):
        assert x.dtype == F32
    return dict(ok=ok, t=t, v=v, w=w, p=P, ratio=ratio, before=before)


def cast(rays, verts, faces, cull=CULL_NONE, chunk=128, tau_log2=TAU_LOG2):
    """All pairs -> dict(t [n] f32, face [n] i32, uv [n, 2], point [n, 3], hit [n] u8, stats [4] u32: invalid rays, bad faces, non-finite faces, 0; ratio: the largest
    consistency ratio over candidates accepted but for that rule; rejected: how many such candidates the rule removed)"""
    o, d, lo, hi, valid_ray = ray_parts(rays)
    cls, a, b, c = CR.face_classes(verts, faces)
    valid = cls == 0
    n = len(o)
    best = np.full(n, NONE, np.uint64)
    idx = np.arange(len(cls), dtype=np.uint64)
    ratio, rejected = 0.0, 0
    if len(cls):
        for c0 in range(0, n, chunk):
            s = slice(c0, c0 + chunk)
            r = candidate(o[s, None, :], d[s, None, :], lo[s, None], hi[s, None], a[None], b[None], c[None], cull, tau_log2)
            live = valid[None] & valid_ray[s, None]
            key = (r["t"].view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx[None]
            best[s] = np.where(r["ok"] & live, key, NONE).min(1)
            pre = r["before"] & live
            if pre.any():
                ratio = max(ratio, float(r["ratio"][pre].max()))
            rejected += int((pre & ~r["ok"]).sum())
    t = (best >> np.uint64(32)).astype(np.uint32).view(F32)
    face = (best & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    uv, point = np.zeros((n, 2), F32), np.zeros((n, 3), F32)
    hit = face >= 0
    if hit.any():
        f = face[hit]
        r = candidate(o[hit], d[hit], lo[hit], hi[hit], a[f], b[f], c[f], cull, tau_log2)
        assert r["ok"].all() and np.array_equal(r["t"].view(np.uint32), t[hit].view(np.uint32))
        uv[hit] = np.stack([r["v"], r["w"]], -1)
        point[hit] = r["p"]
    stats = np.array([(~valid_ray).sum(), (cls == 1).sum(), (cls == 2).sum(), 0], np.uint32)
    return dict(t=t, face=face, uv=uv, point=point, hit=hit.astype(np.uint8), stats=stats, ratio=ratio, rejected=rejected)


# ---- hemisphere directions and ambient occlusion ----
def unit_normals(normals):
    """-> (n-hat [n, 3] f32, zeros for a bad normal; ok [n])"""
    nrm = np.asarray(normals, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        l2 = _dot(nrm, nrm)
        ok = np.isfinite(nrm).all(-1) & (l2 > 0) & (l2 < INF)
        nh = nrm / np.sqrt(np.where(ok, l2, F32(1)))[:, None]
    assert nh.dtype == F32
    return np.where(ok[:, None], nh, F32(0)), ok


def hemisphere_dirs(normals, k, seed=0, index0=0):
    """-> (dirs [n, k, 3] f32, stats0: the bad normals)"""
    nh, ok = unit_normals(normals)
    n = len(nh)
    i = (np.arange(n, dtype=np.uint64) + np.uint64(index0))[:, None]
    j = np.arange(k, dtype=np.uint64)[None]
    base = (i << np.uint64(20)) | (j << np.uint64(4))
    q = np.zeros((n, k, 3), F32)
    q[..., 2] = 1
    done = np.zeros((n, k), bool)
    for a in range(HEMI_ATTEMPTS):
        x1 = F32(2) * G.rng_uniform(seed, RNG_HEMI_DIR, base | np.uint64(2 * a)) - F32(1)
        x2 = F32(2) * G.rng_uniform(seed, RNG_HEMI_DIR, base | np.uint64(2 * a + 1)) - F32(1)
        s = x1 * x1 + x2 * x2
        take = ~done & (s < 1)
        with np.errstate(invalid="ignore"):
            rr = np.sqrt(F32(1) - s)
        cand = np.stack([(F32(2) * x1) * rr, (F32(2) * x2) * rr, F32(1) - F32(2) * s], -1)
        q = np.where(take[..., None], cand, q).astype(F32)
        done |= take
    v = nh[:, None, :] + q
    l2 = _dot(v, v)
    small = l2 < HEMI_MIN_LEN2
    dirs = np.where(small[..., None], nh[:, None, :], v / np.sqrt(np.where(small, F32(1), l2))[..., None])
    assert dirs.dtype == F32 and l2.dtype == F32
    return np.where(ok[:, None, None], dirs, F32(0)).astype(F32), int((~ok).sum())


def ao_rays(points, normals, k, offset, max_dist, seed=0, index0=0):
    """The rays of nrf_mesh_ambient_occlusion as packed rows [n * k, 8]"""
    p = np.asarray(points, F32).reshape(-1, 3)
    nh, _ = unit_normals(normals)
    dirs, _ = hemisphere_dirs(normals, k, seed, index0)
    with np.errstate(all="ignore"):
        o = p + F32(offset) * nh
    rays = np.zeros((len(p), k, 8), F32)
    rays[..., 0:3] = o[:, None, :]
    rays[..., 3:6] = dirs
    rays[..., 7] = F32(max_dist)
    return rays.reshape(-1, 8)


def ambient_occlusion(points, normals, k, offset, max_dist, verts, faces, seed=0, index0=0):
    """-> (ao [n] f32, stats0: invalid rays)"""
    rays = ao_rays(points, normals, k, offset, max_dist, seed, index0)
    r = cast(rays, verts, faces)
    hits = r["hit"].reshape(-1, k).astype(np.int64).sum(1)
    ao = (k - hits).astype(F32) / F32(k)
    assert ao.dtype == F32
    return ao, int(r["stats"][0])


def clip_rays(rays, t, band, miss="keep"):
    """ClipRaysToMesh: near = max(near, t - band), far = min(far, t + band) on a hit (t finite); a miss keeps its range or gets near = 1, far = 0"""
    out = np.array(rays, F32, copy=True)
    t = np.asarray(t, F32)
    hit = np.isfinite(t)
    with np.errstate(all="ignore"):
        near, far = np.maximum(out[:, 6], t - F32(band)), np.minimum(out[:, 7], t + F32(band))
    out[:, 6] = np.where(hit, near, F32(1) if miss == "empty" else out[:, 6])
    out[:, 7] = np.where(hit, far, F32(0) if miss == "empty" else out[:, 7])
    return out


# ---- the inputs of the tests ----
def pack(o, d, near=0.0, far=np.inf):
    o, d = np.asarray(o, F32).reshape(-1, 3), np.asarray(d, F32).reshape(-1, 3)
    r = np.zeros((len(o), 8), F32)
    r[:, 0:3], r[:, 3:6] = o, d
    r[:, 6], r[:, 7] = near, far
    return r


def mesh_rays(verts, faces, seed, n=200, box=None):
    """Rays of every kind around a mesh of valid faces -> (rays [m, 8] f32, kinds: {name: slice}).  Kinds: outside (random origins around the mesh aimed into it),
    inside (origins near the centre), zero (one direction component exactly 0), axis (axis-parallel rays that start on multiples of an eighth of the box: cell
    boundaries of the power-of-two grids), vertex / edge (aimed at vertices and edge midpoints), plane (origin in a face's plane, direction in that plane or leaving
    it), finite (far finite, some before the surface), empty (near > far, far < 0), invalid (NaN, inf, d = 0, NaN near / far)"""
    rng = np.random.default_rng(seed)
    V = np.asarray(verts, F32)
    tri = V[np.asarray(faces, np.int64)]
    lo, hi = (V.min(0), V.max(0)) if box is None else (np.asarray(box[:3], F32), np.asarray(box[3:], F32))
    cen, ext = ((lo + hi) / 2).astype(np.float64), float((hi - lo).max())

    def unit(m):
        x = rng.standard_normal((m, 3))
        return x / np.linalg.norm(x, axis=1, keepdims=True)
    sets, kinds = [], {}

    def add(name, r):
        at = sum(len(s) for s in sets)
        kinds[name] = slice(at, at + len(r))
        sets.append(np.asarray(r, F32))
    o = cen + unit(n) * rng.uniform(0.8, 2.5, (n, 1)) * ext
    add("outside", pack(o, cen + unit(n) * rng.uniform(0, 0.6, (n, 1)) * ext - o))
    o = cen + unit(n) * rng.uniform(0, 0.2, (n, 1)) * ext
    add("inside", pack(o, unit(n) * rng.uniform(0.1, 3, (n, 1))))
    o = cen + unit(n) * rng.uniform(0.0, 1.5, (n, 1)) * ext
    d = cen + unit(n) * rng.uniform(0, 0.5, (n, 1)) * ext - o
    d[np.arange(n), rng.integers(0, 3, n)] = 0
    add("zero", pack(o, d))
    o = lo.astype(np.float64) + np.round(rng.uniform(-2, 10, (n, 3))) / 8 * (hi - lo).astype(np.float64)
    d = np.zeros((n, 3))
    d[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-1.0, 1.0, 0.25], n)
    add("axis", pack(o, d))
    o = cen + unit(n) * rng.uniform(0.0, 2.0, (n, 1)) * ext
    add("vertex", pack(o, V[rng.integers(0, len(V), n)].astype(np.float64) - o))
    f, e = rng.integers(0, len(tri), n), rng.integers(0, 3, n)
    mid = F32(0.5) * (tri[f, e] + tri[f, (e + 1) % 3])
    add("edge", pack(o, mid.astype(np.float64) - o))
    f = rng.integers(0, len(tri), n)
    w = rng.dirichlet((1, 1, 1), n)
    start = (w[:, :, None] * tri[f]).sum(1).astype(F32)          # about in the plane of face f
    at_corner = n // 4
    start[:at_corner] = tri[f[:at_corner], 0]                    # exactly a corner
    d = np.where((np.arange(n) % 2 == 0)[:, None], tri[f, 1] - tri[f, 0], unit(n))
    add("plane", pack(start, d))
    o = cen + unit(n) * rng.uniform(0.8, 2.0, (n, 1)) * ext
    add("finite", pack(o, cen - o, near=rng.uniform(0, 0.5, n), far=rng.uniform(0.3, 1.5, n)))
    add("empty", pack(o[:16], (cen - o)[:16], near=np.where(np.arange(16) % 2 == 0, 2.0, 0.0), far=np.where(np.arange(16) % 2 == 0, 1.0, -0.5)))
    bad = pack(o[:7], (cen - o)[:7])
    bad[0, 0], bad[1, 4], bad[2, 2], bad[3, 3:6], bad[4, 6], bad[5, 7], bad[6, 5] = np.nan, np.inf, -np.inf, 0, np.nan, np.nan, np.nan
    add("invalid", bad)
    return np.concatenate(sets).astype(F32), kinds


def floor_mesh(verts, faces, z, half):
    """The mesh plus a quad of two faces in the plane `z` (a cell boundary of a grid whose box is symmetric about z with an even dim)"""
    nv = len(verts)
    quad = np.array([[-half, -half, z], [half, -half, z], [half, half, z], [-half, half, z]], F32)
    return np.concatenate([verts, quad]).astype(F32), np.concatenate([faces, np.array([[nv, nv + 1, nv + 2], [nv, nv + 2, nv + 3]], np.int32)]).astype(np.int32)


def camera_rays(h, w, K, c2w):
    """GetRays in numpy fp32, as the project's rays.hip forms them: d = ((i - cx) / fx, -(j - cy) / fy, -1) rotated by c2w -> (o, d) [h * w, 3]"""
    K, c2w = np.asarray(K, F32).reshape(3, 3), np.asarray(c2w, F32).reshape(-1, 4)[:3]
    j, i = np.mgrid[0:h, 0:w]
    dx = (i.astype(F32) - K[0, 2]) / K[0, 0]
    dy = -(j.astype(F32) - K[1, 2]) / K[1, 1]
    dz = -np.ones_like(dx)
    dirs = np.stack([dx, dy, dz], -1).astype(F32)
    d = (dirs[..., None, 0] * c2w[:, 0] + dirs[..., None, 1] * c2w[:, 1]) + dirs[..., None, 2] * c2w[:, 2]
    o = np.broadcast_to(c2w[:, 3], d.shape)
    return o.reshape(-1, 3).astype(F32), d.reshape(-1, 3).astype(F32)
