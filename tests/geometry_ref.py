"""numpy restatement of the geometry contract (include/nerfpp_hip.h: nrf_mesh_sample_count / _emit, nrf_nearest_points, nrf_distance_stats): one numpy fp32 operation
per source operation, the fp64 sums in the header's order, and a nearest-neighbour search that is brute force over all pairs and knows nothing of grids.  The GPU tests
compare with it bit for bit.  Also the inputs the host and GPU tests share.  Imports nothing of the package."""
import numpy as np

from ordered_sum_ref import block_sums as _block_sums, finish as _finish          # the ordered fp64 sums

F32 = np.float32
RNG_SURFACE_COUNT, RNG_SURFACE_UV = 10, 11
SAMPLE_MAX_PER_FACE = 65536
NN_MAX_DIM, NN_MAX_CELLS, NN_MAX_RINGS, STATS_MAX_TAU = 1024, 1 << 26, 16, 4
STATS_TILE = 4096
INF_BITS = np.uint64(0x7F800000)


# ---- include/nrf_rng.h ----
def rng_u32(seed, stream, idx):
    with np.errstate(over="ignore"):
        x = np.uint64(seed) + np.asarray(idx, np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        x = x ^ (np.uint64(stream) * np.uint64(0xD1B54A32D192ED03))
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return (x >> np.uint64(32)).astype(np.uint32)


def rng_uniform(seed, stream, idx):
    return (rng_u32(seed, stream, idx) >> np.uint32(8)).astype(F32) * F32(1.0 / 16777216.0)


# ---- 1. surface sampling ----
def _corners(verts, faces):
    """-> (bad [F], v0, e1, e2 [F,3] f32 (of vertex 0 where bad), finite [F])"""
    P = np.asarray(verts, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    bad = ((f < 0) | (f >= len(P))).any(-1) if len(P) else np.ones(len(f), bool)
    if len(P) == 0:
        P = np.zeros((1, 3), F32)
    g = np.where(bad[:, None], 0, f)
    with np.errstate(all="ignore"):
        v0, v1, v2 = P[g[:, 0]], P[g[:, 1]], P[g[:, 2]]
        e1, e2 = v1 - v0, v2 - v0
    finite = np.isfinite(v0).all(-1) & np.isfinite(v1).all(-1) & np.isfinite(v2).all(-1)
    return bad, v0, e1, e2, finite


def face_areas(verts, faces):
    """step 1 -> (area [F] f32, valid [F]: neither bad nor non-finite, bad [F])"""
    bad, _, e1, e2, finite = _corners(verts, faces)
    with np.errstate(all="ignore"):
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        s = (cx * cx + cy * cy) + cz * cz
        area = F32(0.5) * np.sqrt(s)
    assert area.dtype == F32
    return area, ~bad & finite & np.isfinite(area), bad


def sample_count(verts, faces, density, seed):
    """steps 1-5 -> dict(count [F] i32, offset [F] i64, n_points, total_area (float64), stats [3] u32: bad, non-finite, clamped)"""
    area, valid, bad = face_areas(verts, faces)
    nf = len(area)
    with np.errstate(all="ignore"):
        a = area * F32(density)
        fa = np.floor(a)
        frac = a - fa
        draw = rng_uniform(seed, RNG_SURFACE_COUNT, np.arange(nf, dtype=np.uint64)) < frac
        huge = fa > F32(SAMPLE_MAX_PER_FACE)
        n = np.where(huge | ~valid, 0, fa).astype(np.int64) + draw
    n = np.where(huge, SAMPLE_MAX_PER_FACE + 1, n)
    clamped = valid & (n > SAMPLE_MAX_PER_FACE)
    n = np.where(valid, np.minimum(n, SAMPLE_MAX_PER_FACE), 0)
    offset = np.cumsum(n) - n
    lanes = np.zeros(-(-max(nf, 1) // 256) * 256)
    lanes[:nf] = np.where(valid, area.astype(np.float64), 0.0)
    total_area = _finish(_block_sums(lanes.reshape(-1, 256))) if nf else 0.0
    stats = np.array([bad.sum(), (~bad & ~valid).sum(), clamped.sum()], np.uint32)
    return dict(count=n.astype(np.int32), offset=offset, n_points=int(n.sum()), total_area=float(total_area), stats=stats)


def sample_emit(verts, faces, seed, counted):
    """step 6 -> (points [n,3] f32, face [n] i32, uv [n,2] f32)"""
    n = counted["n_points"]
    f = np.repeat(np.arange(len(counted["count"])), counted["count"])
    p = np.arange(n, dtype=np.uint64)
    u = rng_uniform(seed, RNG_SURFACE_UV, np.uint64(2) * p)
    v = rng_uniform(seed, RNG_SURFACE_UV, np.uint64(2) * p + np.uint64(1))
    flip = u + v > F32(1)
    u, v = np.where(flip, F32(1) - u, u), np.where(flip, F32(1) - v, v)
    _, v0, e1, e2, _ = _corners(verts, np.asarray(faces).reshape(-1, 3)[f] if n else np.zeros((0, 3), np.int64))
    pts = (v0 + u[:, None] * e1) + v[:, None] * e2
    assert pts.dtype == F32
    return pts.reshape(-1, 3), f.astype(np.int32), np.stack([u, v], -1).astype(F32).reshape(-1, 2)


def sample(verts, faces, density, seed):
    c = sample_count(verts, faces, density, seed)
    return (c,) + sample_emit(verts, faces, seed, c)


# ---- 2. nearest points: all pairs ----
def nearest(query, target, max_dist=np.inf, chunk=256):
    """-> (d2 [nq] f32, index [nq] i32, stats [2] u32: non-finite queries, non-finite targets)"""
    q = np.asarray(query, F32).reshape(-1, 3)
    t = np.asarray(target, F32).reshape(-1, 3)
    qf, tf = np.isfinite(q).all(-1), np.isfinite(t).all(-1)
    with np.errstate(all="ignore"):
        md2 = F32(max_dist) * F32(max_dist)
    none = (INF_BITS << np.uint64(32)) | np.uint64(0xFFFFFFFF)
    best = np.full(len(q), none, np.uint64)
    idx = np.arange(len(t), dtype=np.uint64)
    if len(t):
        for c0 in range(0, len(q), chunk):
            qq = q[c0:c0 + chunk]
            with np.errstate(all="ignore"):
                dx, dy, dz = qq[:, None, 0] - t[None, :, 0], qq[:, None, 1] - t[None, :, 1], qq[:, None, 2] - t[None, :, 2]
                d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == F32
            key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx[None]
            ok = tf[None] & qf[c0:c0 + chunk, None] & (d2 <= md2)
            best[c0:c0 + chunk] = np.where(ok, key, none).min(1)
    d2 = (best >> np.uint64(32)).astype(np.uint32).view(F32)
    index = (best & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    return d2, index, np.array([(~qf).sum(), (~tf).sum()], np.uint32)


# ---- 3. distance statistics ----
def distance_stats(d2, taus=()):
    """-> [4 + n_tau] float64: count, sum d, sum d2, max d, count(d <= tau_k) over the finite entries, in the header's order"""
    v = np.asarray(d2, F32).reshape(-1)
    taus = [F32(t) for t in taus]
    nb = max(1, -(-len(v) // STATS_TILE))
    pad = np.full(nb * STATS_TILE, np.inf, F32)
    pad[:len(v)] = v
    fin = np.isfinite(pad)
    with np.errstate(all="ignore"):
        d = np.sqrt(np.where(fin, pad, F32(0)))
    assert d.dtype == F32
    cols = [fin.astype(np.float64), np.where(fin, d.astype(np.float64), 0.0), np.where(fin, pad.astype(np.float64), 0.0), np.where(fin, d.astype(np.float64), 0.0)]
    cols += [(fin & (d <= t)).astype(np.float64) for t in taus]
    out = []
    for k, c in enumerate(cols):
        c = c.reshape(nb, STATS_TILE // 256, 256)
        if k == 3:
            out.append(c.max() if len(v) else 0.0)
            continue
        lanes = np.zeros((nb, 256))
        for i in range(STATS_TILE // 256):          # lane t: entries t, t + 256, ... in ascending order
            lanes = lanes + c[:, i]
        out.append(_finish(_block_sums(lanes)))
    return np.array(out, np.float64)


# ---- 4. the Python layer's composition ----
def surface_distance(pa, pb, taus=(), max_dist=np.inf):
    """SurfaceDistance of two point sets (pa the prediction, pb the truth), composed by hand from the pieces above -> dict of float64"""
    sa = distance_stats(nearest(pa, pb, max_dist)[0], taus)
    sb = distance_stats(nearest(pb, pa, max_dist)[0], taus)
    na, nb = np.float64(len(pa)), np.float64(len(pb))
    with np.errstate(all="ignore"):
        acc, comp = sa[1] / sa[0], sb[1] / sb[0]
        p, r = sa[4:] / na, sb[4:] / nb
        f = np.where(p + r > 0, 2.0 * p * r / (p + r), 0.0)
        return dict(Accuracy=acc, Completeness=comp, Chamfer=0.5 * (acc + comp), ChamferSq=sa[2] / sa[0] + sb[2] / sb[0], Hausdorff=max(sa[3], sb[3]),
                    Precision=p, Recall=r, FScore=f)


# ---- the inputs of the tests ----
def next_float(x, up=True):
    return np.nextafter(F32(x), F32(np.inf if up else -np.inf))


def adversarial_mesh():
    """Every class of face at least once -> (verts, faces, dict(bad, nonfinite, clamped, zero: the indices of the faces of each kind))"""
    v = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0.5, 0.5, 1),                      # 0-3 ordinary
         (2, 2, 2), (3, 3, 3), (4, 4, 4),                                      # 4-6 collinear (exactly: integers)
         (np.nan, 0, 0), (np.inf, 1, 1), (0, -np.inf, 2),                      # 7-9
         (-300, -300, 0), (300, -300, 0), (0, 300, 0),                         # 10-12 a face of area 1.8e5: clamps at density 1
         (3e19, 0, 0), (0, 3e19, 0), (0, 0, 3e19)]                             # 13-15 finite corners whose area overflows
    f = [(0, 1, 2), (0, 1, 3), (1, 2, 3), (0, 2, 3),                           # 0-3 ordinary
         (0, 0, 1), (2, 2, 2),                                                 # 4-5 zero area by index
         (4, 5, 6),                                                            # 6 zero area by collinearity
         (-1, 0, 1), (0, 16, 1), (0, 1, 2 ** 31 - 1),                          # 7-9 bad
         (7, 0, 1), (0, 8, 1), (0, 1, 9),                                      # 10-12 non-finite vertex
         (13, 14, 15),                                                         # 13 non-finite area
         (10, 11, 12),                                                         # 14 clamped
         (0, 3, 1)]
    kinds = dict(zero=[4, 5, 6], bad=[7, 8, 9], nonfinite=[10, 11, 12, 13], clamped=[14])
    return np.array(v, F32), np.array(f, np.int32), kinds
