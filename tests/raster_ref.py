"""numpy restatement of the mesh rasteriser's contract (include/nerfpp_hip.h, nrf_raster_mesh): one numpy fp32 operation per source operation of the kernels and the
same int64 edge functions, so the GPU output is compared with this bit for bit.  Every face is evaluated on the whole image (a pixel inside a face lies inside its
bounding box, so this is the scan the header describes without its bookkeeping).  Also the meshes the host and GPU tests share.  Imports nothing of the package."""
import numpy as np

F32 = np.float32
SUBPIXEL = 256
GUARD = 16384
MAX_ATTR = 8
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
FACE_CHUNK = 128


def project(verts, K, c2w, near_z):
    """Steps 1-3 per vertex -> (X, Y int64, zd f32, ok bool); X = Y = 0 where not ok."""
    P = np.asarray(verts, F32).reshape(-1, 3)
    K = np.asarray(K, F32).reshape(3, 3)
    c2w = np.asarray(c2w, F32)[:3, :4]
    fx, cx, fy, cy = K[0, 0], K[0, 2], K[1, 1], K[1, 2]
    R, t = c2w[:, :3], c2w[:, 3]
    with np.errstate(all="ignore"):
        qx, qy, qz = P[:, 0] - t[0], P[:, 1] - t[1], P[:, 2] - t[2]
        xc = (R[0, 0] * qx + R[1, 0] * qy) + R[2, 0] * qz
        yc = (R[0, 1] * qx + R[1, 1] * qy) + R[2, 1] * qz
        zc = (R[0, 2] * qx + R[1, 2] * qy) + R[2, 2] * qz
        zd = -zc
        u = fx * (xc / zd) + cx
        v = cy - fy * (yc / zd)
        ok = (zd > F32(near_z)) & (np.abs(u) <= F32(GUARD)) & (np.abs(v) <= F32(GUARD))
        X = np.rint(np.where(ok, u, F32(0)) * F32(SUBPIXEL)).astype(np.int64)
        Y = np.rint(np.where(ok, v, F32(0)) * F32(SUBPIXEL)).astype(np.int64)
    assert zd.dtype == F32 and u.dtype == F32
    return X, Y, zd.astype(F32), ok


def classify(faces, n_verts, X, Y, ok, cull):
    """-> (cls [F]: 0 drawn, 1 clipped, 2 degenerate or culled, 3 bad index; A [F] int64, 0 where cls is 1 or 3)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    bad = ((f < 0) | (f >= n_verts)).any(-1)
    g = np.where(bad[:, None], 0, f) if n_verts else np.zeros_like(f)
    if n_verts == 0:
        return np.full(len(f), 3, np.int64), np.zeros(len(f), np.int64)
    clipped = ~bad & ~ok[g].all(-1)
    A = (X[g[:, 1]] - X[g[:, 0]]) * (Y[g[:, 2]] - Y[g[:, 0]]) - (Y[g[:, 1]] - Y[g[:, 0]]) * (X[g[:, 2]] - X[g[:, 0]])
    A = np.where(bad | clipped, 0, A)
    skipped = ~bad & ~clipped & ((A == 0) | (bool(cull) & (A > 0)))
    return np.where(bad, 3, np.where(clipped, 1, np.where(skipped, 2, 0))), A


def _edges(x, y, px, py):
    """e_k [..] int64 at p = (px, py) of the corners x, y [3][..]: e0 = E_12, e1 = E_20, e2 = E_01"""
    def E(a, b):
        return (x[b] - x[a]) * (py - y[a]) - (y[b] - y[a]) * (px - x[a])
    return E(1, 2), E(2, 0), E(0, 1)


def _top_left(x, y, s):
    """per edge k (v1->v2, v2->v0, v0->v1): (dx, dy) = s * (b - a); dy < 0 or (dy == 0 and dx > 0)"""
    out = []
    for a, b in ((1, 2), (2, 0), (0, 1)):
        dx, dy = s * (x[b] - x[a]), s * (y[b] - y[a])
        out.append((dy < 0) | ((dy == 0) & (dx > 0)))
    return out


def _depth(se, sA, r):
    """Step 6 -> (b [3], p [3], S, depth), all f32"""
    with np.errstate(all="ignore"):
        b = [(se[k].astype(np.float64) / sA.astype(np.float64)).astype(F32) for k in range(3)]
        p = [b[k] * r[k] for k in range(3)]
        S = (p[0] + p[1]) + p[2]
        depth = F32(1) / S
    return b, p, S, depth


def bbox_pixels(verts, faces, h, w, K, c2w, near_z=1e-3):
    """[F] the pixel count of each face's clamped bounding box (0 for a face that is bad or clipped): what sends a face to the wide kernel"""
    X, Y, _, ok = project(verts, K, c2w, near_z)
    cls, _ = classify(faces, len(X), X, Y, ok, 0)
    f = np.where((cls == 1)[:, None] | (cls == 3)[:, None], 0, np.asarray(faces, np.int64).reshape(-1, 3))
    i0, i1 = np.maximum((X[f].min(-1) + 255) >> 8, 0), np.minimum(X[f].max(-1) >> 8, w - 1)
    j0, j1 = np.maximum((Y[f].min(-1) + 255) >> 8, 0), np.minimum(Y[f].max(-1) >> 8, h - 1)
    return np.where((cls == 1) | (cls == 3), 0, np.maximum(i1 - i0 + 1, 0) * np.maximum(j1 - j0 + 1, 0))


def rasterize(verts, faces, attr, h, w, K, c2w, near_z=1e-3, cull=0):
    """-> dict(depth [h,w] f32, face [h,w] i32, bary [h,w,3] f32, attr [h,w,C] f32 or None, stats [4] u32, count [h,w] i64: how many drawn faces cover the pixel)"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    X, Y, zd, ok = project(verts, K, c2w, near_z)
    cls, A = classify(faces, len(X), X, Y, ok, cull)
    stats = np.array([(cls == c).sum() for c in range(4)], np.uint32)
    py, px = np.mgrid[0:h, 0:w].astype(np.int64) * SUBPIXEL
    key = np.full((h, w), NO_KEY, np.uint64)
    count = np.zeros((h, w), np.int64)
    drawn = np.nonzero(cls == 0)[0]
    with np.errstate(all="ignore"):
        r_all = F32(1) / zd
    for c0 in range(0, len(drawn), FACE_CHUNK):
        idx = drawn[c0:c0 + FACE_CHUNK]
        f = faces[idx]
        x = [X[f[:, k]][:, None, None] for k in range(3)]
        y = [Y[f[:, k]][:, None, None] for k in range(3)]
        r = [r_all[f[:, k]][:, None, None] for k in range(3)]
        a = A[idx][:, None, None]
        s = np.sign(a)
        e = _edges(x, y, px[None], py[None])
        tl = _top_left(x, y, s)
        se = [s * e[k] for k in range(3)]
        inside = np.ones(se[0].shape, bool)
        for k in range(3):
            inside &= (se[k] > 0) | ((se[k] == 0) & tl[k])
        _, _, _, depth = _depth(se, s * a, r)
        k64 = (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)[:, None, None]
        key = np.minimum(key, np.where(inside, k64, NO_KEY).min(0))
        count += inside.sum(0)
    hit = key != NO_KEY
    face = np.where(hit, (key & np.uint64(0xFFFFFFFF)).astype(np.int64), 0)
    out_depth = np.where(hit, (key >> np.uint64(32)).astype(np.uint32), np.uint32(0)).view(F32)
    # resolve: the winner's b_k by the same expressions
    f = faces[face] if len(faces) else np.zeros((h, w, 3), np.int64)
    f = np.where(hit[..., None], f, 0)
    nv = len(X)
    if nv == 0:
        X, Y, r_all = np.zeros(1, np.int64), np.zeros(1, np.int64), np.ones(1, F32)
    x, y, r = [X[f[..., k]] for k in range(3)], [Y[f[..., k]] for k in range(3)], [r_all[f[..., k]] for k in range(3)]
    a = np.where(hit, A[face] if len(faces) else 0, 1)
    s = np.sign(a)
    e = _edges(x, y, px, py)
    b, p, S, _ = _depth([s * e[k] for k in range(3)], s * a, r)
    bary = np.where(hit[..., None], np.stack(b, -1), F32(0)).astype(F32)
    out_attr = None
    if attr is not None:
        at = np.asarray(attr, F32).reshape(nv, -1)
        with np.errstate(all="ignore"):
            a3 = [at[f[..., k]] for k in range(3)]
            val = ((p[0][..., None] * a3[0] + p[1][..., None] * a3[1]) + p[2][..., None] * a3[2]) / S[..., None]
        out_attr = np.where(hit[..., None], val, F32(0)).astype(F32)
    return dict(depth=out_depth, face=np.where(hit, face, -1).astype(np.int32), bary=bary, attr=out_attr, stats=stats, count=count)


# ---- the meshes of the tests ----
def lattice_mesh(spacing, n=9, z=-2.0, x0=-0.5, y0=0.25, seed=0):
    """n x n vertices on the plane z, x = x0 + spacing * i, y = y0 - spacing * j (v grows with j); two faces per cell, diagonals alternating, each face's winding
    flipped at random -> (verts [n*n, 3] f32, faces [2 (n-1)^2, 3] i32)"""
    j, i = np.mgrid[0:n, 0:n]
    verts = np.stack([x0 + spacing * i, y0 - spacing * j, np.full(i.shape, z)], -1).reshape(-1, 3).astype(F32)
    rng = np.random.default_rng(seed)
    faces = []
    for cj in range(n - 1):
        for ci in range(n - 1):
            a, b, c, d = cj * n + ci, cj * n + ci + 1, (cj + 1) * n + ci + 1, (cj + 1) * n + ci
            for t in (((a, b, c), (a, c, d)) if (ci + cj) % 2 == 0 else ((a, b, d), (b, c, d))):
                faces.append(t[::-1] if rng.integers(2) else t)
    return verts, np.array(faces, np.int32)


LATTICE_K = np.array([[8, 0, 3], [0, 8, 2], [0, 0, 1]], F32)
LATTICE_POSE = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], F32)
LATTICE_H, LATTICE_W = 12, 14


def octa_sphere(centre, radius, levels=3):
    """An octahedron subdivided `levels` times onto the sphere: (verts [V, 3] f32, faces [F, 3] i32), counter-clockwise seen from outside; 258 / 512 at 3 levels"""
    v = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    v = [np.array(p, np.float64) for p in v]
    for _ in range(levels):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        f = nf
    verts = (np.asarray(centre, np.float64) + radius * np.array(v)).astype(F32)
    return verts, np.array(f, np.int32)


def face_plane_distances(verts, faces, centre):
    """float64 distance of every face's plane from centre"""
    p = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return np.abs(((p[:, 0] - np.asarray(centre, np.float64)) * n).sum(-1))
