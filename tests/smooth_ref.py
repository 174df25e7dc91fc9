"""The definition of nrf_mesh_adjacency_count / _emit, nrf_mesh_smooth and nrf_mesh_vertex_normals (include/nerfpp_hip.h, "Mesh adjacency, smoothing and vertex
normals") restated in numpy.  Integers decide the adjacency; every float32 operation is one numpy float32 operation, and every sequential sum is np.add applied
position by position along the rows (never np.sum), so the GPU tests compare bit for bit."""
import numpy as np

import raster_ref as R

F32 = np.float32
ADJ_BOUNDARY, ADJ_NONMANIFOLD, ADJ_SHORT_ROW = 1, 2, 32
SMOOTH_MAX_CHANNELS = 4
SMOOTH_FREE, SMOOTH_FIXED, SMOOTH_CURVE = 0, 1, 2
NORMALS_AREA, NORMALS_UNIT = 0, 1
STATS = ("bad_index", "repeated_corner", "used_vertices", "edges", "boundary_edges", "nonmanifold_edges", "longest_face_row", "longest_nbr_row")


def _starts(owner, n):
    return np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=n))]).astype(np.int64)


def adjacency(faces, n_verts):
    """dict(face_start [V+1] i64, face_list i32, nbr_start [V+1] i64, nbr i32, nbr_faces i32, flags [V] u8, stats [8] i64, valid [F] bool)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    v = int(n_verts)
    bad = ((f < 0) | (f >= v)).any(axis=1)
    rep = ~bad & ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2]))
    valid = ~bad & ~rep
    ids = np.nonzero(valid)[0]
    g = f[ids]
    corner, face = g.reshape(-1), np.repeat(ids, 3)
    order = np.lexsort((face, corner))          # by vertex, then ascending face index
    face_list = face[order].astype(np.int32)
    face_start = _starts(corner, v)
    a = np.concatenate([g[:, 0], g[:, 0], g[:, 1], g[:, 1], g[:, 2], g[:, 2]])
    b = np.concatenate([g[:, 1], g[:, 2], g[:, 0], g[:, 2], g[:, 0], g[:, 1]])
    key, count = np.unique(a * max(v, 1) + b, return_counts=True)          # ascending (vertex, neighbour)
    own, nbr = key // max(v, 1), key % max(v, 1)
    nbr_start = _starts(own, v)
    flags = np.zeros(v, np.uint8)
    flags[own[count == 1]] |= ADJ_BOUNDARY
    flags[own[count > 2]] |= ADJ_NONMANIFOLD
    low = own < nbr
    stats = np.array([bad.sum(), rep.sum(), (np.diff(face_start) > 0).sum(), low.sum(), (low & (count == 1)).sum(), (low & (count > 2)).sum(),
                      np.diff(face_start).max(initial=0), np.diff(nbr_start).max(initial=0)], np.int64)
    return dict(face_start=face_start, face_list=face_list, nbr_start=nbr_start, nbr=nbr.astype(np.int32), nbr_faces=count.astype(np.int32), flags=flags, stats=stats,
                valid=valid, n_verts=v)


def topology(adj):
    s = dict(zip(STATS, (int(x) for x in adj["stats"])))
    faces_valid = int(adj["face_start"][-1]) // 3
    return dict(vertices_used=s["used_vertices"], edges=s["edges"], faces_valid=faces_valid, boundary_edges=s["boundary_edges"],
                nonmanifold_edges=s["nonmanifold_edges"], euler=s["used_vertices"] - s["edges"] + faces_valid, closed=s["boundary_edges"] == 0,
                manifold=s["nonmanifold_edges"] == 0)


def _row_sums(owner, values, n):
    """(S [n, C], count [n]): per owner the values of its entries added sequentially in their stored order, the first one starting the sum; zeros and 0 without one.
    `owner` ascends."""
    count = np.bincount(owner, minlength=n)
    first = np.concatenate([[0], np.cumsum(count)])[:-1]
    pos = np.arange(len(owner)) - first[owner]
    s = np.zeros((n,) + values.shape[1:], F32)
    by_pos = np.argsort(pos, kind="stable")
    cut = np.concatenate([[0], np.cumsum(np.bincount(pos, minlength=1))])
    with np.errstate(all="ignore"):
        for p in range(len(cut) - 1):
            e = by_pos[cut[p]:cut[p + 1]]          # every owner at most once
            s[owner[e]] = values[e] if p == 0 else np.add(s[owner[e]], values[e])
    return s, count


def smooth_step(x, adj, factor, boundary):
    x = np.asarray(x, F32)
    n = adj["n_verts"]
    own = np.repeat(np.arange(n), np.diff(adj["nbr_start"]))
    on_boundary = (adj["flags"] & ADJ_BOUNDARY) != 0
    keep = np.ones(len(own), bool)
    if boundary == SMOOTH_CURVE:
        keep = ~on_boundary[own] | (adj["nbr_faces"] == 1)
    s, count = _row_sums(own[keep], x[adj["nbr"][keep]], n)
    moves = count > 0
    if boundary == SMOOTH_FIXED:
        moves &= ~on_boundary
    out = x.copy()
    with np.errstate(all="ignore"):
        m = s[moves] / count[moves].astype(F32)[:, None]
        d = m - x[moves]
        out[moves] = x[moves] + F32(factor) * d
    return out


def smooth(x, adj, iterations, lam, mu, boundary):
    x = np.asarray(x, F32)
    flat = x.ndim == 1
    y = x.reshape(len(x), -1).copy()
    for _ in range(iterations):
        y = smooth_step(y, adj, lam, boundary)
        if F32(mu) != 0:
            y = smooth_step(y, adj, mu, boundary)
    return y.reshape(-1) if flat else y


def vertex_normals(verts, faces, adj, weighting=NORMALS_AREA):
    verts = np.asarray(verts, F32)
    n = adj["n_verts"]
    fl = adj["face_list"].astype(np.int64)
    own = np.repeat(np.arange(n), np.diff(adj["face_start"]))
    f = np.asarray(faces, np.int64).reshape(-1, 3)[fl]
    with np.errstate(all="ignore"):
        a, b, c = verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]]
        e1, e2 = b - a, c - a
        nrm = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        if weighting == NORMALS_UNIT:
            l = np.sqrt((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2])
            nrm = np.where((l == 0)[:, None], F32(0), nrm / l[:, None]).astype(F32)
        s, _ = _row_sums(own, nrm, n)
        ln = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        return np.where((ln == 0)[:, None], F32(0), s / ln[:, None]).astype(F32)


# ---- the meshes the tests share ----

CENTRE, RADIUS = (0.05, -0.1, 0.15), 0.7


def sphere(level, centre=CENTRE, radius=RADIUS):
    return R.octa_sphere(centre, radius, level)


def hemisphere(level, centre=CENTRE, radius=RADIUS):
    """The faces of the sphere whose centroid lies above the centre; the vertices stay, so the lower ones are unused"""
    verts, faces = sphere(level, centre, radius)
    up = verts[faces.astype(np.int64)].astype(np.float64).mean(axis=1)[:, 2] > centre[2]
    return verts, np.ascontiguousarray(faces[up])


def fan(n, seed=3):
    """n faces around vertex 0: rim vertices 1 .. n + 1 on a slightly bumpy circle, face k = (0, 1 + k, 2 + k): an open fan, vertex 0 has n faces and n + 1 neighbours"""
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 1.9 * np.pi, n + 1)
    rim = np.stack([np.cos(t), np.sin(t), 0.1 * rng.standard_normal(n + 1)], axis=1)
    verts = np.concatenate([[[0.0, 0.0, 0.3]], rim]).astype(F32)
    k = np.arange(n)
    return verts, np.stack([np.zeros(n, np.int64), 1 + k, 2 + k], axis=1).astype(np.int32)


def dirty():
    """10 vertices (vertex 9 unused, vertex 5 NaN): corners of -1 and of V, repeated corners, a duplicated face, three faces on the edge (0, 1)"""
    verts = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -1, 0.2], [0.5, 0.3, 1], [2, 1, 0], [2, -1, 0.5], [3, 0, 0.25], [1.5, 2, 1], [9, 9, 9]], F32)
    verts[5] = np.nan
    faces = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4],          # three faces on (0, 1)
                      [1, 5, 2], [1, 6, 5], [5, 6, 7], [5, 6, 7],          # a duplicated face
                      [0, -1, 2], [3, 10, 1], [2, 2, 8], [4, 8, 4], [7, 7, 7], [-1, 3, 3],          # bad, bad, repeated, repeated, repeated, bad (and repeated)
                      [2, 5, 8]], np.int32)
    return verts, faces


def permuted(faces, seed):
    """The same faces in another order, every face with one of the 6 orders of its corners (3 keep the winding, 3 flip it)"""
    rng = np.random.default_rng(seed)
    orders = np.array([[0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1], [2, 1, 0], [1, 0, 2]])
    f = np.asarray(faces)[rng.permutation(len(faces))]
    pick = orders[rng.integers(0, 6, len(f))]
    return np.ascontiguousarray(np.take_along_axis(f, pick, axis=1))
