"""numpy restatement of the mesh simplification contract (include/nerfpp_hip.h: nrf_mesh_simplify_count / _emit): one numpy fp32 operation per source-level
operation, integers for everything else, np.unique for the coincident faces.  tests/test_simplify_host.py pins it on subdivided spheres; the GPU tests compare the
library with it bit for bit."""
import numpy as np

F32 = np.float32
SIMPLIFY_MAX_DIM, SIMPLIFY_MAX_CELLS = 1024, 1 << 27
POS_MEAN, POS_MEMBER = 0, 1
FIXED = F32(1048576.0)          # 2^20 steps per cell
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def grid(bbox, dims):
    """(bmin [3], inv_h [3], h [3]) f32: inv_h = (float)n / (bmax - bmin), h = 1.0f / inv_h"""
    b = np.asarray(bbox, F32).reshape(6)
    n = np.asarray(dims, np.int64).reshape(3)
    inv_h = n.astype(F32) / (b[3:] - b[:3])
    return b[:3].copy(), inv_h, F32(1.0) / inv_h


def vertex_cells(verts, bbox, dims):
    """Step 1 -> (cell [V] int64, -1 for a vertex without one; t [V, 3] f32; c [V, 3] int64)"""
    v = np.asarray(verts, F32).reshape(-1, 3)
    n = np.asarray(dims, np.int64).reshape(3)
    bmin, inv_h, _ = grid(bbox, dims)
    finite = np.isfinite(v).all(axis=1)
    with np.errstate(all="ignore"):
        t = (np.where(finite[:, None], v, F32(0)) - bmin) * inv_h
        c = np.clip(np.floor(t), F32(0), (n - 1).astype(F32)).astype(np.int64)
    cell = c[:, 0] + n[0] * (c[:, 1] + n[1] * c[:, 2])
    cell[~finite] = -1
    return cell, t, c


def classify(faces, cell):
    """Step 2 -> (cls [F]: 0 candidate, 1 bad, 2 non-finite, 3 collapsed; tri [F, 3] int64 the cells of the corners (-1 rows for bad faces); used [V] bool)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    nv = len(cell)
    bad = ((f < 0) | (f >= nv)).any(axis=1)
    tri = np.full(f.shape, -1, np.int64)
    tri[~bad] = cell[f[~bad]]
    nonfinite = ~bad & (tri < 0).any(axis=1)
    collapsed = ~bad & ~nonfinite & ((tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 0] == tri[:, 2]))
    cls = np.zeros(len(f), np.int64)
    cls[bad], cls[nonfinite], cls[collapsed] = 1, 2, 3
    used = np.zeros(nv, bool)
    used[f[~bad & ~nonfinite].reshape(-1)] = True
    return cls, tri, used


def coincident(cls, tri):
    """Step 3 -> keep [F] bool: per sorted triple the even or odd candidate of lowest index the net orientation names, none where it is zero"""
    cand = np.nonzero(cls == 0)[0]
    keep = np.zeros(len(cls), bool)
    if len(cand) == 0:
        return keep
    t = tri[cand]
    s = np.sort(t, axis=1)
    even = np.zeros(len(cand), bool)
    for r in range(3):
        even |= (t == np.roll(s, -r, axis=1)).all(axis=1)
    _, group = np.unique(s, axis=0, return_inverse=True)
    group = group.reshape(-1)
    k = int(group.max()) + 1
    net = np.bincount(group, weights=np.where(even, 1, -1), minlength=k).astype(np.int64)
    big = np.iinfo(np.int64).max
    low = np.full((2, k), big, np.int64)          # [0] the lowest odd face, [1] the lowest even face
    np.minimum.at(low[1], group[even], cand[even])
    np.minimum.at(low[0], group[~even], cand[~even])
    winner = np.where(net > 0, low[1], np.where(net < 0, low[0], big))
    keep[winner[winner != big]] = True
    return keep


def simplify(verts, faces, bbox, dims, position=POS_MEAN):
    """Steps 1-6 -> dict(n_verts, n_faces, stats [4] uint32 {bad, non-finite, collapsed, removed}, verts [n_verts, 3] f32, faces [n_faces, 3] int32, rep [n_verts]
    int32, face_src [n_faces] int32, cluster [V] int32, cells [n_verts] int64 the cell of every output vertex, mean [n_verts, 3] f32 the P of step 5)"""
    v = np.asarray(verts, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    n = np.asarray(dims, np.int64).reshape(3)
    cell, t, c = vertex_cells(v, bbox, dims)
    cls, tri, used = classify(f, cell)
    keep = coincident(cls, tri)
    stats = np.array([(cls == 1).sum(), (cls == 2).sum(), (cls == 3).sum(), ((cls == 0) & ~keep).sum()], np.uint32)
    face_src = np.nonzero(keep)[0]
    out_cells = np.unique(tri[keep])          # ascending cell index
    cluster = np.full(len(v), -1, np.int64)
    has = cell >= 0
    at = np.searchsorted(out_cells, cell[has])
    hit = (at < len(out_cells)) & (out_cells[np.minimum(at, max(len(out_cells) - 1, 0))] == cell[has]) if len(out_cells) else np.zeros(has.sum(), bool)
    cluster[np.nonzero(has)[0][hit]] = at[hit]
    out_faces = np.searchsorted(out_cells, tri[keep]).astype(np.int32).reshape(-1, 3)
    # step 5: the fixed-point mean of the members, the USED vertices of the cell
    k = len(out_cells)
    member = np.nonzero(used & (cluster >= 0))[0]
    o = cluster[member]
    with np.errstate(all="ignore"):
        frac = np.clip(t[member] - c[member].astype(F32), F32(0), F32(1))
        q = (frac * FIXED).astype(np.int64)
    S = np.zeros((k, 3), np.int64)
    np.add.at(S, o, q)
    m = np.bincount(o, minlength=k).astype(np.int64)
    oc = np.stack([out_cells % n[0], (out_cells // n[0]) % n[1], out_cells // (n[0] * n[1])], axis=1)
    bmin, _, h = grid(bbox, dims)
    tm = (oc.astype(np.float64) + (S.astype(np.float64) / m.astype(np.float64)[:, None]) * 2.0 ** -20).astype(F32)
    P = bmin + tm * h
    # step 6: the member nearest the mean, lowest index on a tie
    with np.errstate(all="ignore"):
        d = v[member] - P[o]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    key = np.full(k, NO_KEY, np.uint64)
    np.minimum.at(key, o, (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | member.astype(np.uint64))
    rep = (key & np.uint64(0xFFFFFFFF)).astype(np.int64)
    if position == POS_MEAN:
        out_verts = P
    elif position == POS_MEMBER:
        out_verts = v[rep]
    else:
        raise ValueError(f"position {position}")
    return dict(n_verts=k, n_faces=int(keep.sum()), stats=stats, verts=np.ascontiguousarray(out_verts, F32).reshape(-1, 3), faces=out_faces, rep=rep.astype(np.int32),
                face_src=face_src.astype(np.int32), cluster=cluster.astype(np.int32), cells=out_cells, mean=P.reshape(-1, 3))


def mesh_box(verts):
    """[6] f32: the box of the finite vertices"""
    v = np.asarray(verts, F32).reshape(-1, 3)
    v = v[np.isfinite(v).all(axis=1)]
    return np.concatenate([v.min(axis=0), v.max(axis=0)]).astype(F32)


def edge_use(faces):
    """(edges [E, 2] sorted pairs, count [E]) of the undirected edges of a triangle list"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    return np.unique(e, axis=0, return_counts=True)
