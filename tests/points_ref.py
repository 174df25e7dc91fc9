"""numpy restatement of the point-cloud contract (include/nerfpp_hip.h "Point clouds"): the point BVH as bvh_ref's tree over the faces (i, i, i), the k nearest
neighbours as the k smallest packed keys of a brute-force pass over all pairs, the same search restated over the tree with the header's skip rule (and the census of
that rule), normals and eigenvalues by the header's fp64 steps with the Jacobi iteration of align_ref, the scores, the value statistics and the plane sums from
given normals.  One numpy operation per source operation.  Also the clouds the host and GPU tests share.  Imports nothing of the package."""
import functools

import numpy as np

import align_ref as A
import bvh_ref as B
import geometry_ref as G
import ordered_sum_ref as OS

F32, F64 = np.float32, np.float64
MAGIC = 0x4e52465042563031          # "NRFPBV01"
KNN_MAX_K = 32
JACOBI_SWEEPS = 6
BIG_THETA = 1e150
NONE = (G.INF_BITS << np.uint64(32)) | np.uint64(0xFFFFFFFF)
STATS_TILE = 4096
JPAIRS = [(0, 1), (0, 2), (1, 2)]


# ---- the clouds ----
def faces_iii(n):
    return np.repeat(np.arange(n, dtype=np.int32)[:, None], 3, axis=1)


def lattice(m=6):
    g = np.arange(m, dtype=F32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(F32)


@functools.lru_cache(maxsize=None)
def clouds():
    """name -> points [n, 3] f32: sizes around the block, the icosphere's vertices, copies of one point, a flat cloud, an integer lattice (exact ties), and
    non-finite points mixed in and alone"""
    out = {}
    for n in (0, 1, 2, 3, 255, 256, 257):
        out[f"rand{n}"] = np.random.default_rng(100 + n).uniform(-1, 1, (n, 3)).astype(F32)
    v, _ = A.ico_sphere(3)
    out["ico642"] = (np.asarray(v, F32) * F32(0.7) + np.array([0.1, -0.15, 0.2], F32)).astype(F32)
    out["copies300"] = np.repeat(np.array([[0.3, -0.2, 0.9]], F32), 300, axis=0)
    flat = np.random.default_rng(7).uniform(-1, 1, (200, 3)).astype(F32)
    flat[:, 2] = F32(0.25)
    out["flat"] = flat
    out["lattice"] = lattice(6)
    mixed = np.random.default_rng(8).uniform(-1, 1, (120, 3)).astype(F32)
    mixed[5, 0], mixed[17, 1], mixed[40, 2], mixed[99] = np.nan, np.inf, -np.inf, (np.nan, np.nan, np.nan)
    out["mixed"] = mixed
    out["nonfinite_only"] = np.array([[np.nan, 0, 0], [0, np.inf, 0], [1, 2, -np.inf]], F32)
    for v in out.values():
        v.setflags(write=False)
    return out


def build(points):
    """The tree of a cloud: bvh_ref's over verts = points, faces = (i, i, i)"""
    points = np.asarray(points, F32).reshape(-1, 3)
    return B.build(points, faces_iii(len(points)))


def queries(points, seed=0, n=257):
    """n queries of every kind around a cloud: its own points, points near it, uniform ones, ones 10 and 1 000 box diagonals away, non-finite rows"""
    points = np.asarray(points, F32).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    fin = points[np.isfinite(points).all(-1)]
    lo, hi = (fin.min(0), fin.max(0)) if len(fin) else (np.zeros(3, F32), np.ones(3, F32))
    diag = max(float(np.linalg.norm(hi.astype(F64) - lo.astype(F64))), 1.0)
    q = rng.uniform(lo - 0.3, hi + 0.3, (n, 3)).astype(F32)
    if len(fin):
        m = n // 3
        q[:m] = fin[rng.integers(0, len(fin), m)]
        q[m:2 * m] = fin[rng.integers(0, len(fin), m)] + rng.normal(0, 0.05, (m, 3)).astype(F32)
    d = rng.normal(size=(4, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    c = (lo.astype(F64) + hi.astype(F64)) / 2
    q[-8:-6] = (c + 10 * diag * d[:2]).astype(F32)
    q[-6:-4] = (c + 1000 * diag * d[2:]).astype(F32)
    q[-4] = (np.nan, 0, 0)
    q[-3] = (0, np.inf, 0)
    q[-2] = (0, 0, -np.inf)
    return q[:n]


# ---- k nearest: all pairs ----
def pair_keys(query, target, max_dist=np.inf, exclude_self=False):
    """-> keys [nq, n] uint64, NONE where the pair is no candidate"""
    q, t = np.asarray(query, F32).reshape(-1, 3), np.asarray(target, F32).reshape(-1, 3)
    qf, tf = np.isfinite(q).all(-1), np.isfinite(t).all(-1)
    with np.errstate(all="ignore"):
        md2 = F32(max_dist) * F32(max_dist)
        dx, dy, dz = q[:, None, 0] - t[None, :, 0], q[:, None, 1] - t[None, :, 1], q[:, None, 2] - t[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == F32
    key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(len(t), dtype=np.uint64)[None]
    ok = tf[None] & qf[:, None] & (d2 <= md2)
    if exclude_self:
        ok &= np.arange(len(q))[:, None] != np.arange(len(t))[None]
    return np.where(ok, key, NONE)


def unpack(keys):
    keys = np.asarray(keys, np.uint64)
    return (keys >> np.uint64(32)).astype(np.uint32).view(F32), (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)


def knn(query, target, k, max_dist=np.inf, exclude_self=False):
    """-> dict(d2 [nq, k] f32, index [nq, k] i32, count [nq] i32, keys [nq, k] u64, stats0: non-finite queries)"""
    q = np.asarray(query, F32).reshape(-1, 3)
    keys = pair_keys(q, target, max_dist, exclude_self)
    keys = np.concatenate([keys, np.full((len(q), k), NONE, np.uint64)], 1)
    best = np.sort(keys, axis=1)[:, :k]
    d2, idx = unpack(best)
    return dict(d2=d2, index=idx, count=(best != NONE).sum(1).astype(np.int32), keys=best, stats0=int((~np.isfinite(q).all(-1)).sum()))


# ---- k nearest over the tree, the header's traversal ----
def knn_tree(tree, points, q, k, max_dist=np.inf, self_index=-1):
    """One finite query q [3] through the restated tree -> (keys [k] u64 ascending, nodes visited).  The list is a sorted Python list; the skip rule is the header's"""
    points = np.asarray(points, F32).reshape(-1, 3)
    q = np.asarray(q, F32).reshape(1, 3)
    with np.errstate(all="ignore"):
        md2 = F32(max_dist) * F32(max_dist)
    held = []

    def kth():
        return F32(np.inf) if len(held) < k else unpack(np.uint64(held[-1]))[0]

    def take(pos, d2):
        j = int(tree["leaf_face"][pos])
        if j == self_index or not d2 <= md2:
            return
        key = (int(np.asarray(d2, F32).view(np.uint32)) << 32) | j
        if len(held) < k or key < held[-1]:
            held.append(key)
            held.sort()
            del held[k:]

    nv = tree["n_valid"]
    visited = 0
    if nv == 1:
        j = tree["leaf_face"][0]
        take(0, pair_d2(q[0], points[j]))
    elif nv > 1:
        stack, at = [], 0
        while True:
            visited += 1
            box = tree["box"][at]
            b = [B.box_d2(q, box[0:3], box[3:6])[0], B.box_d2(q, box[6:9], box[9:12])[0]]
            ch = [int(tree["child"][at, 0]), int(tree["child"][at, 1])]
            if b[1] < b[0]:
                b, ch = b[::-1], ch[::-1]
            nxt = -1
            for which in range(2):
                if b[which] > min(kth(), md2):
                    continue
                if ch[which] < 0:
                    take(-(ch[which] + 1), b[which])          # a leaf's bound is its d2
                elif nxt < 0:
                    nxt = ch[which]
                else:
                    stack.append(ch[which])
            if nxt < 0:
                if not stack:
                    break
                nxt = stack.pop()
            at = nxt
    out = np.full(k, NONE, np.uint64)
    out[:len(held)] = np.array(held, np.uint64)
    return out, visited


def pair_d2(q, p):
    q, p = np.asarray(q, F32), np.asarray(p, F32)
    with np.errstate(all="ignore"):
        dx, dy, dz = q[0] - p[0], q[1] - p[1], q[2] - p[2]
        return (dx * dx + dy * dy) + dz * dz


def pruning_violations(tree, points, query):
    """Over every (finite query, node, child box, point under it): how often the bound exceeds d2; and over every leaf child, how often bound != d2 as bits"""
    points = np.asarray(points, F32).reshape(-1, 3)
    q = np.asarray(query, F32).reshape(-1, 3)
    q = q[np.isfinite(q).all(-1)]
    above = unequal = triples = 0
    for i in range(len(tree["child"])):
        for c in range(2):
            ch = int(tree["child"][i, c])
            l, r = (-(ch + 1), -(ch + 1)) if ch < 0 else tree["range"][ch]
            b2 = B.box_d2(q, tree["box"][i, 6 * c:6 * c + 3], tree["box"][i, 6 * c + 3:6 * c + 6])
            under = points[tree["leaf_face"][l:r + 1]]
            with np.errstate(all="ignore"):
                dx, dy, dz = q[:, None, 0] - under[None, :, 0], q[:, None, 1] - under[None, :, 1], q[:, None, 2] - under[None, :, 2]
                d2 = (dx * dx + dy * dy) + dz * dz
            above += int((b2[:, None] > d2).sum())
            triples += d2.size
            if ch < 0:
                unequal += int((b2.view(np.uint32) != d2[:, 0].view(np.uint32)).sum())
    return above, unequal, triples


# ---- normals ----
def _jacobi3(a, census=None):
    """a: dict (r, c) -> [n] float64 arrays of the symmetric 3x3 (all nine entries) -> (diagonal [3][n], V [3][3][n]).  align_ref's rotation, vectorised: a skipped
    pair keeps every entry"""
    n = len(a[0, 0])
    V = {(r, c): np.full(n, 1.0 if r == c else 0.0) for r in range(3) for c in range(3)}
    with np.errstate(all="ignore"):
        for _ in range(JACOBI_SWEEPS):
            for p, q in JPAIRS:
                apq = a[p, q]
                skip = apq == 0.0
                th = (a[q, q] - a[p, p]) / (2.0 * apq)
                ath = np.abs(th)
                t = np.where(ath > BIG_THETA, 0.5 / th, np.where(th >= 0.0, 1.0, -1.0) / (ath + np.sqrt(th * th + 1.0)))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                new = dict(a)
                for k in range(3):
                    akp, akq = new[k, p], new[k, q]
                    new[k, p], new[k, q] = c * akp - s * akq, s * akp + c * akq
                for k in range(3):
                    apk, aqk = new[p, k], new[q, k]
                    new[p, k], new[q, k] = c * apk - s * aqk, s * apk + c * aqk
                nv = dict(V)
                for k in range(3):
                    vkp, vkq = V[k, p], V[k, q]
                    nv[k, p], nv[k, q] = c * vkp - s * vkq, s * vkp + c * vkq
                a = {key: np.where(skip, a[key], new[key]) for key in a}
                V = {key: np.where(skip, V[key], nv[key]) for key in V}
            if census is not None:
                off = np.maximum(np.maximum(np.abs(a[0, 1]), np.abs(a[0, 2])), np.abs(a[1, 2]))
                dia = np.maximum(np.maximum(np.abs(a[0, 0]), np.abs(a[1, 1])), np.abs(a[2, 2]))
                census.append((off, dia))
    return [a[0, 0], a[1, 1], a[2, 2]], V


def normals(points, index, toward=None, toward_stride=0, census=None):
    """-> dict(normals [n, 3] f32, eigen [n, 3] f32, valid [n] bool, stats0: degenerate sets).  census: a list that receives per sweep (largest |off-diagonal|,
    largest |diagonal|) [n] of every set that reached the iteration"""
    p32 = np.asarray(points, F32).reshape(-1, 3)
    index = np.asarray(index, np.int32).reshape(len(p32), -1)
    n, k = index.shape
    p = p32.astype(F64)
    filled = (index >= 0) & (index < n)
    at = np.where(filled, index, 0)
    m = 1 + filled.sum(1)
    fin = np.isfinite(p32).all(-1)
    total = p.copy()
    with np.errstate(all="ignore"):
        for s in range(k):
            x = p[at[:, s]]
            fin = fin & (~filled[:, s] | np.isfinite(p32[at[:, s]]).all(-1))
            total = np.where(filled[:, s, None], total + x, total)
        mean = total / m[:, None].astype(F64)
        d = p - mean
        c = {(r, cc): d[:, r] * d[:, cc] for r in range(3) for cc in range(r, 3)}
        for s in range(k):
            d = p[at[:, s]] - mean
            for key in c:
                c[key] = np.where(filled[:, s], c[key] + d[:, key[0]] * d[:, key[1]], c[key])
        a = {(r, cc): c[min(r, cc), max(r, cc)] for r in range(3) for cc in range(3)}
        ok = fin & (m >= 3)
        sub = []
        ev, V = _jacobi3(a, sub if census is not None else None)
        if census is not None:
            census.extend((off[ok], dia[ok]) for off, dia in sub)
        ev = np.stack(ev, -1)                                  # [n, 3]
        order = np.argsort(ev, axis=1, kind="stable")         # ascending, the lowest column first on a tie
        order = np.where(np.isnan(ev).any(-1, keepdims=True), np.arange(3)[None], order)
        lam = np.take_along_axis(ev, order, 1)
        Vm = np.stack([np.stack([V[r, cc] for cc in range(3)], -1) for r in range(3)], 1)          # [n, row, column]
        col = np.take_along_axis(Vm, order[:, None, :1].repeat(3, 1), 2)[:, :, 0]                  # [n, 3]
        nrm = np.sqrt((col[:, 0] * col[:, 0] + col[:, 1] * col[:, 1]) + col[:, 2] * col[:, 2])
        ok = ok & np.isfinite(lam).all(-1) & (lam[:, 1] > 0.0) & (nrm > 0.0) & np.isfinite(nrm)
        nn = col / nrm[:, None]
        if toward is not None:
            tw = np.asarray(toward, F32).astype(F64)
            tw = tw.reshape(n, 3) if toward_stride else np.broadcast_to(tw.reshape(1, 3), (n, 3))
            w = tw - p
            flip = ((nn[:, 0] * w[:, 0] + nn[:, 1] * w[:, 1]) + nn[:, 2] * w[:, 2]) < 0.0
        else:
            big = np.zeros(n, np.int64)
            mag = np.abs(nn)
            big = np.where(mag[:, 1] > mag[:, 0], 1, big)
            big = np.where(mag[:, 2] > np.take_along_axis(mag, big[:, None], 1)[:, 0], 2, big)
            flip = np.take_along_axis(nn, big[:, None], 1)[:, 0] < 0.0
        nn = np.where(flip[:, None], -nn, nn)
        out_n = np.where(ok[:, None], nn, 0.0).astype(F32)
        out_e = np.where(ok[:, None], lam, 0.0).astype(F32)
    return dict(normals=out_n, eigen=out_e, valid=ok, stats0=int((~ok).sum()))


# ---- scores and statistics ----
def mean_distance(d2):
    d2 = np.asarray(d2, F32)
    d2 = d2.reshape(len(d2), -1)
    filled = d2 < np.inf
    total = np.zeros(len(d2), F32)
    with np.errstate(all="ignore"):
        for s in range(d2.shape[1]):
            total = np.where(filled[:, s], total + np.sqrt(np.where(filled[:, s], d2[:, s], F32(0))), total)
        cnt = filled.sum(1)
        out = np.where(cnt > 0, total / np.maximum(cnt, 1).astype(F32), F32(np.inf))
    assert total.dtype == F32 and out.dtype == F32
    return out


def value_stats(values):
    """-> [4] float64: count, sum, sum of squares, max(0, largest) over the finite entries, in nrf_distance_stats's order"""
    v = np.asarray(values, F32).reshape(-1)
    nb = max(1, -(-len(v) // STATS_TILE))
    pad = np.full(nb * STATS_TILE, np.inf, F32)
    pad[:len(v)] = v
    fin = np.isfinite(pad)
    x = np.where(fin, pad, F32(0)).astype(F64)
    out = []
    for c in (fin.astype(F64), x, x * x):
        c = c.reshape(nb, STATS_TILE // 256, 256)
        lanes = np.zeros((nb, 256))
        for i in range(STATS_TILE // 256):
            lanes = lanes + c[:, i]
        out.append(float(OS.finish(OS.block_sums(lanes))))
    out.append(max(0.0, float(x[fin].max())) if fin.any() else 0.0)
    return np.array(out, F64)


def outlier_threshold(scores, ratio):
    """mean + ratio * std as StatisticalOutliers forms it, in float64 from value_stats"""
    st = value_stats(scores)
    cnt = max(st[0], 1.0)
    mean = st[1] / cnt
    return mean + F64(ratio) * np.sqrt(max(st[2] / cnt - mean * mean, 0.0))


# ---- the plane sums from given normals ----
def terms_normals(y, p, nrm, index):
    """-> (terms [n, 37] float64, zero rows where the pair is dropped; stats [4] u32)"""
    y32, p32, n32 = (np.asarray(v, F32).reshape(-1, 3) for v in (y, p, nrm))
    index = np.asarray(index, np.int32).reshape(-1)
    n = len(index)
    none = index < 0
    nonfinite = ~none & ~(np.isfinite(y32).all(-1) & np.isfinite(p32).all(-1))
    keep = ~none & ~nonfinite
    yy, pp, c = ([v[:, k].astype(F64) for k in range(3)] for v in (y32, p32, n32))
    one = np.ones(n)
    with np.errstate(all="ignore"):
        d = [pp[k] - yy[k] for k in range(3)]
        len2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
        flat = keep & (~(len2 > 0.0) | ~np.isfinite(len2))
        keep = keep & ~flat
        ln = np.sqrt(len2)
        nn = [c[k] / ln for k in range(3)]
        r = A._dot(nn, d)
        row = [yy[1] * nn[2] - yy[2] * nn[1], yy[2] * nn[0] - yy[0] * nn[2], yy[0] * nn[1] - yy[1] * nn[0], nn[0], nn[1], nn[2], A._dot(nn, yy)]
        cols = [row[i] * row[j] for i in range(7) for j in range(i, 7)] + [row[i] * r for i in range(7)] + [one, r * r]
    t = np.stack(cols, -1) if n else np.zeros((0, 37))
    stats = np.array([none.sum(), nonfinite.sum(), 0, flat.sum()], np.uint32)
    return np.where(keep[:, None], t, 0.0), stats


def sums_normals(y, p, nrm, index):
    t, stats = terms_normals(y, p, nrm, index)
    return A.partials(t), stats
