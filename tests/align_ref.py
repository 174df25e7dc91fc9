"""numpy restatement of the registration contract (include/nerfpp_hip.h "Registration": nrf_align_state_init, nrf_align_apply, nrf_align_sums, nrf_align_solve) and of
the ICP loop built on it: float64, one operation per source operation, scalar Python loops (a Python float is an IEEE double) wherever the order matters; the sums
go through tests/ordered_sum_ref.py and the closest points through the brute force of tests/closest_ref.py / tests/geometry_ref.py.  The GPU tests compare with it
bit for bit.  Also the inputs the host and GPU tests share.  Imports nothing of the package."""
import math

import numpy as np

import closest_ref as CR
import geometry_ref as G
import ordered_sum_ref as OS

F32, F64 = np.float32, np.float64
POINT, PLANE = 0, 1
TILE, BLOCK = 1024, 256
COLUMNS = {POINT: 19, PLANE: 37}
SWEEPS, BIG_THETA = 8, 1e150
OK, FEW_PAIRS, NO_SPREAD, BAD_PIVOT, BAD_SCALE, BAD_ROTATION = range(6)
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)
PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def bits64(a):
    return np.ascontiguousarray(a, F64).view(np.uint64)


# ---- the pose ----
def quat_rot(w, x, y, z):
    """R of the header, row-major list of 9 (scalars or arrays)"""
    return [1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
            2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
            2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]


def state_init(pose=None):
    if pose is None:
        return list(IDENTITY)
    p = [float(v) for v in pose]
    nrm = math.sqrt(((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]) + p[3] * p[3])
    return [p[0] / nrm, p[1] / nrm, p[2] / nrm, p[3] / nrm] + p[4:]


def apply(points, state, rotate_only=False):
    """[n, 3] f32 -> [n, 3] f32"""
    x = np.asarray(points, F32).reshape(-1, 3).astype(F64)
    st = [F64(v) for v in state]
    R = quat_rot(*st[:4])
    M = R if rotate_only else [st[4] * r for r in R]
    out = np.empty(x.shape, F32)
    with np.errstate(all="ignore"):
        for a in range(3):
            r = (M[a * 3 + 0] * x[:, 0] + M[a * 3 + 1] * x[:, 1]) + M[a * 3 + 2] * x[:, 2]
            out[:, a] = (r if rotate_only else r + st[5 + a]).astype(F32)
    return out


def matrix(state):
    """[4, 4] float64 of a state: [[s R, t], [0 0 0 1]]"""
    m = np.eye(4)
    m[:3, :3] = state[4] * np.array(quat_rot(*state[:4])).reshape(3, 3)
    m[:3, 3] = state[5:8]
    return m


# ---- the sums ----
def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def terms(y, p, face, mode, verts=None, faces=None):
    """-> (terms [n, NV] float64, zero rows where the pair is dropped; stats [4] u32)"""
    y32, p32 = np.asarray(y, F32).reshape(-1, 3), np.asarray(p, F32).reshape(-1, 3)
    face = np.asarray(face, np.int32).reshape(-1)
    n = len(face)
    none = face < 0
    nonfinite = ~none & ~(np.isfinite(y32).all(-1) & np.isfinite(p32).all(-1))
    keep = ~none & ~nonfinite
    stats = np.array([none.sum(), nonfinite.sum(), 0, 0], np.uint32)
    yy, pp = [y32[:, k].astype(F64) for k in range(3)], [p32[:, k].astype(F64) for k in range(3)]
    one = np.ones(n)
    with np.errstate(all="ignore"):
        d = [pp[k] - yy[k] for k in range(3)]
        if mode == POINT:
            cols = [one] + yy + pp + [yy[a] * pp[b] for a in range(3) for b in range(3)] + [_dot(yy, yy), _dot(pp, pp), _dot(d, d)]
        else:
            cls, A, B, C = CR.face_classes(verts, faces)
            nf = len(cls)
            inside = face < nf
            fi = np.where(keep & inside, face, 0)
            bad = keep & (~inside | (cls[fi] != 0 if nf else True))
            if nf == 0:
                A = B = C = np.zeros((1, 3), F32)
            a64, b64, c64 = A[fi].astype(F64), B[fi].astype(F64), C[fi].astype(F64)
            e1 = [b64[:, k] - a64[:, k] for k in range(3)]
            e2 = [c64[:, k] - a64[:, k] for k in range(3)]
            c = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
            len2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
            flat = keep & ~bad & ~(len2 > 0.0)
            stats[2], stats[3] = bad.sum(), flat.sum()
            keep = keep & ~bad & ~flat
            ln = np.sqrt(len2)
            nn = [c[k] / ln for k in range(3)]
            r = _dot(nn, d)
            row = [yy[1] * nn[2] - yy[2] * nn[1], yy[2] * nn[0] - yy[0] * nn[2], yy[0] * nn[1] - yy[1] * nn[0], nn[0], nn[1], nn[2], _dot(nn, yy)]
            cols = [row[i] * row[j] for i in range(7) for j in range(i, 7)] + [row[i] * r for i in range(7)] + [one, r * r]
    t = np.stack(cols, -1)
    assert t.shape == (n, COLUMNS[mode]) and t.dtype == F64
    return np.where(keep[:, None], t, 0.0), stats          # an accumulator is never -0.0, so adding +0.0 for a dropped pair equals skipping it


def partials(t):
    """terms [n, NV] -> [blocks, NV]: lane l of block k adds entries l, l + 256, ... of its tile in ascending order from 0.0, then the ordered block sum"""
    n, nv = t.shape
    nb = max(1, -(-n // TILE))
    pad = np.zeros((nb * TILE, nv))
    pad[:n] = t
    pad = pad.reshape(nb, TILE // BLOCK, BLOCK, nv)
    acc = np.zeros((nb, BLOCK, nv))
    for j in range(TILE // BLOCK):
        acc = acc + pad[:, j]
    return np.stack([OS.block_sums(acc[:, :, c]) for c in range(nv)], -1)


def totals(part):
    return [float(OS.finish(part[:, c])) for c in range(part.shape[1])]


def sums(y, p, face, mode, verts=None, faces=None):
    """-> (partials [blocks, NV], stats [4])"""
    t, stats = terms(y, p, face, mode, verts, faces)
    return partials(t), stats


# ---- the solve: Python floats only ----
def solve_point(T, scale):
    """-> (flag, dq [4], ds, dt [3])"""
    ident = ([1.0, 0.0, 0.0, 0.0], 1.0, [0.0, 0.0, 0.0])
    cnt = T[0]
    if not cnt >= 3.0:
        return (FEW_PAIRS,) + ident
    sy, sp = T[1:4], T[4:7]
    yb, pb = [v / cnt for v in sy], [v / cnt for v in sp]
    S = [[T[7 + 3 * a + b] - (sy[a] * sp[b]) / cnt for b in range(3)] for a in range(3)]
    vy = T[16] - _dot(sy, sy) / cnt
    if not vy > 0.0:
        return (NO_SPREAD,) + ident
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = S
    A = [[0.0] * 4 for _ in range(4)]
    A[0][0], A[1][1], A[2][2], A[3][3] = (Sxx + Syy) + Szz, (Sxx - Syy) - Szz, (Syy - Sxx) - Szz, (Szz - Sxx) - Syy
    A[0][1] = A[1][0] = Syz - Szy
    A[0][2] = A[2][0] = Szx - Sxz
    A[0][3] = A[3][0] = Sxy - Syx
    A[1][2] = A[2][1] = Sxy + Syx
    A[1][3] = A[3][1] = Szx + Sxz
    A[2][3] = A[3][2] = Syz + Szy
    V = [[1.0 if a == b else 0.0 for b in range(4)] for a in range(4)]
    for _ in range(SWEEPS):
        for p, q in PAIRS:
            apq = A[p][q]
            if apq == 0.0:
                continue
            th = (A[q][q] - A[p][p]) / (2.0 * apq)
            if abs(th) > BIG_THETA:
                t = 0.5 / th
            else:
                t = (1.0 if th >= 0.0 else -1.0) / (abs(th) + math.sqrt(th * th + 1.0))
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            for k in range(4):
                akp, akq = A[k][p], A[k][q]
                A[k][p], A[k][q] = c * akp - s * akq, s * akp + c * akq
            for k in range(4):
                apk, aqk = A[p][k], A[q][k]
                A[p][k], A[q][k] = c * apk - s * aqk, s * apk + c * aqk
            for k in range(4):
                vkp, vkq = V[k][p], V[k][q]
                V[k][p], V[k][q] = c * vkp - s * vkq, s * vkp + c * vkq
    best = 0
    for k in range(1, 4):
        if A[k][k] > A[best][best]:
            best = k
    q = [V[k][best] for k in range(4)]
    if q[0] < 0.0:
        q = [-v for v in q]
    nrm = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    if not nrm > 0.0 or not math.isfinite(nrm):
        return (BAD_ROTATION,) + ident
    dq = [v / nrm for v in q]
    R = quat_rot(*dq)
    ds = 1.0
    if scale:
        num = None
        for a in range(3):
            for b in range(3):
                term = R[a * 3 + b] * S[b][a]
                num = term if num is None else num + term
        ds = num / vy
        if not ds > 0.0 or not math.isfinite(ds):
            return (BAD_SCALE,) + ident
    dt = [pb[a] - ds * ((R[a * 3 + 0] * yb[0] + R[a * 3 + 1] * yb[1]) + R[a * 3 + 2] * yb[2]) for a in range(3)]
    return OK, dq, ds, dt


def plane_system(T):
    """-> (H [7][7], g [7]) of the plane totals"""
    H = [[0.0] * 7 for _ in range(7)]
    c = 0
    for a in range(7):
        for b in range(a, 7):
            H[a][b] = H[b][a] = T[c]
            c += 1
    return H, list(T[28:35])


def solve_plane(T, scale):
    ident = ([1.0, 0.0, 0.0, 0.0], 1.0, [0.0, 0.0, 0.0])
    m = 7 if scale else 6
    if not T[35] >= float(m):
        return (FEW_PAIRS,) + ident
    H, g = plane_system(T)
    Lc = [[0.0] * 7 for _ in range(7)]
    for j in range(m):
        d = H[j][j]
        for k in range(j):
            d = d - Lc[j][k] * Lc[j][k]
        if not d > 0.0 or not math.isfinite(d):
            return (BAD_PIVOT,) + ident
        Lc[j][j] = math.sqrt(d)
        for i in range(j + 1, m):
            v = H[i][j]
            for k in range(j):
                v = v - Lc[i][k] * Lc[j][k]
            Lc[i][j] = v / Lc[j][j]
    z, x = [0.0] * 7, [0.0] * 7
    for i in range(m):
        v = g[i]
        for k in range(i):
            v = v - Lc[i][k] * z[k]
        z[i] = v / Lc[i][i]
    for i in range(m - 1, -1, -1):
        v = z[i]
        for k in range(i + 1, m):
            v = v - Lc[k][i] * x[k]
        x[i] = v / Lc[i][i]
    if not all(math.isfinite(v) for v in x[:m]):
        return (BAD_PIVOT,) + ident
    qa, qb, qc = x[0] / 2.0, x[1] / 2.0, x[2] / 2.0
    nrm = math.sqrt(((1.0 + qa * qa) + qb * qb) + qc * qc)
    if not math.isfinite(nrm):
        return (BAD_ROTATION,) + ident
    ds = 1.0 + x[6] if scale else 1.0
    if not ds > 0.0 or not math.isfinite(ds):
        return (BAD_SCALE,) + ident
    return OK, [1.0 / nrm, qa / nrm, qb / nrm, qc / nrm], ds, [x[3], x[4], x[5]]


def compose(state, dq, ds, dt):
    w, x, y, z = state[:4]
    t = state[5:8]
    q = [((dq[0] * w - dq[1] * x) - dq[2] * y) - dq[3] * z, ((dq[0] * x + dq[1] * w) + dq[2] * z) - dq[3] * y,
         ((dq[0] * y - dq[1] * z) + dq[2] * w) + dq[3] * x, ((dq[0] * z + dq[1] * y) - dq[2] * x) + dq[3] * w]
    nrm = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    R = quat_rot(*dq)
    return [v / nrm for v in q] + [ds * state[4]] + [ds * ((R[a * 3 + 0] * t[0] + R[a * 3 + 1] * t[1]) + R[a * 3 + 2] * t[2]) + dt[a] for a in range(3)]


def solve(part, mode, scale, state):
    """partials [blocks, NV] and a state (8 floats) -> (the new state, the history row [8])"""
    T = totals(part)
    state = [float(v) for v in state]
    flag, dq, ds, dt = solve_point(T, scale) if mode == POINT else solve_plane(T, scale)
    new = compose(state, dq, ds, dt) if flag == OK else state
    row = [T[0] if mode == POINT else T[35], T[18] if mode == POINT else T[36], float(flag), 2.0 * math.sqrt((dq[1] * dq[1] + dq[2] * dq[2]) + dq[3] * dq[3]),
           math.sqrt((dt[0] * dt[0] + dt[1] * dt[1]) + dt[2] * dt[2]), ds, new[4], 0.0]
    return new, row


def align_points(src, dst, scale):
    part, _ = sums(src, dst, np.zeros(len(src), np.int32), POINT)
    return solve(part, POINT, scale, IDENTITY)


# ---- the ICP loop ----
def closest_pruned(query, verts, faces, max_dist=np.inf, slack=1e-3):
    """CR.closest's d2, face and point (tests/test_align_host.py holds it to that brute force bit for bit) at a fraction of the pairs.  Still grid-free: a face is
    left out for a query only where the float64 distance from the query to the face's coordinate box exceeds, by the slack, its distance to some face's first
    corner.  The header's closest point is clamped to that box, so such a face's d2 is above the d2 of the face that owns the corner and it can neither win nor tie.
    Inputs outside that argument (non-finite values, invalid faces, an empty mesh) go to the brute force itself."""
    q = np.asarray(query, F32).reshape(-1, 3)
    cls, a, b, c = CR.face_classes(verts, faces)
    if len(cls) == 0 or (cls != 0).any() or not np.isfinite(q).all():
        return CR.closest(q, verts, faces, max_dist=max_dist)
    q64, a64 = q.astype(F64), a.astype(F64)
    lo, hi = np.minimum(np.minimum(a, b), c).astype(F64), np.maximum(np.maximum(a, b), c).astype(F64)
    upper = ((q64[:, None, :] - a64[None]) ** 2).sum(-1).min(1)
    gap = np.maximum(np.maximum(lo[None] - q64[:, None, :], q64[:, None, :] - hi[None]), 0.0)
    qi, fi = np.nonzero((gap ** 2).sum(-1) <= upper[:, None] * (1.0 + slack) + 1e-30)
    r = CR.closest_on_triangle(q[qi], a[fi], b[fi], c[fi])
    with np.errstate(all="ignore"):
        md2 = F32(max_dist) * F32(max_dist)
    key = (r["d2"].view(np.uint32).astype(np.uint64) << np.uint64(32)) | fi.astype(np.uint64)
    best = np.full(len(q), CR.NONE, np.uint64)
    np.minimum.at(best, qi, np.where(r["d2"] <= md2, key, CR.NONE))
    d2 = (best >> np.uint64(32)).astype(np.uint32).view(F32)
    face = (best & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    point = np.zeros((len(q), 3), F32)
    hit = face >= 0
    if hit.any():
        point[hit] = CR.closest_on_triangle(q[hit], a[face[hit]], b[face[hit]], c[face[hit]])["p"]
    return dict(d2=d2, face=face, point=point)


def icp(src, target, mode, scale, iterations, max_dist=np.inf, init=None, tolerance=None, check_every=5, closest=closest_pruned):
    """src [n, 3] f32; target (verts, faces) -- closest point through `closest`, CR.closest or its pruned twin -- or points [m, 3] (POINT only) -> (state, history [its, 8],
    states [its + 1] the state before every iteration and after the last)"""
    state = state_init(init)
    dists = [max_dist] * iterations if np.isscalar(max_dist) else list(max_dist)
    history, states = [], [list(state)]
    for it in range(iterations):
        y = apply(src, state)
        if isinstance(target, tuple):
            r = closest(y, target[0], target[1], max_dist=dists[it])
            p, face = r["point"], r["face"]
            part, _ = sums(y, p, face, mode, target[0], target[1])
        else:
            _, face, _ = G.nearest(y, target, max_dist=dists[it])
            p = np.asarray(target, F32)[np.maximum(face, 0)]
            part, _ = sums(y, p, face, mode)
        state, row = solve(part, mode, scale, state)
        history.append(row)
        states.append(list(state))
        if tolerance is not None and (it + 1) % check_every == 0 and row[3] < tolerance and row[4] < tolerance:
            break
    return state, np.array(history, F64), np.array(states, F64)


# ---- the inputs of the tests ----
SEMI_AXES = np.array([0.5, 0.35, 0.2])
BUMP_AT, BUMP_HEIGHT, BUMP_WIDTH = np.array([0.6, 0.64, 0.48]), 0.35, 8.0
TRUE_AXIS, TRUE_DEG, TRUE_SCALE, TRUE_SHIFT = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0), 10.0, 1.1, np.array([0.05, -0.03, 0.02])
N_SAMPLES, SAMPLE_SEED = 2000, 0


def bumped_ellipsoid(d):
    """unit directions [n, 3] -> points of the test surface: an ellipsoid with a bump, so that no rotation maps it onto itself"""
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    return d * (1.0 + BUMP_HEIGHT * np.exp(-BUMP_WIDTH * ((d - BUMP_AT) ** 2).sum(1)))[:, None] * SEMI_AXES


def ico_sphere(levels=3):
    """An icosahedron subdivided `levels` times onto the unit sphere: (verts [V, 3] f64, faces [F, 3] i32), counter-clockwise seen from outside; 642 / 1280 at 3"""
    g = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, F64) / np.linalg.norm(p) for p in v]
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
    return np.array(v), np.array(f, np.int32)


def rotation(axis, deg):
    a = np.deg2rad(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def ellipsoid_case():
    """The registration problem of the tests -> dict(target=(verts, faces) of the bumped ellipsoid at 1280 faces, source=(verts, faces) the same surface in another
    frame (x = R^T (v - t) / s, so the true pose source -> target is (R, s, t)), R, s, t)"""
    d, faces = ico_sphere(3)
    tv = bumped_ellipsoid(d).astype(F32)
    R = rotation(TRUE_AXIS, TRUE_DEG)
    sv = ((tv.astype(F64) - TRUE_SHIFT) @ R / TRUE_SCALE).astype(F32)
    return dict(target=(tv, faces), source=(sv, faces), R=R, s=TRUE_SCALE, t=TRUE_SHIFT)


def surface_samples(verts, faces, n_points=N_SAMPLES, seed=SAMPLE_SEED):
    """What SampleSurface(mesh, n_points=n_points, seed=seed).Points holds: the area from a count at density 0, then density = n_points / area"""
    area = G.sample_count(verts, faces, 0.0, seed)["total_area"]
    density = F32(float(n_points) / area)
    return G.sample(verts, faces, density, seed)[1]


def pose_error(state, case):
    """(rotation error in degrees, |s - s_true|, |t - t_true|_inf) of a state against the true pose"""
    R = np.array(quat_rot(*state[:4])).reshape(3, 3)
    E = R @ case["R"].T          # the angle from the skew part as well: arccos of the trace alone cannot tell angles below 1e-6 degrees from zero
    sin = 0.5 * math.sqrt((E[2, 1] - E[1, 2]) ** 2 + (E[0, 2] - E[2, 0]) ** 2 + (E[1, 0] - E[0, 1]) ** 2)
    return math.degrees(math.atan2(sin, (np.trace(E) - 1.0) / 2.0)), abs(state[4] - case["s"]), float(np.abs(np.array(state[5:8]) - case["t"]).max())
