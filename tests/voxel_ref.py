"""numpy restatement of the mesh voxelisation contract (include/nerfpp_hip.h: nrf_mesh_voxelize), steps 1-10 by brute force: every face against every column and every
lattice point, int64 edge functions, one numpy fp32 operation per source operation in the stated order.  It knows nothing of bounding boxes of columns, wide lists or
workgroups; the lattice box of step 7 is applied as the mask the header states.  The GPU tests compare with it bit for bit.  Also the inputs the host and GPU tests
share.  Imports nothing of the package."""
import numpy as np

import closest_ref as CR

F32 = np.float32
SUBPIXEL, GUARD = 256, 16384          # NRF_RASTER_SUBPIXEL, NRF_RASTER_GUARD
NONZERO, POSITIVE, ODD = 0, 1, 2
RULES = (NONZERO, POSITIVE, ODD)
NONE = CR.NONE


def lattice(bbox, dims):
    """-> (bmin [3] f32, step [3] f32): step = (bmax - bmin) / (float)(n - 1)"""
    b = np.asarray(bbox, F32).reshape(6)
    n = np.asarray(dims, np.int64)
    step = (b[3:] - b[:3]) / (n - 1).astype(F32)
    assert step.dtype == F32
    return b[:3].copy(), step


def lattice_points(bbox, dims):
    """P [nz, ny, nx, 3] f32 = bmin + (float)i * step"""
    bmin, step = lattice(bbox, dims)
    nx, ny, nz = dims
    ax = [bmin[a] + np.arange(n).astype(F32) * step[a] for a, n in enumerate((nx, ny, nz))]
    P = np.empty((nz, ny, nx, 3), F32)
    P[..., 0], P[..., 1], P[..., 2] = ax[0][None, None, :], ax[1][None, :, None], ax[2][:, None, None]
    return P


def inside_of(winding, rule):
    return winding != 0 if rule == NONZERO else (winding > 0 if rule == POSITIVE else (winding & 1) != 0)


def delta_of(verts, faces, bbox, dims):
    """Steps 1-5 -> (delta [nz, ny, nx] int32, stats [4] uint32: clipped, bad, non-finite, 0, covered [F, ny, nx] int8: s where face f covers the column)"""
    nx, ny, nz = dims
    bmin, step = lattice(bbox, dims)
    V = np.asarray(verts, F32).reshape(-1, 3)
    fc = np.asarray(faces, np.int64).reshape(-1, 3)
    cls, _, _, _ = CR.face_classes(V, fc)
    with np.errstate(all="ignore"):
        g = ((V - bmin) / step).astype(F32)
        ok = (np.abs(g[:, 0]) <= F32(GUARD)) & (np.abs(g[:, 1]) <= F32(GUARD))
        X = np.where(ok, np.rint(g[:, 0] * F32(SUBPIXEL)), 0).astype(np.int64)
        Y = np.where(ok, np.rint(g[:, 1] * F32(SUBPIXEL)), 0).astype(np.int64)
    delta = np.zeros((nz, ny, nx), np.int64)
    covered = np.zeros((len(fc), ny, nx), np.int8)
    px = (SUBPIXEL * np.arange(nx, dtype=np.int64))[None, :]
    py = (SUBPIXEL * np.arange(ny, dtype=np.int64))[:, None]
    jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    clipped = 0
    for f in range(len(fc)):
        if cls[f] != 0:
            continue
        v = fc[f]
        if not ok[v].all():
            clipped += 1
            continue
        x, y, gz = X[v], Y[v], g[v, 2]
        A = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
        if A == 0:
            continue
        s = 1 if A > 0 else -1
        inside = np.ones((ny, nx), bool)
        se = []
        for k in range(3):
            ia, ib = (k + 1) % 3, (k + 2) % 3          # e0 = E_12, e1 = E_20, e2 = E_01
            e = (x[ib] - x[ia]) * (py - y[ia]) - (y[ib] - y[ia]) * (px - x[ia])
            dx, dy = s * (x[ib] - x[ia]), s * (y[ib] - y[ia])
            tl = dy < 0 or (dy == 0 and dx > 0)
            se.append(s * e)
            inside &= (se[k] > 0) | ((se[k] == 0) & tl)
        with np.errstate(all="ignore"):
            b = [(se[k].astype(np.float64) / np.float64(s * A)).astype(F32) for k in range(3)]
            zc = (b[0] * gz[0] + b[1] * gz[1]) + b[2] * gz[2]
            assert zc.dtype == F32
            t = np.ceil(zc) - F32(1)
            take = inside & (t >= 0)          # NaN fails
            kc = np.minimum(np.where(take, t, 0), F32(nz - 1)).astype(np.int64)
        np.add.at(delta, (kc[take], jj[take], ii[take]), s)
        covered[f] = np.where(inside, s, 0)
    stats = np.array([clipped, (cls == 1).sum(), (cls == 2).sum(), 0], np.uint32)
    return delta.astype(np.int32), stats, covered


def winding_of(delta):
    """Step 6: the suffix sum down every column"""
    return np.flip(np.cumsum(np.flip(delta.astype(np.int64), 0), 0), 0).astype(np.int32)


def face_box(a, b, c, bbox, dims, trunc):
    """Step 7 for one face -> (lo [3], hi [3]) ints, or None where the box is empty"""
    bmin, step = lattice(bbox, dims)
    tr = F32(trunc)
    with np.errstate(all="ignore"):
        l, h = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
        top = (np.asarray(dims) - 1).astype(F32)
        fl = np.floor(((l - tr) - bmin) / step) - F32(1)
        fh = np.ceil(((h + tr) - bmin) / step) + F32(1)
        assert fl.dtype == F32 and fh.dtype == F32
        if not ((fh >= 0) & (fl <= top)).all():
            return None
        return np.maximum(fl, F32(0)).astype(np.int64), np.minimum(fh, top).astype(np.int64)


def keys_of(verts, faces, bbox, dims, trunc, use_box=True):
    """Steps 7-8 -> key [nz, ny, nx] uint64.  use_box=False: every face against every lattice point, what WHY THE BOX IS COMPLETE says changes nothing"""
    nx, ny, nz = dims
    cls, a, b, c = CR.face_classes(verts, faces)
    P = lattice_points(bbox, dims)
    with np.errstate(all="ignore"):
        t2 = F32(trunc) * F32(trunc)
    key = np.full((nz, ny, nx), NONE, np.uint64)
    for f in range(len(cls)):
        if cls[f] != 0:
            continue
        mask = np.ones((nz, ny, nx), bool)
        if use_box:
            box = face_box(a[f], b[f], c[f], bbox, dims, trunc)
            if box is None:
                continue
            lo, hi = box
            mask[:] = False
            mask[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = True
        d2 = CR.closest_on_triangle(P, a[f], b[f], c[f])["d2"]
        k = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
        with np.errstate(all="ignore"):
            okk = mask & (d2 <= t2)          # a NaN d2 fails the comparison
        key = np.where(okk, np.minimum(key, k), key)
    return key


def voxelize(verts, faces, bbox, dims, trunc, rule, use_box=True):
    """Steps 1-10 -> dict(winding int32, sdf f32, face int32 (each [nz, ny, nx]), stats [4] uint32, key uint64)"""
    delta, stats, _ = delta_of(verts, faces, bbox, dims)
    winding = winding_of(delta)
    key = keys_of(verts, faces, bbox, dims, trunc, use_box)
    found = key != NONE
    d2 = (key >> np.uint64(32)).astype(np.uint32).view(F32)
    face = np.where(found, (key & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    tr = F32(trunc)
    with np.errstate(all="ignore"):
        dist = np.minimum(np.where(found, np.sqrt(d2), tr), tr).astype(F32)
    sdf = np.where(inside_of(winding, rule), -dist, dist).astype(F32)
    return dict(winding=winding, sdf=sdf, face=face, stats=stats, key=key)


# ---- the inputs of the tests ----
# the two lattices of the GPU tests: (bbox, (nx, ny, nz)); the first has steps of exactly 0.25, the second inexact ones
LATTICE_EXACT = (np.array([-1.0, -0.5, -2.0, 1.0, 0.5, 2.0], F32), (9, 5, 17))
LATTICE_INEXACT = (np.array([-1.1, -0.9, -1.0, 1.3, 1.0, 0.7], F32), (7, 6, 5))
LATTICES = {"exact": LATTICE_EXACT, "inexact": LATTICE_INEXACT}
_QUADS = ((0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5))          # -z +z -y +y -x +x, counter-clockwise seen from outside


def cube(lo, hi, flip=False):
    """The box [lo, hi] as 8 vertices (bit 0 = x, bit 1 = y, bit 2 = z) and 12 outward-oriented faces; flip reverses every face"""
    lo, hi = np.broadcast_to(np.asarray(lo, F32), 3), np.broadcast_to(np.asarray(hi, F32), 3)
    V = np.array([[(hi if (i >> a) & 1 else lo)[a] for a in range(3)] for i in range(8)], F32)
    Fc = np.array([t for q in _QUADS for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.int32)
    return V, (Fc[:, ::-1].copy() if flip else Fc)


def merge(*meshes):
    """One vertex and face list of several (V, F) pairs"""
    Vs, Fs, at = [], [], 0
    for V, Fc in meshes:
        Vs.append(np.asarray(V, F32))
        Fs.append(np.asarray(Fc, np.int32) + at)
        at += len(V)
    return np.concatenate(Vs), np.concatenate(Fs).astype(np.int32)


def icosphere(radius=0.8, centre=(0.0, 0.0, 0.0), subdivisions=1):
    """An outward-oriented icosphere: 20 * 4^subdivisions faces (80 at one subdivision)"""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    V = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    Fc = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6),
          (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    V = [np.asarray(v, np.float64) / np.linalg.norm(v) for v in V]
    for _ in range(subdivisions):
        mid, out = {}, []

        def m(i, j):
            k = (min(i, j), max(i, j))
            if k not in mid:
                w = V[i] + V[j]
                V.append(w / np.linalg.norm(w))
                mid[k] = len(V) - 1
            return mid[k]
        for a, b, c in Fc:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        Fc = out
    V = np.asarray(V)
    Fc = np.asarray(Fc, np.int32)
    n = np.cross(V[Fc[:, 1]] - V[Fc[:, 0]], V[Fc[:, 2]] - V[Fc[:, 0]])
    assert ((n * V[Fc].mean(1)).sum(1) > 0).all()          # counter-clockwise seen from outside
    return (V * radius + np.asarray(centre)).astype(F32), Fc


def quad_stack(n=64):
    """n coincident quads (2 n faces over 4 vertices), alternately facing +z and -z but for the last two: they all contend for the same columns and keys"""
    V = np.array([[-0.6, -0.3, 0.3], [0.55, -0.3, 0.3], [0.55, 0.35, 0.3], [-0.6, 0.35, 0.3]], F32)
    Fc = []
    for q in range(n):
        up = q % 2 == 0 or q >= n - 2
        Fc += [(0, 1, 2), (0, 2, 3)] if up else [(0, 2, 1), (0, 3, 2)]
    return V, np.asarray(Fc, np.int32)


def meshes():
    """name -> (V, F): the meshes of the GPU tests, sized for both lattices"""
    out = {}
    out["cube_between"] = cube((-0.6, -0.3, -0.9), (0.55, 0.35, 0.6))                      # faces between lattice planes of the exact lattice
    out["cube_on_columns"] = cube((-0.5, -0.25, -1.0), (0.5, 0.25, 0.5))                   # vertices on lattice columns of the exact lattice
    out["cube_inverted"] = cube((-0.6, -0.3, -0.9), (0.55, 0.35, 0.6), flip=True)
    out["cube_nested_like"] = merge(cube((-0.8, -0.4, -0.9), (0.8, 0.4, 0.6)), cube((-0.3, -0.2, -0.4), (0.3, 0.2, 0.3)))
    out["cube_nested_cavity"] = merge(cube((-0.8, -0.4, -0.9), (0.8, 0.4, 0.6)), cube((-0.3, -0.2, -0.4), (0.3, 0.2, 0.3), flip=True))
    out["icosphere"] = icosphere(0.45, (0.05, 0.02, -0.1))
    out["open_triangle"] = (np.array([[-0.7, -0.4, 0.1], [0.8, -0.3, -0.2], [0.1, 0.45, 0.4]], F32), np.array([[0, 1, 2]], np.int32))
    out["z_parallel"] = (np.array([[-0.5, 0.1, -0.5], [0.5, 0.1, -0.5], [0.0, 0.1, 0.5]], F32), np.array([[0, 1, 2]], np.int32))
    out["quad_stack"] = quad_stack(64)
    V, Fc = cube((-0.6, -0.3, -0.9), (0.55, 0.35, 0.6))
    V = np.concatenate([V, np.array([[np.nan, 0.0, 0.0]], F32)])
    out["bad_and_nan"] = (V, np.concatenate([Fc, np.array([[0, 1, 8], [0, 9, 1], [-1, 2, 3]], np.int32)]))          # one NaN face, two bad-index faces
    out["beyond_box"] = merge(cube((-3.0, -2.5, -4.5), (2.75, 2.25, 5.0)), cube((-0.3, -0.2, -6.0), (0.3, 0.2, 7.0)),
                              (np.array([[-5, -5, -3.0], [5, -5, -2.5], [0, 6, -2.25], [-5, -5, 9.0], [5, -5, 9.5], [0, 6, 8.0]], F32),
                               np.array([[0, 1, 2], [3, 4, 5]], np.int32)))
    # vertices 1 and 4 have equal coordinates and different indices, on the edge the two faces share
    out["twin_vertices"] = (np.array([[-0.5, -0.3, 0.2], [0.5, -0.25, 0.1], [0.1, 0.4, 0.3], [0.9, 0.45, -0.2], [0.5, -0.25, 0.1]], F32),
                            np.array([[0, 1, 2], [4, 3, 2]], np.int32))
    return out


def wide_case():
    """(bbox, dims, (V, F) with two triangles that span the whole 33 x 33 x 9 lattice beside 40 small ones, (V, F) with the two wide faces split at the midpoint of
    their shared diagonal into four).  The split keeps the union of the covered columns: winding agrees, the distances need not."""
    bbox, dims = np.array([-2.0, -2.0, -1.0, 2.0, 2.0, 1.0], F32), (33, 33, 9)
    big = np.array([[-2.5, -2.5, 0.1], [2.5, -2.5, 0.1], [2.5, 2.5, 0.1], [-2.5, 2.5, 0.1], [0.0, 0.0, 0.1]], F32)
    small_v, small_f = icosphere(0.5, (0.3, -0.2, 0.4), 0)
    extra_v, extra_f = icosphere(0.3, (-1.0, 1.0, -0.5), 0)
    wide = merge((big, np.array([[0, 1, 2], [0, 2, 3]], np.int32)), (small_v, small_f), (extra_v, extra_f))
    split = merge((big, np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]], np.int32)), (small_v, small_f), (extra_v, extra_f))
    return bbox, dims, wide, split
