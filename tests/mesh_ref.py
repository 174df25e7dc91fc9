"""numpy restatement of the mesh export's contract (include/nerfpp_hip.h, nrf_density_grid / nrf_isosurface_*): lattice points, marching tetrahedra on
the Kuhn split, vertex / face order, winding and normals.  Every fp32 operation is the one the kernels perform, so the GPU output is compared with this bit for
bit (normals: within 1e-6).  Vectorised over cells; the host tests pin it on analytic fields."""
import numpy as np

F32 = np.float32
# edge types: offsets of the far end from the origin lattice point, in order
EDGE_OFFSETS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
# axis permutations xyz, xzy, yxz, yzx, zxy, zyx
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
PERM_ODD = (0, 1, 1, 0, 0, 1)


def _corner(off):
    """cell corner index of an (x, y, z) offset: bit 0 = x, bit 1 = y, bit 2 = z"""
    return off[0] | (off[1] << 1) | (off[2] << 2)


TYPE_OF_DIFF = {_corner(o): t for t, o in enumerate(EDGE_OFFSETS)}


def lattice_axes(bbox, nx, ny, nz):
    """P per axis: bmin + (float)i * step, step = (bmax - bmin) / (float)(n - 1), all fp32 -> (xs, ys, zs)"""
    b = np.asarray(bbox, F32).reshape(6)
    out = []
    for a, n in enumerate((nx, ny, nz)):
        step = (b[3 + a] - b[a]) / F32(n - 1)
        out.append(b[a] + np.arange(n, dtype=F32) * step)
    return out


def lattice_points(bbox, nx, ny, nz):
    """[nz, ny, nx, 3] fp32 lattice points (x fastest)"""
    xs, ys, zs = lattice_axes(bbox, nx, ny, nz)
    z, y, x = np.meshgrid(zs, ys, xs, indexing="ij")
    return np.stack([x, y, z], -1).astype(F32)


def chain(perm):
    """the 4 cell corners of tetrahedron `perm`: c, c + e_p0, c + e_p0 + e_p1, c + (1,1,1)"""
    c1 = 1 << perm[0]
    c2 = c1 | (1 << perm[1])
    return (0, c1, c2, 7)


def tet_triangles(mask, odd):
    """triangles of a tetrahedron whose chain corners j with bit j of `mask` are inside: a list of triangles, each three edges (j, k) of chain positions j < k,
    wound counter-clockwise seen from outside"""
    ins = [j for j in range(4) if mask >> j & 1]
    out = [j for j in range(4) if not mask >> j & 1]
    e = lambda u, w: (min(u, w), max(u, w))
    if len(ins) in (1, 3):
        k = ins[0] if len(ins) == 1 else out[0]
        tris = [[e(k, j) for j in range(4) if j != k]]
        flip = (k & 1) ^ (len(ins) == 3) ^ odd
    elif len(ins) == 2:
        a, b = ins
        c, d = out
        tris = [[e(a, c), e(a, d), e(b, d)], [e(a, c), e(b, d), e(b, c)]]
        flip = ((a + b) % 2 == 0) ^ odd
    else:
        return []
    return [[t[0], t[2], t[1]] for t in tris] if flip else tris


def _grad_axis(f, coords, axis):
    """central difference along a lattice axis of f [nz, ny, nx] (axis 0 = x = numpy axis 2), one-sided at the border"""
    n = f.shape[2 - axis]
    i = np.arange(n)
    lo, hi = np.maximum(i - 1, 0), np.minimum(i + 1, n - 1)
    num = np.take(f, hi, axis=2 - axis) - np.take(f, lo, axis=2 - axis)
    den = coords[hi] - coords[lo]
    shape = [1, 1, 1]
    shape[2 - axis] = n
    return (num / den.reshape(shape)).astype(F32)


def tet_cases(sigma, iso):
    """[C, 6] 4-bit inside masks of every tetrahedron (cells in linear order)"""
    f = np.asarray(sigma, F32)
    inside = f > F32(iso)
    nz, ny, nx = f.shape
    corner = [inside[(o >> 2):nz - 1 + (o >> 2), (o >> 1 & 1):ny - 1 + (o >> 1 & 1), (o & 1):nx - 1 + (o & 1)].reshape(-1) for o in range(8)]
    return np.stack([sum(corner[cc].astype(np.int64) << j for j, cc in enumerate(chain(p))) for p in PERMS], 1)


def isosurface(sigma, bbox, iso):
    """-> (verts [V, 3] f32, faces [F, 3] int32, normals [V, 3] f32, n_nonfinite)"""
    f = np.ascontiguousarray(sigma, F32)
    iso = F32(iso)
    nz, ny, nx = f.shape
    xs, ys, zs = lattice_axes(bbox, nx, ny, nz)
    inside = f > iso
    # ---- vertices: crossed edges in (linear index of the origin, type) order ----
    crossed = np.zeros((nz, ny, nx, 7), bool)
    for t, (dx, dy, dz) in enumerate(EDGE_OFFSETS):
        crossed[:nz - dz, :ny - dy, :nx - dx, t] = inside[:nz - dz, :ny - dy, :nx - dx] != inside[dz:, dy:, dx:]
    flat = crossed.reshape(-1, 7)
    vid = np.full(flat.shape, -1, np.int64)
    a_lin, a_type = np.nonzero(flat)
    vid[a_lin, a_type] = np.arange(a_lin.size)
    az, rem = np.divmod(a_lin, ny * nx)
    ay, ax = np.divmod(rem, nx)
    off = np.asarray(EDGE_OFFSETS)[a_type]
    bx, by, bz = ax + off[:, 0], ay + off[:, 1], az + off[:, 2]
    fa, fb = f[az, ay, ax], f[bz, by, bx]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t = (iso - fa) / (fb - fa)
        pa = np.stack([xs[ax], ys[ay], zs[az]], 1)
        pb = np.stack([xs[bx], ys[by], zs[bz]], 1)
        verts = (pa + t[:, None] * (pb - pa)).astype(F32)
        # ---- normals: lattice gradient interpolated with the same t, n = -g / |g| ----
        grads = [_grad_axis(f, c, a) for a, c in enumerate((xs, ys, zs))]
        ga = np.stack([g[az, ay, ax] for g in grads], 1)
        gb = np.stack([g[bz, by, bx] for g in grads], 1)
        gv = (ga + t[:, None] * (gb - ga)).astype(F32)
        ln = np.sqrt(gv[:, 0] * gv[:, 0] + gv[:, 1] * gv[:, 1] + gv[:, 2] * gv[:, 2])
        normals = np.where(ln[:, None] > 0, -gv / np.where(ln > 0, ln, F32(1))[:, None], F32(0)).astype(F32)
    # ---- faces: cells in linear order of their min corner, tetrahedra in permutation order ----
    cz, cy, cx = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    c_lin = ((cz * ny + cy) * nx + cx).reshape(-1)
    corner_lin = [c_lin + (o & 1) + (o >> 1 & 1) * nx + (o >> 2) * nx * ny for o in range(8)]
    cases = tet_cases(f, iso)
    C = c_lin.size
    tri = np.zeros((C, 6, 2, 3), np.int64)
    valid = np.zeros((C, 6, 2), bool)
    for p, perm in enumerate(PERMS):
        ch = chain(perm)
        for m in range(1, 15):
            sel = np.nonzero(cases[:, p] == m)[0]
            if sel.size == 0:
                continue
            for k, tr in enumerate(tet_triangles(m, PERM_ODD[p])):
                for s, (j, l) in enumerate(tr):
                    lo, hi = ch[j], ch[l]
                    tri[sel, p, k, s] = vid[corner_lin[lo][sel], TYPE_OF_DIFF[lo ^ hi]]
                valid[sel, p, k] = True
    faces = tri[valid].astype(np.int32)
    assert (faces >= 0).all()
    return verts, faces, normals, int((~np.isfinite(f)).sum())


# ---- checks on a mesh ----
def edge_check(faces):
    """(every undirected edge in exactly 2 triangles, every directed edge once)"""
    d = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
    n = int(faces.max()) + 1 if faces.size else 1
    dk = d[:, 0] * n + d[:, 1]
    uk = np.minimum(d[:, 0], d[:, 1]) * n + np.maximum(d[:, 0], d[:, 1])
    _, uc = np.unique(uk, return_counts=True)
    _, dc = np.unique(dk, return_counts=True)
    return bool((uc == 2).all()), bool((dc == 1).all())


def euler(verts, faces):
    d = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
    n = len(verts)
    e = np.unique(np.minimum(d[:, 0], d[:, 1]) * n + np.maximum(d[:, 0], d[:, 1])).size
    return len(np.unique(faces)) - e + len(faces)


def signed_volume(verts, faces):
    v = verts.astype(np.float64)[faces]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def read_ply(path):
    """minimal binary little-endian PLY reader for the writer's layout"""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").splitlines()
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0"
    nv = nf = 0
    fields = []
    for line in head:
        w = line.split()
        if w[:2] == ["element", "vertex"]:
            nv = int(w[2])
        elif w[:2] == ["element", "face"]:
            nf = int(w[2])
        elif w[0] == "property" and w[1] != "list":
            fields.append((w[2], {"float": "<f4", "uchar": "u1"}[w[1]]))
    assert "property list uchar int vertex_indices" in head
    vt = np.dtype(fields)
    verts = np.frombuffer(data, vt, nv, end)
    faces = np.frombuffer(data, np.dtype([("n", "u1"), ("idx", "<i4", (3,))]), nf, end + nv * vt.itemsize)
    assert end + nv * vt.itemsize + nf * 13 == len(data)
    return verts, faces
