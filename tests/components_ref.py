"""Connected components restated in numpy: the canonical labels of include/nerfpp_hip.h (nrf_mesh_components, nrf_lattice_components) by another algorithm --
rounds of "hook every root onto the smallest root it shares an edge with, then flatten", not the library's lock-free union-find.  Components are numbered
0 .. K-1 in ascending order of their smallest member; items that take no part get -1."""
import numpy as np

KUHN = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]            # (dx, dy, dz): the isosurface's 7 edge types


def offsets(connectivity):
    """The forward half of the neighbourhood as (dx, dy, dz); the other half is its negatives."""
    if connectivity == 6:
        return KUHN[:3]
    if connectivity == 14:
        return list(KUHN)
    if connectivity == 26:
        return [(dx, dy, dz) for dz in (0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) > (0, 0, 0)]
    raise ValueError(f"connectivity {connectivity}")


def roots(n, a, b):
    """The smallest member of the component of each of n items joined by the edges (a[k], b[k])."""
    parent = np.arange(n, dtype=np.int64)
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    while True:
        ra, rb = parent[a], parent[b]                       # flat: these are roots
        lo, hi = np.minimum(ra, rb), np.maximum(ra, rb)
        open_ = lo != hi
        if not open_.any():
            return parent
        np.minimum.at(parent, hi[open_], lo[open_])
        while True:
            pp = parent[parent]
            if (pp == parent).all():
                break
            parent = pp


def canonical(root, takes_part):
    """labels [n] int32 and K from the roots: the rank of an item's root among the roots of the items that take part."""
    labels = np.full(root.shape, -1, np.int32)
    uniq, inv = np.unique(root[takes_part], return_inverse=True)
    labels[takes_part] = inv.astype(np.int32)
    return labels, len(uniq)


def mesh_components(faces, n_verts):
    """(labels [V] int32, K): vertices sharing a face share a label; a vertex used by no face gets -1."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    used = np.zeros(n_verts, bool)
    used[f.reshape(-1)] = True
    return canonical(roots(n_verts, np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]])), used)


def lattice_edges(mask, connectivity):
    """Flat indices (a, b) of the pairs of set neighbours of mask [nz, ny, nx], each pair once."""
    m = np.asarray(mask) != 0
    nz, ny, nx = m.shape
    idx = np.arange(m.size, dtype=np.int64).reshape(m.shape)

    def window(n, d):           # (source, neighbour) slices of one axis for the step d
        return (slice(max(0, -d), n - max(0, d)), slice(max(0, d), n - max(0, -d)))
    a, b = [], []
    for dx, dy, dz in offsets(connectivity):
        (sz, tz), (sy, ty), (sx, tx) = window(nz, dz), window(ny, dy), window(nx, dx)
        both = m[sz, sy, sx] & m[tz, ty, tx]
        a.append(idx[sz, sy, sx][both])
        b.append(idx[tz, ty, tx][both])
    return np.concatenate(a), np.concatenate(b)


def lattice_components(mask, connectivity):
    """(labels [nz, ny, nx] int32, K): -1 where the mask is 0."""
    m = np.asarray(mask) != 0
    a, b = lattice_edges(m, connectivity)
    labels, k = canonical(roots(m.size, a, b), m.reshape(-1))
    return labels.reshape(m.shape), k


# ---- the shapes the host and the GPU tests share ----
def strip(n_verts, first=0):
    """Triangle strip over the vertices first .. first + n_verts - 1."""
    i = np.arange(first, first + n_verts - 2, dtype=np.int64)
    return np.stack([i, i + 1, i + 2], 1)


def scramble(faces, n_verts, seed):
    """Vertex ids through a seeded random permutation, face order shuffled."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n_verts)
    f = perm[np.asarray(faces, np.int64)]
    return f[rng.permutation(len(f))].astype(np.int32)


def mesh_cases():
    """name -> (faces [F, 3] int32, V, K)."""
    out = {}
    v = (1 << 17) + 3
    out["strip"] = (scramble(strip(v), v, 1), v, 1)
    tets = np.array([[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]], np.int64)
    f = (tets[None] + 4 * np.arange(5000, dtype=np.int64)[:, None, None]).reshape(-1, 3)
    out["tetrahedra"] = (scramble(f, 20000 + 37, 2), 20000 + 37, 5000)            # the permutation spreads the 37 unused ids
    # two strips that only the last face of the list joins
    rng = np.random.default_rng(3)
    perm = rng.permutation(80000)
    two = np.concatenate([strip(40000), strip(40000, 40000)])
    two = perm[two[rng.permutation(len(two))]]
    out["joined_last"] = (np.concatenate([two, perm[np.array([[39999, 40000, 40001]])]]).astype(np.int32), 80000, 1)
    out["two_strips"] = (two.astype(np.int32), 80000, 2)
    # degenerate (a, a, b), (a, a, a) and exact duplicates mixed into the tetrahedra; (a, a, a) on an unused vertex makes a component of its own
    base, nv, _ = out["tetrahedra"]
    used = np.zeros(nv, bool)
    used[base.reshape(-1)] = True
    free = np.nonzero(~used)[0]
    a, b = base[::7, 0], base[::7, 1]
    extra = np.concatenate([np.stack([a, a, b], 1), np.stack([b, b, b], 1), base[::5], np.repeat(free[:5, None], 3, 1), [[free[5], free[5], free[6]]]])
    mixed = np.concatenate([base, extra]).astype(np.int32)
    out["degenerate"] = (mixed[np.random.default_rng(4).permutation(len(mixed))], nv, 5000 + 6)
    return out


LATTICE_SHAPE = (29, 33, 40)            # (nz, ny, nx)
PERCOLATION = {6: 0.35, 14: 0.20, 26: 0.12}


def percolation_mask(connectivity):
    """Random occupancy near the percolation threshold of the connectivity: many clusters and one tortuous large one."""
    return np.random.default_rng(7).random(LATTICE_SHAPE) < PERCOLATION[connectivity]


def serpentine(n=32):
    """One long path folded into the n^3 lattice (n even): in every even z plane the even y rows are full and joined alternately at their right and left ends by
    one point of the odd row between them; consecutive even planes are joined by one point of the odd plane between them, alternately at the path's end and at
    its start.  One component under 6, 14 and 26, some n^3 / 4 points long."""
    m = np.zeros((n, n, n), bool)
    rows = n // 2
    end = (2 * (rows - 1), 0 if rows % 2 == 0 else n - 1)            # (y, x) where a plane's path ends; it starts at (0, 0)
    for z in range(0, n, 2):
        for r in range(rows):
            m[z, 2 * r, :] = True
            if r + 1 < rows:
                m[z, 2 * r + 1, n - 1 if r % 2 == 0 else 0] = True
        if z + 2 < n:
            y, x = end if (z // 2) % 2 == 0 else (0, 0)
            m[z + 1, y, x] = True
    return m


def wrap_mask(nx, ny, nz):
    """Pairs of points that are neighbours in memory (consecutive flat indices) and never on the lattice: (nx-1, j, k) with (0, j+1, k) across a row end, and
    (nx-1, ny-1, k) with (0, 0, k+1) across a plane end.  j and k step by 2 (j from 2) so that no two set points are neighbours under 26 either: every point is a
    component of its own.  (With every j and k the points (nx-1, j, k) would form a connected sheet.)"""
    m = np.zeros((nz, ny, nx), bool)
    m[0::2, 2:ny - 1:2, nx - 1] = True
    m[0::2, 3:ny:2, 0] = True
    m[0:nz - 1:2, ny - 1, nx - 1] = True
    m[1::2, 0, 0] = True
    return m


def lattice_masks():
    """name -> mask [nz, ny, nx] bool: every lattice input of the GPU tests."""
    nz, ny, nx = LATTICE_SHAPE
    out = {f"percolation{c}": percolation_mask(c) for c in (6, 14, 26)}
    out["serpentine"] = serpentine(32)
    out["ones"] = np.ones((5, 6, 7), bool)
    out["zeros"] = np.zeros((5, 6, 7), bool)
    out["row"] = np.random.default_rng(1).random((1, 1, 64)) < 0.7
    out["column"] = np.array([1, 1, 0, 1, 1], bool).reshape(5, 1, 1)
    out["wrap"] = wrap_mask(nx, ny, nz)
    return out


def known_field():
    """Two balls and a torus on the 33^3 lattice over [-1.5, 1.5]^3, formed in float64 and rounded to fp32; the level is 0."""
    from mesh_ref import lattice_points
    box = np.array([-1.5, -1.5, -1.5, 1.5, 1.5, 1.5], np.float32)
    p = lattice_points(box, 33, 33, 33).astype(np.float64)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    f = np.maximum.reduce([0.35 - np.linalg.norm(p - [-.8, -.8, -.8], axis=-1), 0.22 - np.linalg.norm(p - [.9, .9, -.7], axis=-1),
                           0.18 - np.hypot(np.hypot(x - .2, y + .1) - .6, z - .6)])
    return f.astype(np.float32), box
