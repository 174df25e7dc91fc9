"""numpy restatement of the mesh BVH (include/nerfpp_hip.h "Mesh BVH": nrf_mesh_bvh_build and the two pruning bounds of its queries): the classes, the mesh box, the
Morton codes and the stable order of the leaves, the tree as a TOP-DOWN recursion (split a range where the highest differing bit of its first and last key changes)
with the header's numbering, the boxes as exact minima and maxima, the layout of the caller-owned buffer, and the two bounds in one numpy fp32 operation per source
operation.  It knows nothing of Karras's bottom-up search or of refit passes.  Also the meshes the host and GPU tests share.  Imports nothing of the package."""
import numpy as np

import closest_ref as CR
import raster_ref as R
import raycast_ref as RR
import tsdf_ref as T

F32 = np.float32
MAGIC = 0x4e52464256483031
MAX_DEPTH = 64
CODE_INVALID = 1 << 30
NODE_BYTES = 64
RAY_MARGIN, RAY_MIN_SCALE = F32(2.0 ** -10), F32(2.0 ** -100)
INF = F32(np.inf)


# ---- the mesh box, the codes and the leaves ----
def image(x):
    """The unsigned image of a float whose order is the float's, -0 below +0"""
    u = np.ascontiguousarray(x, F32).view(np.uint32)
    return np.where(u >> np.uint32(31) != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unimage(u):
    u = np.asarray(u, np.uint32)
    return np.where(u >> np.uint32(31) != 0, u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32).view(F32)


def _min3(a, b, c):
    """Per component the smallest / largest of three floats in the image's order (what the device's fminf / fmaxf give for finite inputs)"""
    ia, ib, ic = image(a), image(b), image(c)
    return unimage(np.minimum(np.minimum(ia, ib), ic)), unimage(np.maximum(np.maximum(ia, ib), ic))


def axis_cell(c, lo, hi):
    """10 bits of one axis: c [...] against the mesh box's [lo, hi] (scalars)"""
    c = np.asarray(c, F32)
    with np.errstate(all="ignore"):
        e = F32(hi) - F32(lo)
        if not (e > 0 and e < INF):
            return np.zeros(c.shape, np.uint32)
        x = np.floor(((c - F32(lo)) / e) * F32(1024))
        assert x.dtype == F32
        x = np.where(np.isnan(x), F32(0), x)
        return np.minimum(np.maximum(x, F32(0)), F32(1023)).astype(np.uint32)


def _spread(v):
    v = v.astype(np.uint32)
    out = np.zeros_like(v)
    for k in range(10):
        out |= ((v >> np.uint32(k)) & np.uint32(1)) << np.uint32(3 * k)
    return out


def morton(c, lo, hi):
    """c [..., 3] f32 against the mesh box -> uint32 codes"""
    c = np.asarray(c, F32)
    return _spread(axis_cell(c[..., 0], lo[0], hi[0])) | (_spread(axis_cell(c[..., 1], lo[1], hi[1])) << np.uint32(1)) | \
        (_spread(axis_cell(c[..., 2], lo[2], hi[2])) << np.uint32(2))


def build(verts, faces):
    """-> dict(F, n_valid, lo, hi [3] f32 the mesh box, codes [F] in face order, leaf_face [F], sorted [F] the codes in leaf order, child [n_valid - 1, 2],
    parent [n_valid - 1], range [n_valid - 1, 2] the leaves a node covers, box [n_valid - 1, 12] f32 (lo0, hi0, lo1, hi1), leaf_lo / leaf_hi [n_valid, 3], height,
    stats [4])"""
    cls, a, b, c = CR.face_classes(verts, faces)
    F = len(cls)
    valid = cls == 0
    nv = int(valid.sum())
    flo, fhi = _min3(a, b, c)          # [F, 3]
    if nv:
        lo = unimage(image(flo[valid]).min(0))
        hi = unimage(image(fhi[valid]).max(0))
    else:
        lo, hi = np.full(3, np.inf, F32), np.full(3, -np.inf, F32)
    with np.errstate(all="ignore"):
        ctr = flo * F32(0.5) + fhi * F32(0.5)
    assert ctr.dtype == F32
    codes = np.where(valid, morton(ctr, lo, hi) if F else np.zeros(0, np.uint32), np.uint32(CODE_INVALID)).astype(np.uint32)
    leaf_face = np.argsort(codes, kind="stable").astype(np.int32)
    srt = codes[leaf_face]
    keys = (srt[:nv].astype(np.uint64) << np.uint64(32)) | leaf_face[:nv].astype(np.uint64)
    assert (keys[1:] > keys[:-1]).all(), "the keys of the leaves ascend strictly"
    n_int = max(nv - 1, 0)
    child = np.zeros((n_int, 2), np.int32)
    parent = np.full(n_int, -2, np.int32)
    rng = np.zeros((n_int, 2), np.int64)
    depth = np.zeros(n_int, np.int64)
    height = 0
    if n_int:
        parent[0] = -1
        todo = [(0, 0, nv - 1, 0)]          # node, first leaf, last leaf, depth
        while todo:
            i, l, r, dep = todo.pop()
            assert i in (l, r), "a node's index is an end of its range"
            rng[i], depth[i] = (l, r), dep
            height = max(height, dep + 1)          # its children lie one edge deeper
            x = int(keys[l]) ^ int(keys[r])
            bit = x.bit_length() - 1          # the highest differing bit; the keys of [l, r] agree above it
            first_set = l + int(np.searchsorted((keys[l:r + 1] >> np.uint64(bit)) & np.uint64(1), 1))
            s = first_set - 1
            assert l <= s < r
            for k, (cl, cr, ci) in enumerate(((l, s, s), (s + 1, r, s + 1))):
                if cl == cr:
                    child[i, k] = -(cl + 1)
                else:
                    child[i, k] = ci
                    parent[ci] = i
                    todo.append((ci, cl, cr, dep + 1))
    leaf_lo, leaf_hi = flo[leaf_face[:nv]], fhi[leaf_face[:nv]]
    box = np.zeros((n_int, 12), F32)
    for i in range(n_int):
        for k in range(2):
            ch = child[i, k]
            l, r = (-(ch + 1), -(ch + 1)) if ch < 0 else rng[ch]
            box[i, 6 * k:6 * k + 3] = unimage(image(leaf_lo[l:r + 1]).min(0))
            box[i, 6 * k + 3:6 * k + 6] = unimage(image(leaf_hi[l:r + 1]).max(0))
    stats = np.array([0, (cls == 1).sum(), (cls == 2).sum(), 0], np.uint32)
    return dict(F=F, n_valid=nv, lo=lo, hi=hi, codes=codes, leaf_face=leaf_face, sorted=srt, child=child, parent=parent, range=rng, box=box, leaf_lo=leaf_lo,
                leaf_hi=leaf_hi, height=height, stats=stats)


# ---- the buffer ----
def _up(x):
    return (x + 255) // 256 * 256


def layout(F):
    """-> (offset of leaf_face, offset of the nodes, bytes): every piece starts at a multiple of 256"""
    at_leaf = 256
    at_node = _up(at_leaf + 4 * F)
    return at_leaf, at_node, _up(at_node + NODE_BYTES * max(F - 1, 0))


def parse(buf, F):
    """The bytes of a built buffer (uint8 [nrf_mesh_bvh_bytes(F)]) -> the pieces of build()'s dict that the buffer holds, plus head [8] int64 and rest: whether
    everything the tree does not use is zero"""
    buf = np.ascontiguousarray(buf, np.uint8)
    at_leaf, at_node, total = layout(F)
    assert len(buf) == total, (len(buf), total)
    head = buf[:64].view(np.int64).copy()
    nv = int(head[2])
    box_words = head[3:6].view(np.uint64)
    lo = (box_words & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(F32)
    hi = (box_words >> np.uint64(32)).astype(np.uint32).view(F32)
    leaf_face = buf[at_leaf:at_leaf + 4 * F].view(np.int32).copy()
    nodes = buf[at_node:at_node + NODE_BYTES * max(F - 1, 0)].view(np.uint32).reshape(-1, 16)
    n_int = max(nv - 1, 0)
    used = nodes[:n_int]
    rest = not buf[64:at_leaf].any() and not buf[at_leaf + 4 * F:at_node].any() and not nodes[n_int:].any() and not used[:, 15].any() and not head[6:].any() and \
        not buf[at_node + NODE_BYTES * max(F - 1, 0):].any()
    return dict(F=int(head[1]), n_valid=nv, lo=lo, hi=hi, leaf_face=leaf_face, child=used[:, 12:14].view(np.int32).copy(), parent=used[:, 14].view(np.int32).copy(),
                box=used[:, :12].view(F32).copy(), head=head, rest=rest)


def same_tree(got, want):
    """A parsed buffer against build()'s tree, node for node -> a list of what differs (empty: equal)"""
    bad = []
    if got["head"][0] != MAGIC or got["F"] != want["F"] or got["n_valid"] != want["n_valid"]:
        bad.append(f"head {got['head'][:3]}")
    for name in ("lo", "hi", "box"):
        if not np.array_equal(np.ascontiguousarray(got[name], F32).view(np.uint32), np.ascontiguousarray(want[name], F32).view(np.uint32)):
            bad.append(name)
    for name in ("leaf_face", "child", "parent"):
        if not np.array_equal(got[name], want[name]):
            bad.append(name)
    if not got["rest"]:
        bad.append("unused bytes are not zero")
    return bad


def check_invariants(tree, verts, faces):
    """What every tree must satisfy, on any tree given as build()'s or parse()'s dict -> its height (edges from the root to the deepest leaf)"""
    cls, a, b, c = CR.face_classes(verts, faces)
    nv, F = tree["n_valid"], len(cls)
    assert nv == int((cls == 0).sum())
    assert sorted(tree["leaf_face"].tolist()) == list(range(F)), "the leaves and the faces behind them are a permutation of all faces"
    assert sorted(tree["leaf_face"][:nv].tolist()) == np.flatnonzero(cls == 0).tolist(), "the leaves are the valid faces"
    flo, fhi = _min3(a, b, c)
    if nv:
        assert np.array_equal(image(tree["lo"]), image(flo[cls == 0]).min(0)) and np.array_equal(image(tree["hi"]), image(fhi[cls == 0]).max(0)), "the mesh box"
    else:
        assert (tree["lo"] == np.inf).all() and (tree["hi"] == -np.inf).all()
    if nv < 2:
        assert len(tree["child"]) == 0
        return 0
    child, parent, box = tree["child"], tree["parent"], tree["box"]
    assert len(child) == nv - 1 and parent[0] == -1
    seen_leaf, seen_node = np.zeros(nv, int), np.zeros(nv - 1, int)
    lo_of, hi_of, height = {}, {}, 0
    order, todo = [], [(0, 0)]
    while todo:          # parents before children
        i, dep = todo.pop()
        order.append(i)
        height = max(height, dep + 1)
        for k in range(2):
            ch = int(child[i, k])
            if ch < 0:
                assert 0 <= -(ch + 1) < nv
                seen_leaf[-(ch + 1)] += 1
            else:
                assert 0 < ch < nv - 1 and parent[ch] == i, "parent and child agree"
                seen_node[ch] += 1
                todo.append((ch, dep + 1))
    assert (seen_leaf == 1).all() and (seen_node[1:] == 1).all() and seen_node[0] == 0, "every leaf and every node but the root is the child of exactly one node"
    leaf_lo, leaf_hi = image(flo[tree["leaf_face"][:nv]]), image(fhi[tree["leaf_face"][:nv]])
    for i in reversed(order):          # children before parents: the exact box of what lies under each child
        for k in range(2):
            ch = int(child[i, k])
            l, h = (leaf_lo[-(ch + 1)], leaf_hi[-(ch + 1)]) if ch < 0 else (lo_of[ch], hi_of[ch])
            assert np.array_equal(image(box[i, 6 * k:6 * k + 3]), l) and np.array_equal(image(box[i, 6 * k + 3:6 * k + 6]), h), f"the box of child {k} of node {i}"
        lo_of[i] = np.minimum(image(box[i, 0:3]), image(box[i, 6:9]))
        hi_of[i] = np.maximum(image(box[i, 3:6]), image(box[i, 9:12]))
    assert np.array_equal(lo_of[0], image(tree["lo"])) and np.array_equal(hi_of[0], image(tree["hi"])), "the root covers the mesh box"
    assert height <= 62
    return height


# ---- the two bounds ----
def box_d2(q, lo, hi):
    """q [n, 3], lo / hi [3] -> b2 [n] f32 in the header's order"""
    q, lo, hi = np.asarray(q, F32), np.asarray(lo, F32), np.asarray(hi, F32)
    with np.errstate(all="ignore"):
        g = np.where(q < lo, lo - q, np.where(q > hi, q - hi, F32(0))).astype(F32)
        b2 = (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]
    assert b2.dtype == F32
    return b2


def box_ray(o, d, rlo, rhi, lo, hi):
    """The node test: o, d [n, 3], rlo, rhi [n] the rays' ranges, lo / hi [3] the box -> (nonempty [n], t_in [n], t_out [n]) f32"""
    o, d, lo, hi = np.asarray(o, F32), np.asarray(d, F32), np.asarray(lo, F32), np.asarray(hi, F32)
    with np.errstate(all="ignore"):
        M = np.maximum(np.abs(o).max(-1), max(np.abs(lo).max(), np.abs(hi).max())).astype(F32)
        m = np.where(M >= RAY_MIN_SCALE, RAY_MARGIN * M, INF).astype(F32)
        wlo, whi = lo[None] - m[:, None], hi[None] + m[:, None]
        zero = d == 0
        dd = np.where(zero, F32(1), d)
        ta, tb = (wlo - o) / dd, (whi - o) / dd
        ta, tb = np.where(ta > tb, tb, ta), np.where(ta > tb, ta, tb)
        outside = (zero & ((o < wlo) | (o > whi))).any(-1)
        ta, tb = np.where(zero, -INF, ta), np.where(zero, INF, tb)
        t_in = np.maximum(np.asarray(rlo, F32), ta.max(-1))
        t_out = np.minimum(np.asarray(rhi, F32), tb.min(-1))
    assert t_in.dtype == F32 and t_out.dtype == F32 and wlo.dtype == F32
    return ~outside & (t_in <= t_out), t_in, t_out


# ---- the meshes of the tests ----
def sphere(level):
    return R.octa_sphere(T.SPHERE["centre"], T.SPHERE["radius"], level)


def soup(n, seed=0, size=0.2):
    """n small triangles strewn through the unit cube, no shared vertices"""
    rng = np.random.default_rng(seed)
    v = (rng.uniform(-1, 1, (n, 1, 3)) + rng.uniform(-size, size, (n, 3, 3))).astype(F32).reshape(-1, 3)
    return v, np.arange(3 * n, dtype=np.int32).reshape(-1, 3)


def meshes():
    """name -> (verts, faces): the face counts around the block size, the 1 280-face icosphere, 300 copies of one face, a flat mesh, the three classes of invalid
    faces mixed in and alone, and one huge face beside tiny ones"""
    import align_ref as A
    out = {f"soup{n}": soup(n, seed=n) for n in (0, 1, 2, 3, 255, 256, 257)}
    v, f = A.ico_sphere(3)
    out["ico1280"] = (np.asarray(v, F32) * F32(0.7) + np.array([0.1, -0.15, 0.2], F32), np.asarray(f, np.int32))
    v, f = soup(1, seed=9)
    out["copies300"] = (v, np.repeat(f, 300, axis=0))
    v, f = soup(200, seed=4)
    v[:, 2] = F32(0.25)
    out["flat"] = (v, f)
    v, f = sphere(2)
    v, f = v.copy(), f.copy()
    f[5] = (0, 1, len(v))          # bad
    f[17] = (-1, 2, 3)             # bad
    v = np.concatenate([v, np.array([[np.nan, 0, 0], [0, np.inf, 0]], F32)])
    f[40] = (0, 1, len(v) - 2)     # non-finite
    f[99] = (len(v) - 1, 2, 3)     # non-finite
    out["mixed"] = (v, f)
    out["invalid_only"] = (v, np.array([[0, 1, len(v)], [len(v) - 1, 2, 3], [len(v) - 2, 0, 1]], np.int32))
    sv, sf = sphere(2)
    out["floor"] = RR.floor_mesh(sv, sf, F32(-0.6), F32(50.0))
    return out
