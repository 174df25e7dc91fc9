"""Mesh simplification without a GPU: the definition (tests/simplify_ref.py, the numpy restatement the GPU tests compare nrf_mesh_simplify_count / _emit with bit
for bit) pinned on subdivided spheres -- closed surfaces, Euler characteristic 2, the face counts of the prototype, the orientation rule on hand-made coincident
faces, invariance under permutations of the input -- and the header, the binding, the constants, the workspace sizes and every refusal of the three entries (they
come before any device call)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import raster_ref as R
import simplify_ref as S
import tsdf_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
INVALID_ARG, WORKSPACE = 1, 4
LEVELS = (3, 4, 5)
GRIDS = (2, 3, 4, 6, 8, 12, 16, 24, 32)


@functools.lru_cache(maxsize=None)
def sphere(level):
    return R.octa_sphere(T.SPHERE["centre"], T.SPHERE["radius"], level)


@functools.lru_cache(maxsize=None)
def simplified(level, n, position=S.POS_MEAN):
    verts, faces = sphere(level)
    return S.simplify(verts, faces, S.mesh_box(verts), (n, n, n), position)


def test_header_binding_and_constants_agree():
    from nerfpp_amd import _lib, mesh
    hdr = open(os.path.join(ROOT, "include", "nerfpp_hip.h")).read()
    for name, value in (("MAX_DIM", 1024), ("POS_MEAN", 0), ("POS_MEMBER", 1)):
        m = re.search(rf"#define\s+NRF_SIMPLIFY_{name}\s+(\d+)", hdr)
        assert m and int(m[1]) == value == getattr(mesh, "SIMPLIFY_" + name) == getattr(S, ("SIMPLIFY_" if name == "MAX_DIM" else "") + name), name
    assert re.search(r"#define\s+NRF_SIMPLIFY_MAX_CELLS\s+\(1 << 27\)", hdr) and mesh.SIMPLIFY_MAX_CELLS == S.SIMPLIFY_MAX_CELLS == 1 << 27
    want = [("nrf_mesh_simplify_workspace_bytes", ("z", "lliii")), ("nrf_mesh_simplify_count", ("i", "plplpiiippppzp")),
            ("nrf_mesh_simplify_emit", ("i", "plplpiiiillppppppzp"))]
    at = _lib.SYMBOLS.index("nrf_distance_stats")
    assert _lib.SYMBOLS[at + 1:at + 5] == [n for n, _ in want] + ["nrf_ssim_window"], "between nrf_distance_stats and nrf_ssim_window, in the header's order"
    assert hdr.index("nrf_distance_stats(") < hdr.index("Mesh simplification") < hdr.index("nrf_mesh_simplify_workspace_bytes(") < hdr.index("Image metrics")
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    for name, sig in want:
        assert _lib.SIGNATURES[name] == sig and hasattr(lib, name) and re.search(rf"NRF_API (size_t|int) {name}\(", hdr), name
    for name in ("SimplifyMesh", "SimplifyToFaces"):
        assert callable(getattr(mesh, name)), name
    import inspect
    assert inspect.signature(mesh.ExtractMesh).parameters["simplify_cell"].default is None
    assert "monotone" in mesh.SimplifyToFaces.__doc__


def test_workspace_sizes_and_refusals_need_no_gpu():
    """Every bad argument of the header is refused before anything touches the device, so the whole list is checked here over pointers that are never dereferenced."""
    from nerfpp_amd import _lib
    lib = _lib.lib()
    fake = C.c_void_p(256)
    big = 1 << 40
    box = np.array([0, 0, 0, 1, 1, 1], F32)
    pb = lambda a: a.ctypes.data_as(C.c_void_p)
    nan, inf = float("nan"), float("inf")

    def refused(name, status, fn, cases):
        for kw in cases:
            assert fn(**kw) == status, (name, kw)
            assert lib.nrf_last_error().startswith(name.encode()), (kw, lib.nrf_last_error())

    size = lib.nrf_mesh_simplify_workspace_bytes
    # per vertex a cell and a mark, per face a triple and a slot, 16-byte slots for at least twice the faces, per cell an id, per possible output vertex 36 bytes
    assert size(258, 512, 4, 5, 6) >= 258 * 5 + 512 * 16 + 1024 * 16 + 120 * 4 + 120 * 36 and size(0, 0, 1, 1, 1) > 0
    assert size(258, 512, 4, 5, 6) == size(258, 512, 6, 5, 4) and size(258, 513, 4, 5, 6) >= size(258, 512, 4, 5, 6) + 1024 * 16
    for bad in ((-1, 1, 1, 1, 1), (1, -1, 1, 1, 1), (2 ** 31, 1, 1, 1, 1), (1, 2 ** 31, 1, 1, 1), (1, 1, 0, 1, 1), (1, 1, 1, 0, 1), (1, 1, 1, 1, 0), (1, 1, 1025, 1, 1),
                (1, 1, 1, 1025, 1), (1, 1, 1, 1, 1025), (1, 1, 1024, 1024, 129), (1, 1, -1, 1, 1)):
        assert size(*bad) == 0, bad
    assert size(1, 1, 1024, 1024, 128) > 2 ** 29 and size(1, 1, 1024, 1, 1) > 0 and size(2 ** 31 - 1, 2 ** 31 - 1, 1, 1, 1) > 2 ** 36

    boxes = [np.array(b, F32) for b in ([0, 0, 0, 1, 0, 1], [0, 0, 0, 1, 1, -1], [0, nan, 0, 1, 1, 1], [0, 0, 0, inf, 1, 1], [-inf, 0, 0, 1, 1, 1],
                                        [-3e38, 0, 0, 3e38, 1, 1], [0, 0, 0, 1, 1e-42, 1])]
    shapes = [dict(nv=-1), dict(nv=2 ** 31), dict(nf=-1), dict(nf=2 ** 31), dict(nx=0), dict(ny=0), dict(nz=-1), dict(nx=1025), dict(ny=1025), dict(nz=1025),
              dict(nx=1024, ny=1024, nz=129), dict(verts=None), dict(faces=None), dict(b=None), dict(ws=None), dict(ws=C.c_void_p(260))] + [dict(b=pb(b)) for b in boxes]

    def count(verts=fake, nv=4, faces=fake, nf=2, b=pb(box), nx=2, ny=2, nz=2, n_v=fake, n_f=fake, ws=fake, ws_bytes=big):
        return lib.nrf_mesh_simplify_count(verts, nv, faces, nf, b, nx, ny, nz, n_v, n_f, None, ws, ws_bytes, None)

    refused("nrf_mesh_simplify_count", INVALID_ARG, count, shapes + [dict(n_v=None), dict(n_f=None)])
    refused("nrf_mesh_simplify_count", WORKSPACE, count, [dict(ws_bytes=size(4, 2, 2, 2, 2) - 1), dict(ws_bytes=0)])

    def emit(verts=fake, nv=4, faces=fake, nf=2, b=pb(box), nx=2, ny=2, nz=2, pos=0, ov=3, of=1, out_v=fake, out_f=fake, ws=fake, ws_bytes=big):
        return lib.nrf_mesh_simplify_emit(verts, nv, faces, nf, b, nx, ny, nz, pos, ov, of, out_v, out_f, None, None, None, ws, ws_bytes, None)

    refused("nrf_mesh_simplify_emit", INVALID_ARG, emit, shapes + [dict(pos=-1), dict(pos=2), dict(ov=-1), dict(of=-1), dict(ov=5), dict(of=3), dict(ov=2, nx=1, ny=1, nz=1),
                                                                   dict(out_v=None), dict(out_f=None)])
    refused("nrf_mesh_simplify_emit", WORKSPACE, emit, [dict(ws_bytes=size(4, 2, 2, 2, 2) - 1), dict(ws_bytes=0)])


@pytest.mark.parametrize("level", LEVELS)
def test_spheres_stay_closed_surfaces(level):
    """What the orientation rule was seen to hold on these inputs: a closed surface of Euler characteristic 2 at every grid (vertex clustering does not promise it in
    general)"""
    verts, faces = sphere(level)
    empty = simplified(level, 1)
    assert empty["n_verts"] == 0 and empty["n_faces"] == 0 and empty["stats"].tolist() == [0, 0, len(faces), 0] and (empty["cluster"] == -1).all()
    for n in GRIDS:
        r = simplified(level, n)
        f = r["faces"]
        edges, use = S.edge_use(f)
        print(f"level {level}, n {n}: {r['n_verts']} vertices, {r['n_faces']} faces, stats {r['stats'].tolist()}")
        assert (use == 2).all(), (n, "every undirected edge is used by exactly two faces")
        assert r["n_verts"] - len(edges) + r["n_faces"] == 2, n
        assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all()
        assert len(np.unique(np.sort(f, axis=1), axis=0)) == len(f), "no two faces share a sorted triple"
        assert np.array_equal(np.unique(f), np.arange(r["n_verts"])), "every output vertex is used by some face"
        assert (np.diff(r["cells"]) > 0).all(), "output vertices ascend in cell index"
        assert r["stats"].sum() + r["n_faces"] == len(faces) and len(r["verts"]) == r["n_verts"] == len(r["rep"]) and len(f) == r["n_faces"] == len(r["face_src"])
        assert (np.diff(r["face_src"]) > 0).all()
    for n in (12, 16, 24, 32):
        if level == 3:
            r = simplified(3, n)
            assert (r["n_verts"], r["n_faces"]) == (258, 512) and r["stats"].tolist() == [0, 0, 0, 0]


def test_face_counts_of_the_prototype():
    for level, n, nv, nf, removed in ((4, 6, 116, 228, 48), (5, 12, 560, 1116, 48), (5, 8, 272, 540, 0)):
        r = simplified(level, n)
        assert (r["n_verts"], r["n_faces"], int(r["stats"][3])) == (nv, nf, removed), (level, n)


@pytest.mark.parametrize("level", LEVELS)
def test_positions_stay_in_their_cells(level):
    """Mean mode: tm lies in [c, c + 1] up to its one rounding, h carries two, the product and the sum one each, every one <= 2^-24 relative: the coordinate lies
    within the cell's interval widened by 2^-21 * max(|bmin|, |bmax|, bmax - bmin).  Member mode: the representative lies in the output vertex's own cell and its
    coordinates are copied exactly."""
    verts, _ = sphere(level)
    box = S.mesh_box(verts).astype(np.float64)
    for n in GRIDS:
        r = simplified(level, n)
        oc = np.stack([r["cells"] % n, (r["cells"] // n) % n, r["cells"] // (n * n)], axis=1)
        h = (box[3:] - box[:3]) / n
        slack = 2.0 ** -21 * np.maximum(np.maximum(np.abs(box[:3]), np.abs(box[3:])), box[3:] - box[:3])
        lo, hi = box[:3] + oc * h - slack, box[:3] + (oc + 1) * h + slack
        p = r["verts"].astype(np.float64)
        assert (p >= lo).all() and (p <= hi).all(), n
        cell, _, _ = S.vertex_cells(verts, box.astype(F32), (n, n, n))
        assert np.array_equal(cell[r["rep"]], r["cells"]), n
        m = simplified(level, n, S.POS_MEMBER)
        assert np.array_equal(m["rep"], r["rep"]) and np.array_equal(m["faces"], r["faces"]) and np.array_equal(m["verts"].view(np.uint32), verts[r["rep"]].view(np.uint32))
        assert np.array_equal(m["mean"].view(np.uint32), r["verts"].view(np.uint32))


def test_the_order_of_the_input_does_not_matter():
    verts, faces = sphere(4)
    box = S.mesh_box(verts)
    rng = np.random.default_rng(11)
    for n in (4, 6, 8, 16):
        want = simplified(4, n)
        perm = rng.permutation(len(verts))          # new vertex k is old vertex perm[k]
        inv = np.argsort(perm)
        got = S.simplify(verts[perm], inv[faces].astype(np.int32), box, (n, n, n))
        assert np.array_equal(got["verts"].view(np.uint32), want["verts"].view(np.uint32)) and np.array_equal(got["faces"], want["faces"]), n
        assert np.array_equal(got["face_src"], want["face_src"]) and np.array_equal(got["stats"], want["stats"])
        fperm = rng.permutation(len(faces))
        got = S.simplify(verts, faces[fperm], box, (n, n, n))
        assert np.array_equal(got["verts"].view(np.uint32), want["verts"].view(np.uint32)), n
        # as oriented triangles: which of several coincident faces is the lowest changes with the order, and with it the corner the triple starts at
        rows = lambda f: sorted(tuple(np.roll(t, -int(np.argmin(t)))) for t in f.tolist())
        assert rows(got["faces"]) == rows(want["faces"]) and np.array_equal(got["stats"], want["stats"]), n


def test_coincident_faces_follow_their_net_orientation():
    """Six vertices, two per cell of a 3 x 1 x 1 grid: faces over (0, 2, 4) and (1, 3, 5) land on the same three cells"""
    verts = np.array([[0.1, 0.2, 0.5], [0.3, 0.8, 0.5], [1.2, 0.1, 0.5], [1.4, 0.6, 0.5], [2.5, 0.5, 0.1], [2.7, 0.5, 0.9]], F32)
    box, dims = np.array([0, 0, 0, 3, 1, 1], F32), (3, 1, 1)
    even, even2, odd, odd2 = (0, 2, 4), (3, 5, 1), (4, 2, 0), (1, 5, 3)

    def run(*faces):
        return S.simplify(verts, np.array(faces, np.int32), box, dims)
    r = run(even2, even)
    assert r["face_src"].tolist() == [0] and r["faces"].tolist() == [[1, 2, 0]] and r["stats"].tolist() == [0, 0, 0, 1], "same winding: the lower face"
    r = run(even, odd)
    assert r["n_faces"] == 0 and r["n_verts"] == 0 and r["stats"].tolist() == [0, 0, 0, 2] and (r["cluster"] == -1).all(), "opposite winding: none"
    r = run(odd, even, even2)
    assert r["face_src"].tolist() == [1] and r["faces"].tolist() == [[0, 1, 2]] and r["stats"].tolist() == [0, 0, 0, 2], "two even and one odd: the lowest even"
    r = run(odd, even, odd2)
    assert r["face_src"].tolist() == [0] and r["faces"].tolist() == [[2, 1, 0]], "two odd and one even: the lowest odd"
    # the mean is over the USED vertices of the cell: with face `even` alone, vertices 1, 3, 5 do not move it
    r = run(even)
    assert r["rep"].tolist() == [0, 2, 4] and np.abs(r["verts"] - verts[[0, 2, 4]]).max() < 2e-6 and r["cluster"].tolist() == [0, 0, 1, 1, 2, 2]
    r = run(even, (1, 1, 3))          # a collapsed face still makes its vertices members
    assert r["stats"].tolist() == [0, 0, 1, 0] and np.abs(r["verts"][:2] - 0.5 * (verts[[0, 2]] + verts[[1, 3]])).max() < 2e-6
    assert np.abs(r["verts"][2] - verts[4]).max() < 2e-6
    r = run(even, (0, 2, 6), (0, -1, 2))
    assert r["stats"].tolist() == [2, 0, 0, 0] and r["n_faces"] == 1
