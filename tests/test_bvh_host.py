"""The mesh BVH without a GPU: the library exports and declares every new entry; the tree of tests/bvh_ref.py satisfies the invariants of a bounding-volume
hierarchy on every mesh of the tests; and the two pruning arguments of the header ("Mesh BVH": WHY IT IS EXACT, WHY THE TRAVERSAL CANNOT MISS) hold as censuses in
fp32 numpy over every (query or ray, node, face under the node) triple, with ZERO violations allowed: the cap is a condition of the proof, not a measurement."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import bvh_ref as B
import closest_ref as CR
import raycast_ref as RR

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"nrf_sort_workspace_bytes": ("z", "l"), "nrf_sort_pairs_u32": ("i", "ppliipppzp"), "nrf_mesh_bvh_bytes": ("z", "l"), "nrf_mesh_bvh_workspace_bytes": ("z", "l"),
           "nrf_mesh_bvh_build": ("i", "plplpzppzp"), "nrf_bvh_query_workspace_bytes": ("z", "l"), "nrf_bvh_closest_on_mesh": ("i", "plplplpzpfppppppzp"),
           "nrf_bvh_ray_cast_mesh": ("i", "pliplplpzpiipppppppzp"), "nrf_bvh_point_codes": ("i", "plipzlpp")}


def test_the_library_exports_and_declares_every_entry():
    from nerfpp_amd import _lib, geometry
    hdr = open(os.path.join(ROOT, "include", "nerfpp_hip.h")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    for name, sig in ENTRIES.items():
        assert _lib.SIGNATURES[name] == sig and hasattr(lib, name) and re.search(rf"NRF_API (size_t|int) {name}\(", hdr), name
    assert int(re.search(r"#define NRF_BVH_MAX_DEPTH (\d+)", hdr)[1]) == B.MAX_DEPTH == geometry.BVH_MAX_DEPTH
    assert hasattr(geometry, "MeshBVH")
    lib.nrf_mesh_bvh_bytes.restype = lib.nrf_mesh_bvh_workspace_bytes.restype = lib.nrf_sort_workspace_bytes.restype = C.c_size_t
    lib.nrf_mesh_bvh_bytes.argtypes = lib.nrf_mesh_bvh_workspace_bytes.argtypes = lib.nrf_sort_workspace_bytes.argtypes = [C.c_int64]
    for F in (0, 1, 2, 3, 255, 256, 257, 1280, 11_000_000):          # the sizes are pure functions of F, and the layout is the restatement's
        assert lib.nrf_mesh_bvh_bytes(F) == B.layout(F)[2], F
        assert lib.nrf_mesh_bvh_workspace_bytes(F) > 0 and lib.nrf_sort_workspace_bytes(F) > 0
    assert lib.nrf_mesh_bvh_bytes(-1) == 0 and lib.nrf_mesh_bvh_bytes(1 << 31) == 0 and lib.nrf_sort_workspace_bytes(1 << 31) == 0


@functools.lru_cache(maxsize=None)
def meshes():
    return B.meshes()


@pytest.mark.parametrize("name", ["soup0", "soup1", "soup2", "soup3", "soup255", "soup256", "soup257", "ico1280", "copies300", "flat", "mixed", "invalid_only", "floor"])
def test_the_restated_tree_is_a_bounding_volume_hierarchy(name):
    verts, faces = meshes()[name]
    tree = B.build(verts, faces)
    cls = CR.face_classes(verts, faces)[0]
    assert tree["stats"].tolist() == [0, int((cls == 1).sum()), int((cls == 2).sum()), 0]
    height = B.check_invariants(tree, verts, faces)
    assert height == tree["height"] <= 62
    assert (tree["sorted"][:tree["n_valid"]] < B.CODE_INVALID).all() and (tree["sorted"][tree["n_valid"]:] == B.CODE_INVALID).all()
    if name == "copies300":
        assert tree["n_valid"] == 300 and len(set(tree["sorted"].tolist())) == 1 and np.array_equal(tree["leaf_face"], np.arange(300)), "equal codes keep the face order"
    if name == "flat":
        assert tree["lo"][2] == tree["hi"][2] and ((tree["sorted"] >> 2) & 0x9249249 == 0).all(), "an axis of zero extent gives cell 0"
    if name == "mixed":
        assert tree["n_valid"] == len(faces) - 4 and sorted(tree["leaf_face"][-4:].tolist()) == [5, 17, 40, 99]
    if name == "invalid_only":
        assert tree["n_valid"] == 0 and (tree["lo"] == np.inf).all()


def test_the_buffer_round_trips_through_the_layout():
    """parse() reads back what a writer of the stated layout wrote"""
    verts, faces = meshes()["mixed"]
    tree = B.build(verts, faces)
    F = tree["F"]
    at_leaf, at_node, total = B.layout(F)
    buf = np.zeros(total, np.uint8)
    head = np.zeros(8, np.int64)
    head[0], head[1], head[2] = B.MAGIC, F, tree["n_valid"]
    head[3:6] = (tree["lo"].view(np.uint32).astype(np.uint64) | (tree["hi"].view(np.uint32).astype(np.uint64) << np.uint64(32))).view(np.int64)
    buf[:64] = head.view(np.uint8)
    buf[at_leaf:at_leaf + 4 * F] = tree["leaf_face"].view(np.uint8)
    nodes = np.zeros((tree["n_valid"] - 1, 16), np.uint32)
    nodes[:, :12] = tree["box"].view(np.uint32)
    nodes[:, 12:14] = tree["child"].view(np.uint32)
    nodes[:, 14] = tree["parent"].view(np.uint32)
    buf[at_node:at_node + nodes.nbytes] = nodes.reshape(-1).view(np.uint8)
    got = B.parse(buf, F)
    assert B.same_tree(got, tree) == []
    assert B.check_invariants(got, verts, faces) == tree["height"]
    buf[at_node + nodes.nbytes] = 1
    assert B.same_tree(B.parse(buf, F), tree) == ["unused bytes are not zero"]


def under(tree, i, k):
    """The sorted positions under child k of node i"""
    ch = int(tree["child"][i, k])
    return (-(ch + 1), -(ch + 1)) if ch < 0 else tuple(tree["range"][ch])


@pytest.mark.parametrize("level", [2, 3])
def test_census_the_box_distance_never_exceeds_a_distance_to_a_face_under_the_node(level):
    """b2 <= d2, as floats, for every (query, node, face under the node): queries of every kind around the mesh, and 100 and 1e6 units away"""
    verts, faces = B.sphere(level)
    tree = B.build(verts, faces)
    rng = np.random.default_rng(level)
    unit = rng.standard_normal((200, 3))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    q = np.concatenate([CR.mesh_queries(verts, faces, 10 + level), (unit[:100] * 100).astype(F32), (unit[100:] * 1e6).astype(F32),
                        np.array([[3e19, 0, 0], [-3e19, 3e19, 3e19], [3.0e38, -3.0e38, 3.0e38]], F32)])          # d2 overflows to +inf: b2 may too, never beyond
    q = q[np.isfinite(q).all(-1)]
    a, b, c = (verts[faces[:, k]] for k in range(3))
    d2 = np.concatenate([CR.closest_on_triangle(q[s:s + 256, None, :], a[None], b[None], c[None])["d2"] for s in range(0, len(q), 256)])
    d2 = d2[:, tree["leaf_face"]]          # in leaf order
    triples = violations = 0
    for i in range(tree["n_valid"] - 1):
        for k in range(2):
            l, r = under(tree, i, k)
            b2 = B.box_d2(q, tree["box"][i, 6 * k:6 * k + 3], tree["box"][i, 6 * k + 3:6 * k + 6])
            sub = d2[:, l:r + 1]
            with np.errstate(invalid="ignore"):
                ok = (b2[:, None] <= sub) | np.isnan(sub)          # a NaN d2 never wins: excluded
            triples += sub.size
            violations += int((~ok).sum())
    assert triples > 5 * len(q) * len(faces) and np.isinf(d2).any()
    assert violations == 0, f"{violations} of {triples} triples have a box bound above the distance"


def ray_sets(verts, faces, seed):
    """RR.mesh_rays, rays with a zero direction axis and in a face's plane among them, plus origins 1e4 units away aimed at the mesh and far = +inf"""
    rays, kinds = RR.mesh_rays(verts, faces, seed)
    rng = np.random.default_rng(seed)
    unit = rng.standard_normal((200, 3))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    cen = verts.mean(0).astype(np.float64)
    o = cen + unit * 1e4
    target = verts[rng.integers(0, len(verts), 200)].astype(np.float64) * 0.5 + cen * 0.5
    far = RR.pack(o, target - o)          # far = +inf
    assert np.isinf(rays[kinds["outside"], 7]).all() and (rays[kinds["zero"], 3:6] == 0).any(-1).all()
    return np.concatenate([rays, far]).astype(F32)


@pytest.mark.parametrize("shift", [0.0, 100.0])
def test_census_every_accepted_candidate_lies_inside_the_interval_of_every_ancestor(shift):
    """t_in <= t <= t_out for all ancestors of the face of every candidate RR.candidate accepts; a box test that calls the interval empty is a violation too"""
    verts, faces = B.sphere(3)
    verts = (verts + F32(shift)).astype(F32)
    tree = B.build(verts, faces)
    rays = ray_sets(verts, faces, 3 + int(shift))
    o, d, rlo, rhi, valid = RR.ray_parts(rays)
    o, d, rlo, rhi = o[valid], d[valid], rlo[valid], rhi[valid]
    a, b, c = (verts[faces[tree["leaf_face"], k]] for k in range(3))          # in leaf order
    ok, t = [], []
    for s in range(0, len(o), 256):
        r = RR.candidate(o[s:s + 256, None, :], d[s:s + 256, None, :], rlo[s:s + 256, None], rhi[s:s + 256, None], a[None], b[None], c[None])
        ok.append(r["ok"])
        t.append(r["t"])
    ok, t = np.concatenate(ok), np.concatenate(t)
    assert ok.sum() > 1000 and (ok.sum(1) == 0).any()
    checked = violations = 0
    for i in range(tree["n_valid"] - 1):
        for k in range(2):
            l, r = under(tree, i, k)
            inside, t_in, t_out = B.box_ray(o, d, rlo, rhi, tree["box"][i, 6 * k:6 * k + 3], tree["box"][i, 6 * k + 3:6 * k + 6])
            sub_ok, sub_t = ok[:, l:r + 1], t[:, l:r + 1]
            good = inside[:, None] & (t_in[:, None] <= sub_t) & (sub_t <= t_out[:, None])
            checked += int(sub_ok.sum())
            violations += int((sub_ok & ~good).sum())
    assert checked > 5 * ok.sum()
    assert violations == 0, f"{violations} of {checked} (candidate, ancestor) pairs lie outside the ancestor's interval"


def test_the_node_test_at_the_scale_of_the_denormals_visits_everything():
    o = np.array([[1e-35, 0, 0]], F32)
    d = np.array([[0, 0, 1]], F32)
    inside, t_in, t_out = B.box_ray(o, d, np.zeros(1, F32), np.full(1, np.inf, F32), np.array([2e-35, 2e-35, 2e-35], F32), np.array([3e-35, 3e-35, 3e-35], F32))
    assert inside[0] and t_in[0] == 0 and np.isinf(t_out[0])
