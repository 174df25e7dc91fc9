"""Closest point on a mesh on the MI355X: nrf_face_grid_count / _build and nrf_closest_on_mesh against the numpy restatement (tests/closest_ref.py, brute force over
all pairs, no grid) with uint32 / integer equality -- spheres at three levels under queries of every kind, every grid shape, both sides of the large-face
threshold, the brute-force fallback, max_dist at a float's edge, invalid faces of every class -- the run-to-run guarantees, the refusals over live buffers, and the
Python layer built on it: FaceGrid, ClosestOnMesh, InterpolateAttributes, SurfaceDistance(to="surface"), TransferAttributes(source="surface") and
BakeTexture(source=<Mesh>).  No input here is outside the contract: bad indices and non-finite values have a defined answer and are rejected before any dereference."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import closest_ref as CR
import geometry_ref as G
import raster_ref as R
import smooth_ref as S
import texture_ref as X
import tsdf_ref as T

pytestmark = pytest.mark.gpu

F32 = np.float32
INVALID_ARG, WORKSPACE = 1, 4
INF = float("inf")
SPHERE_BOX = (-0.8, -1.05, -0.7, 1.0, 0.75, 1.1)          # around the sphere of tsdf_ref.SPHERE, a little wider
GRIDS = [(1, 1, 1), (2, 3, 5), (32, 32, 32), (1024, 1, 1), (1, 1024, 1), (1, 1, 1024)]


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from nerfpp_amd import _lib as L, geometry, mesh, texture
    return L, geometry, mesh, texture


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, F32).view(np.uint32)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def p(t):
    return None if t is None else t.data_ptr()


def buffer(nbytes, pattern):
    ws = torch.empty((max(1, int(nbytes)),), dtype=torch.uint8, device="cuda")
    if pattern is not None:
        ws.fill_(pattern)
    return ws


def build_grid(api, verts, faces, box, dims, pattern=None, stats=None):
    """nrf_face_grid_count + _build -> dict(dv, df, nv, nf, box, dims, n_refs, n_large, grid): what a query call takes"""
    lib = api[0].lib()
    verts, faces = np.asarray(verts, F32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)
    dv, df = (dev(verts, F32) if len(verts) else None), (dev(faces, np.int32) if len(faces) else None)
    box = np.ascontiguousarray(box, F32)
    ws = buffer(lib.nrf_face_grid_workspace_bytes(len(faces), *dims), pattern)
    n_refs, n_large = C.c_int64(-7), C.c_int64(-7)
    status = lib.nrf_face_grid_count(p(dv), len(verts), p(df), len(faces), box.ctypes.data, *dims, C.addressof(n_refs), C.addressof(n_large), p(stats), p(ws), ws.numel(), None)
    assert status == 0, lib.nrf_last_error()
    g = dict(dv=dv, df=df, nv=len(verts), nf=len(faces), box=box, dims=tuple(dims), n_refs=int(n_refs.value), n_large=int(n_large.value))
    g["grid"] = buffer(lib.nrf_face_grid_bytes(g["nf"], *dims, g["n_refs"], g["n_large"]), pattern)
    assert g["grid"].numel() == lib.nrf_face_grid_bytes(g["nf"], *dims, g["n_refs"], g["n_large"]) > 0
    status = lib.nrf_face_grid_build(p(dv), g["nv"], p(df), g["nf"], box.ctypes.data, *dims, g["n_refs"], g["n_large"], p(g["grid"]), g["grid"].numel(), p(ws), ws.numel(), None)
    assert status == 0, lib.nrf_last_error()
    if pattern is not None:
        ws.fill_(pattern ^ 0xFF)          # the workspace may go after the build
    return g


def query_grid(api, g, query, max_dist=INF, skip=(), pattern=None, stats=None, poison=-7.0):
    lib = api[0].lib()
    q = np.asarray(query, F32).reshape(-1, 3)
    dq = dev(q, F32) if len(q) else None
    d2 = torch.full((len(q),), poison, device="cuda")
    face = torch.full((len(q),), -7, dtype=torch.int32, device="cuda")
    uv = None if "uv" in skip else torch.full((len(q), 2), poison, device="cuda")
    pt = None if "point" in skip else torch.full((len(q), 3), poison, device="cuda")
    ws = buffer(lib.nrf_closest_on_mesh_workspace_bytes(len(q)), pattern)
    status = lib.nrf_closest_on_mesh(p(dq), len(q), p(g["dv"]), g["nv"], p(g["df"]), g["nf"], g["box"].ctypes.data, *g["dims"], g["n_refs"], g["n_large"], p(g["grid"]),
                                     g["grid"].numel(), max_dist, p(d2) if len(q) else None, p(face) if len(q) else None, p(uv), p(pt), p(stats), p(ws), ws.numel(), None)
    assert status == 0, lib.nrf_last_error()
    torch.cuda.synchronize()
    h = lambda t: None if t is None else t.cpu().numpy()
    return dict(d2=h(d2), face=h(face), uv=h(uv), point=h(pt))


def run(api, query, verts, faces, box, dims, max_dist=INF, skip=(), pattern=None):
    """count, build, query -> the outputs, stats [4] uint32, n_refs, n_large"""
    stats = torch.zeros((4,), dtype=torch.int32, device="cuda")
    g = build_grid(api, verts, faces, box, dims, pattern, stats)
    out = query_grid(api, g, query, max_dist, skip, pattern, stats)
    out.update(stats=stats.cpu().numpy().view(np.uint32), n_refs=g["n_refs"], n_large=g["n_large"])
    return out


def assert_equal(got, want, what="", fallback=None):
    assert np.array_equal(bits(got["d2"]), bits(want["d2"])), f"{what}: d2 differs at {np.flatnonzero(bits(got['d2']) != bits(want['d2']))[:5]}"
    assert np.array_equal(got["face"], want["face"]), f"{what}: face differs at {np.flatnonzero(got['face'] != want['face'])[:5]}"
    if got["uv"] is not None:
        assert np.array_equal(bits(got["uv"]), bits(want["uv"])), f"{what}: uv"
    if got["point"] is not None:
        assert np.array_equal(bits(got["point"]), bits(want["point"])), f"{what}: point"
    if "stats" in got and "stats" in want:
        assert np.array_equal(got["stats"][:3], want["stats"][:3]), f"{what}: stats {got['stats']} != {want['stats']}"
        if fallback is not None:
            assert got["stats"][3] == fallback, f"{what}: {got['stats'][3]} fallback queries, not {fallback}"


@functools.lru_cache(maxsize=None)
def sphere_case(level):
    verts, faces = R.octa_sphere(T.SPHERE["centre"], T.SPHERE["radius"], level)
    q = CR.mesh_queries(verts, faces, 10 + level)
    return verts, faces, q, CR.closest(q, verts, faces)


# ------------------------------------------------------------------------------------ 1. the C entries
@pytest.mark.parametrize("level", [1, 2, 3])
def test_spheres_equal_the_restatement_on_every_grid(api, level):
    """Random points in and around the box, surface samples, vertices, edge midpoints, centroids, points along normals, non-finite rows; every grid the same bits"""
    verts, faces, q, want = sphere_case(level)
    assert len(faces) == 8 * 4 ** level and want["stats"].tolist() == [4, 0, 0, 0] and (want["face"][np.isfinite(q).all(-1)] >= 0).all()
    default = api[1].GridDims(np.array(SPHERE_BOX, F32), len(faces))
    for dims in GRIDS + [default]:
        got = run(api, q, verts, faces, SPHERE_BOX, dims)
        assert_equal(got, want, f"level {level}, grid {dims}")
        assert got["n_refs"] + got["n_large"] >= len(faces) and (dims != (1, 1, 1) or (got["n_refs"], got["n_large"]) == (len(faces), 0))


def test_ties_across_shared_edges_and_vertices_give_the_lowest_face(api):
    verts, faces, q, want = sphere_case(2)
    n0 = 600          # mesh_queries: 300 random, 300 surface, then the vertices and the edge midpoints
    at_verts = slice(n0, n0 + len(verts))
    at_mids = slice(n0 + len(verts), n0 + len(verts) + 3 * len(faces))
    lowest = np.array([np.flatnonzero((faces == v).any(-1)).min() for v in range(len(verts))])
    assert np.array_equal(want["face"][at_verts], lowest) and (want["d2"][at_verts] == 0).all(), "a vertex query is at distance 0 from every face around it"
    got = run(api, q, verts, faces, SPHERE_BOX, (7, 6, 5))
    assert np.array_equal(got["face"][at_verts], lowest) and np.array_equal(got["face"][at_mids], want["face"][at_mids])
    # an edge midpoint belongs to two faces; where both are at the same d2 the lower index is reported
    a, b, c = (verts[faces[:, k]] for k in range(3))
    for k in np.arange(at_mids.start, at_mids.stop)[::7]:
        r = CR.closest_on_triangle(q[k], a, b, c)
        tied = np.flatnonzero(r["d2"] == want["d2"][k])
        assert got["face"][k] == tied.min()


def test_more_than_one_scan_round_of_cells(api):
    """128 x 128 x 129 cells are 8257 blocks of 256: two rounds of the one-workgroup scan.  Every face of the sphere spans more than 64 such cells (the large list);
    300 small faces strewn through the box are binned, a few cells each"""
    verts, faces, q, _ = sphere_case(3)
    rng = np.random.default_rng(6)
    lo, hi = np.array(SPHERE_BOX[:3]), np.array(SPHERE_BOX[3:])
    small = (rng.uniform(lo, hi, (300, 1, 3)) + rng.uniform(-0.01, 0.01, (300, 3, 3))).astype(F32).reshape(-1, 3)
    verts = np.concatenate([verts, small])
    faces = np.concatenate([faces, (len(verts) - 900 + np.arange(900)).reshape(-1, 3).astype(np.int32)])
    q = q[::3]
    got = run(api, q, verts, faces, SPHERE_BOX, (128, 128, 129))
    want = CR.closest(q, verts, faces)
    assert_equal(got, want, "128 x 128 x 129")
    assert got["n_large"] == 512 and 300 <= got["n_refs"] <= 300 * 64 and (want["face"] >= 512).sum() > 20


def threshold_mesh():
    """h = 1 on a 16^3 grid over [0, 16]^3: face 0 has a cell box of 4 x 4 x 4 = 64 (binned), face 1 of 1 x 5 x 13 = 65 (large)"""
    verts = np.array([[0.5, 0.5, 0.5], [3.5, 0.5, 3.5], [0.5, 3.5, 3.5], [5.2, 0.5, 0.5], [5.8, 4.5, 6.0], [5.5, 2.0, 12.5]], F32)
    return verts, np.array([[0, 1, 2], [3, 4, 5]], np.int32)


def test_both_sides_of_the_large_face_threshold(api):
    box, dims = (0, 0, 0, 16, 16, 16), (16, 16, 16)
    rng = np.random.default_rng(3)
    q = rng.uniform(-2, 18, (500, 3)).astype(F32)
    verts, faces = threshold_mesh()
    got = run(api, q, verts, faces, box, dims)
    assert (got["n_refs"], got["n_large"]) == (64, 1)
    assert_equal(got, CR.closest(q, verts, faces), "threshold")
    for only, counts in ((faces[:1], (64, 0)), (faces[1:], (0, 1))):
        got = run(api, q, verts, only, box, dims)
        assert (got["n_refs"], got["n_large"]) == counts
        assert_equal(got, CR.closest(q, verts, only), f"threshold {counts}")
    # one triangle spans the whole grid, among 500 small ones
    c = rng.uniform(0.5, 15.5, (500, 1, 3))
    small = (c + rng.uniform(-0.2, 0.2, (500, 3, 3))).astype(F32).reshape(-1, 3)
    verts = np.concatenate([small, np.array([[0.1, 0.1, 0.1], [15.9, 0.1, 15.9], [0.1, 15.9, 15.9]], F32)])
    faces = np.arange(1503, dtype=np.int32).reshape(-1, 3)
    got = run(api, q, verts, faces, box, dims)
    cells = np.floor(verts[faces[:500]].astype(np.float64))          # h = 1: the cell of a coordinate inside the box is its floor
    assert got["n_large"] == 1 and got["n_refs"] == int((cells.max(1) - cells.min(1) + 1).prod(-1).sum())
    want = CR.closest(q, verts, faces)
    assert (want["face"] == 500).sum() > 20, "the large face is the answer of some queries"
    assert_equal(got, want, "500 small faces and one across the grid")


def test_the_fallback_serves_what_the_rings_do_not_reach(api):
    """Three small faces in one corner of a 64^3 grid: a query more than 17 cells from them finds nothing in rings 0 .. 16 and no ring completes the grid, so it
    goes to the brute-force list; a query among the faces stops after a ring or two"""
    verts = np.array([[0.1, 0.1, 0.1], [0.6, 0.2, 0.1], [0.2, 0.7, 0.3], [0.9, 0.9, 0.2], [0.4, 0.3, 0.8]], F32)
    faces = np.array([[0, 1, 2], [1, 3, 2], [0, 2, 4]], np.int32)
    rng = np.random.default_rng(8)
    far = rng.uniform(24, 66, (700, 3)).astype(F32)          # cells 24 .. 63 on every axis, some beyond the box
    near = rng.uniform(0, 1, (300, 3)).astype(F32)
    q = np.concatenate([far[:350], near, far[350:]])
    got = run(api, q, verts, faces, (0, 0, 0, 64, 64, 64), (64, 64, 64))
    assert_equal(got, CR.closest(q, verts, faces), "fallback", fallback=700)
    # a coarser grid serves everything from the rings: the same bits
    coarse = run(api, q, verts, faces, (0, 0, 0, 64, 64, 64), (8, 8, 8))
    assert_equal(coarse, got, "coarse", fallback=0)


def test_queries_far_outside_the_box(api):
    verts, faces, _, _ = sphere_case(2)
    rng = np.random.default_rng(9)
    d = rng.standard_normal((400, 3))
    q = (np.asarray(T.SPHERE["centre"]) + d * 10.0 ** rng.uniform(0, 6, (400, 1))).astype(F32)
    want = CR.closest(q, verts, faces)
    for dims in ((6, 6, 6), (40, 40, 40)):
        assert_equal(run(api, q, verts, faces, SPHERE_BOX, dims), want, f"far, grid {dims}")
    # and a mesh far outside the box of its grid: every face lives in border cells
    assert_equal(run(api, q, verts + F32(50), faces, SPHERE_BOX, (9, 9, 9)), CR.closest(q, verts + F32(50), faces), "mesh outside the box")


def test_one_triangle_all_seven_regions(api):
    """tests/test_closest_host.py asserts that these queries reach every region; here the device agrees with the restatement on each"""
    verts, faces = np.stack(CR.TRIANGLE), np.array([[0, 1, 2]], np.int32)
    want = CR.closest(CR.REGION_QUERIES, verts, faces)
    assert CR.closest_on_triangle(CR.REGION_QUERIES, *CR.TRIANGLE)["region"].tolist() == list(range(7)) * 2
    for dims in ((1, 1, 1), (5, 5, 5)):
        assert_equal(run(api, CR.REGION_QUERIES, verts, faces, (-2, -2, -2, 3, 3, 3), dims), want, f"regions, grid {dims}")


def test_max_dist_below_at_and_above_the_nearest_face(api):
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 3], [1, 0, 3], [0, 1, 3]], F32)
    faces = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    q = np.array([[0.25, 0.25, 0.5], [0.25, 0.25, 2.75], [0.25, 0.25, 1.5]], F32)          # d = 0.5, 0.25, 1.5 exactly
    free = run(api, q, verts, faces, (-1, -1, -1, 2, 2, 4), (3, 3, 5))
    assert free["d2"].tolist() == [0.25, 0.0625, 2.25] and free["face"].tolist() == [0, 1, 0]
    for md, faces_found in ((0.5, [0, 1, -1]), (float(G.next_float(0.5, up=False)), [-1, 1, -1]), (0.6, [0, 1, -1]), (0.25, [-1, 1, -1]),
                            (float(G.next_float(0.25, up=False)), [-1, -1, -1]), (0.0, [-1, -1, -1]), (1.5, [0, 1, 0])):
        got = run(api, q, verts, faces, (-1, -1, -1, 2, 2, 4), (3, 3, 5), max_dist=md)
        assert got["face"].tolist() == faces_found, md
        assert_equal(got, CR.closest(q, verts, faces, max_dist=md), f"max_dist {md}")
        miss = got["face"] < 0
        assert np.isinf(got["d2"][miss]).all() and (got["uv"][miss] == 0).all() and (got["point"][miss] == 0).all()


def test_invalid_faces_of_every_class_and_a_d2_that_overflows(api):
    verts, faces, kinds = G.adversarial_mesh()
    q = np.concatenate([CR.mesh_queries(verts[:4], faces[:4], 2, n_random=100, n_surface=100),
                        np.array([[-3e19, -3e19, -3e19], [3e19, 1, 1], [0, 0, 2e19], [-250, -250, 1]], F32)])
    want = CR.closest(q, verts, faces)
    assert want["stats"].tolist() == [4, 3, 3, 0]
    over = np.isinf(want["d2"]) & (want["face"] >= 0)
    assert over.sum() >= 1, "a d2 that overflows to +inf with a valid face is an answer"
    for box, dims in (((-2, -2, -2, 4, 4, 4), (8, 8, 8)), ((-400, -400, -2, 400, 400, 4), (40, 40, 1)), ((-2, -2, -2, 4, 4, 4), (1, 1, 1))):
        got = run(api, q, verts, faces, box, dims)
        assert_equal(got, want, f"adversarial, grid {dims}")
    verts, faces = S.dirty()
    q = CR.mesh_queries(verts[:5], faces[:3], 4, n_random=150, n_surface=100)
    want = CR.closest(q, verts, faces)
    assert want["stats"].tolist() == [4, 3, 5, 0], "three faces with a corner outside the vertices, five that touch the NaN vertex"
    for dims in ((5, 4, 3), (30, 30, 30)):
        assert_equal(run(api, q, verts, faces, (-0.5, -1.5, -0.5, 3.5, 2.5, 1.5), dims), want, f"dirty, grid {dims}")


def test_permutation_two_runs_poison_and_null_outputs(api):
    verts, faces, q, want = sphere_case(3)
    q = q[::2]
    sub = {k: v[::2] for k, v in want.items() if k != "stats"}
    perm = np.random.default_rng(5).permutation(len(faces))
    moved = run(api, q, verts, faces[perm], SPHERE_BOX, (12, 12, 12))
    assert np.array_equal(bits(moved["d2"]), bits(sub["d2"])), "the distance does not depend on the order of the faces"
    first = run(api, q, verts, faces, SPHERE_BOX, (12, 12, 12))
    for pattern in (0xFF, 0x00, 0x5A):
        again = run(api, q, verts, faces, SPHERE_BOX, (12, 12, 12), pattern=pattern)
        for k in ("d2", "face", "uv", "point", "stats"):
            assert np.array_equal(first[k].view(np.uint32), again[k].view(np.uint32)), (pattern, k)
        assert (again["n_refs"], again["n_large"]) == (first["n_refs"], first["n_large"])
    assert_equal(first, sub, "12^3")
    for skip in (("uv",), ("point",), ("uv", "point")):
        got = run(api, q, verts, faces, SPHERE_BOX, (12, 12, 12), skip=skip)
        assert all(got[k] is None for k in skip)
        assert_equal(got, sub, f"without {skip}")
    # one grid, many queries: both halves through the same buffer, no stats
    g = build_grid(api, verts, faces, SPHERE_BOX, (12, 12, 12))
    half = len(q) // 2
    for part in (slice(0, half), slice(half, None)):
        assert_equal(query_grid(api, g, q[part]), {k: v[part] for k, v in sub.items()}, f"reused grid {part}")


def test_empty_inputs_and_a_grid_of_another_mesh(api):
    lib = api[0].lib()
    verts, faces, q, want = sphere_case(1)
    none = run(api, q, verts, np.zeros((0, 3), np.int32), SPHERE_BOX, (4, 4, 4))
    assert (none["n_refs"], none["n_large"]) == (0, 0) and (none["face"] == -1).all() and np.isinf(none["d2"]).all() and (none["uv"] == 0).all() and (none["point"] == 0).all()
    assert none["stats"].tolist() == [4, 0, 0, 0]
    no_verts = run(api, q, np.zeros((0, 3), F32), faces, SPHERE_BOX, (4, 4, 4))
    assert (no_verts["face"] == -1).all() and no_verts["stats"].tolist() == [4, len(faces), 0, 0]
    empty = run(api, np.zeros((0, 3), F32), verts, faces, SPHERE_BOX, (4, 4, 4))
    assert len(empty["d2"]) == 0 and empty["stats"].tolist() == [0, 0, 0, 0]
    # a grid buffer of another size: refused, nothing written
    g = build_grid(api, verts, faces, SPHERE_BOX, (4, 4, 4))
    other_verts, other_faces, _, _ = sphere_case(3)
    big = build_grid(api, other_verts, other_faces, SPHERE_BOX, (4, 4, 4))
    assert big["grid"].numel() != g["grid"].numel()
    dq = dev(q, F32)
    d2, face = torch.full((len(q),), -7.0, device="cuda"), torch.full((len(q),), -7, dtype=torch.int32, device="cuda")
    ws = buffer(lib.nrf_closest_on_mesh_workspace_bytes(len(q)), 0x5A)

    def call(grid, nf=g["nf"], n_refs=g["n_refs"], n_large=g["n_large"], df=g["df"]):
        return lib.nrf_closest_on_mesh(p(dq), len(q), p(g["dv"]), g["nv"], p(df), nf, g["box"].ctypes.data, 4, 4, 4, n_refs, n_large, p(grid), grid.numel(), INF, p(d2),
                                       p(face), None, None, None, p(ws), ws.numel(), None)
    assert call(big["grid"]) == INVALID_ARG and lib.nrf_last_error().startswith(b"nrf_closest_on_mesh")
    torch.cuda.synchronize()
    assert (d2 == -7).all() and (face == -7).all() and (ws == 0x5A).all()
    # a buffer of the right size that was built for another face count: the head of the buffer says so, and the query writes nothing
    assert call(g["grid"], nf=g["nf"] - 1) == 0
    torch.cuda.synchronize()
    assert (d2 == -7).all() and (face == -7).all()
    assert call(g["grid"]) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(d2), bits(want["d2"])) and np.array_equal(face.cpu().numpy(), want["face"])


# ------------------------------------------------------------------------------------ 2. the Python layer
def make_mesh(api, verts, faces, **kw):
    v = dev(verts, F32)
    return api[2].Mesh(v, dev(faces, np.int32), torch.zeros_like(v), **kw)


def affine(verts):
    """Colours that are an affine function of position: interpolation over a face reproduces them at any point of it, a vertex snap does not"""
    m = np.array([[0.3, -0.2, 0.1], [0.1, 0.25, -0.3], [-0.2, 0.1, 0.35]], F32)
    return (verts @ m + np.array([0.5, 0.4, 0.6], F32)).astype(F32)


def test_closest_on_mesh_and_interpolation(api):
    verts, faces, q, want = sphere_case(3)
    colors = affine(verts)
    m = make_mesh(api, verts, faces, Colors=dev(colors, F32), Relevancy=dev(colors[:, 0], F32))
    stats = torch.zeros((4,), dtype=torch.int32, device="cuda")
    res = api[1].ClosestOnMesh(dev(q, F32), m, stats=stats)
    got = dict(d2=res.Dist2.cpu().numpy(), face=res.Face.cpu().numpy(), uv=res.UV.cpu().numpy(), point=res.Points.cpu().numpy(), stats=stats.cpu().numpy().view(np.uint32))
    assert_equal(got, want, "ClosestOnMesh")
    grid = api[1].FaceGrid(m, bbox=SPHERE_BOX, cells=(9, 8, 7))
    assert grid.Dims == (9, 8, 7) and grid.NRefs >= len(faces) and grid.Buffer.is_cuda
    near = api[1].ClosestOnMesh(dev(q, F32), grid, max_dist=0.1, points=False)
    lim = CR.closest(q, verts, faces, max_dist=0.1)
    assert near.Points is None and np.array_equal(near.Face.cpu().numpy(), lim["face"]) and 0 < (lim["face"] < 0).sum() < len(q)
    for name, attr in (("Colors", colors), ("Relevancy", colors[:, 0])):
        c = api[1].InterpolateAttributes(m, near, name)
        ref = CR.interpolate(attr, faces, lim["face"], lim["uv"])
        assert np.array_equal(bits(c), bits(ref if attr.ndim == 2 else ref[:, 0])), name
    # an affine attribute interpolates to its value at the closest point
    c = api[1].InterpolateAttributes(m, res, "Colors").cpu().numpy()
    hit = want["face"] >= 0
    # about 30 roundings of values below 2 on the two ways to the colour, 1.2e-7 each
    assert np.abs(c[hit] - affine(want["point"][hit])).max() < 4e-6 and (c[~hit] == 0).all()


def test_surface_distance_to_the_surface(api):
    n_points, seed = 2000, 2
    meshes, clouds, raw = [], [], []
    for radius in (0.70, 0.75):
        verts, faces = R.octa_sphere(T.SPHERE["centre"], radius, 3)
        area = G.sample_count(verts, faces, 0.0, seed)["total_area"]
        clouds.append(G.sample(verts, faces, F32(n_points / area), seed)[1])
        meshes.append(make_mesh(api, verts, faces))
        raw.append((verts, faces))
    taus = (0.03, 0.05, 0.2)
    d_ab, d_ba = CR.closest(clouds[0], *raw[1])["d2"], CR.closest(clouds[1], *raw[0])["d2"]
    sa, sb = G.distance_stats(d_ab, taus), G.distance_stats(d_ba, taus)
    got = api[1].SurfaceDistance(meshes[0], meshes[1], taus=taus, n_points=n_points, seed=seed, to="surface")
    acc, comp = sa[1] / sa[0], sb[1] / sb[0]
    want = dict(Accuracy=acc, Completeness=comp, Chamfer=0.5 * (acc + comp), ChamferSq=sa[2] / sa[0] + sb[2] / sb[0], Hausdorff=max(sa[3], sb[3]),
                Precision=sa[4:] / np.float64(len(clouds[0])), Recall=sb[4:] / np.float64(len(clouds[1])))
    for name, value in want.items():
        g = getattr(got, name).cpu().numpy()
        assert np.array_equal(np.ascontiguousarray(g, np.float64).view(np.uint64), np.ascontiguousarray(value, np.float64).view(np.uint64)), (name, g, value)
    pts = api[1].SurfaceDistance(meshes[0], meshes[1], taus=taus, n_points=n_points, seed=seed)
    assert float(got.Accuracy) < float(pts.Accuracy) and float(got.Completeness) < float(pts.Completeness), "the sampled distance lies above the exact one"
    same = api[1].SurfaceDistance(meshes[0], meshes[0], taus=(1e-6,), n_points=n_points, seed=seed, to="surface")
    assert float(same.Hausdorff) < 1e-6 and same.FScore.tolist() == [1]
    with pytest.raises(api[0].NrfError):
        api[1].SurfaceDistance(meshes[0], meshes[1], to="faces")


def test_transfer_attributes_from_the_surface(api):
    dense_v, dense_f = R.octa_sphere(T.SPHERE["centre"], 0.7, 3)
    coarse_v, coarse_f = R.octa_sphere(T.SPHERE["centre"], 0.7, 1)
    rng = np.random.default_rng(4)
    moved = (coarse_v + rng.uniform(-0.02, 0.02, coarse_v.shape)).astype(F32)
    colors = affine(dense_v)
    src = make_mesh(api, dense_v, dense_f, Colors=dev(colors, F32), Relevancy=dev(colors[:, :2], F32))
    dst = make_mesh(api, moved, coarse_f)
    out = api[1].TransferAttributes(src, dst, source="surface")
    want = CR.closest(moved, dense_v, dense_f)
    assert np.array_equal(bits(out.Colors), bits(CR.interpolate(colors, dense_f, want["face"], want["uv"])))
    assert np.array_equal(bits(out.Relevancy), bits(CR.interpolate(colors[:, :2], dense_f, want["face"], want["uv"]))) and out.Vertices is dst.Vertices
    snapped = api[1].TransferAttributes(src, dst)
    assert not np.array_equal(bits(snapped.Colors), bits(out.Colors))
    far = api[1].TransferAttributes(src, make_mesh(api, moved + F32(5), coarse_f), names=("Colors",), max_dist=0.5, source="surface")
    assert (far.Colors == 0).all() and far.Relevancy is None
    with pytest.raises(api[0].NrfError):
        api[1].TransferAttributes(src, dst, source="texel")


def test_bake_texture_from_a_dense_mesh(api):
    """Every owned texel of the coarse sphere's atlas holds the dense sphere's colour interpolated at the closest point of ITS surface, bit for bit; colours that are
    affine in position make the difference from a vertex snap visible"""
    dense_v, dense_f = R.octa_sphere(T.SPHERE["centre"], 0.7, 3)
    coarse_v, coarse_f = R.octa_sphere(T.SPHERE["centre"], 0.7, 1)
    colors = affine(dense_v)
    src = make_mesh(api, dense_v, dense_f, Colors=dev(colors, F32), Relevancy=dev(colors[:, 1], F32))
    dst = make_mesh(api, coarse_v, coarse_f)
    tile = 8
    atlas = api[3].BakeTexture(dst, src, tile=tile, chunk_rows=5)
    tex = X.texels(coarse_v, coarse_f, None, tile, 0.0)
    owned = tex["face"] >= 0
    pos = tex["pos"][owned]
    want = CR.closest(pos, dense_v, dense_f)
    image = atlas.Image.cpu().numpy()
    assert image.shape == owned.shape + (3,) and owned.sum() > 300 and (image[~owned] == 0).all()
    assert np.array_equal(bits(image[owned]), bits(CR.interpolate(colors, dense_f, want["face"], want["uv"])))
    # the vertex-snapped transfer of the same texels is another image: the point of the feature
    _, idx, _ = G.nearest(pos, dense_v)
    assert not np.array_equal(bits(image[owned]), bits(colors[idx])) and np.abs(image[owned] - colors[idx]).max() > 1e-3
    assert np.abs(image[owned] - affine(want["point"])).max() < 4e-6
    # relevancy, a limit on the distance, and a grid made once by the caller
    grid = api[1].FaceGrid(src)
    rel = api[3].BakeTexture(dst, grid, tile=tile, attribute="Relevancy").Image.cpu().numpy()
    assert rel.shape == owned.shape + (1,) and np.array_equal(bits(rel[owned][:, 0]), bits(CR.interpolate(colors[:, 1], dense_f, want["face"], want["uv"])[:, 0]))
    md = float(np.sqrt(np.median(want["d2"])))
    cut = api[3].BakeTexture(dst, grid, tile=tile, max_dist=md).Image.cpu().numpy()
    lim = CR.closest(pos, dense_v, dense_f, max_dist=md)
    assert 0 < (lim["face"] < 0).sum() < len(pos) and np.array_equal(bits(cut[owned]), bits(CR.interpolate(colors, dense_f, lim["face"], lim["uv"])))
    with pytest.raises(api[0].NrfError):
        api[3].BakeTexture(dst, make_mesh(api, dense_v, dense_f), tile=tile)
