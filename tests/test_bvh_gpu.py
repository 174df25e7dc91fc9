"""The mesh BVH on the MI355X, every comparison an integer / uint32 equality: nrf_sort_pairs_u32 against np.argsort(kind="stable"); the buffer nrf_mesh_bvh_build
writes against the top-down restatement (tests/bvh_ref.py) node for node; nrf_bvh_closest_on_mesh and nrf_bvh_ray_cast_mesh against the brute-force restatements
(tests/closest_ref.py, tests/raycast_ref.py) AND against the face grid's entries, on the rays and queries the grid sends to its fallback among them; queries in
spatial order; the Python layer against its FaceGrid results; and the refusals over live buffers."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import bvh_ref as B
import closest_ref as CR
import geometry_ref as G
import raycast_ref as RR
import tsdf_ref as T

pytestmark = pytest.mark.gpu

F32 = np.float32
INVALID_ARG, WORKSPACE = 1, 4
INF = float("inf")
MESHES = ["soup0", "soup1", "soup2", "soup3", "soup255", "soup256", "soup257", "ico1280", "copies300", "flat", "mixed", "invalid_only", "floor"]
SPHERE_BOX = (-0.8, -1.05, -0.7, 1.0, 0.75, 1.1)
CENTRE = np.asarray(T.SPHERE["centre"], np.float64)


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from nerfpp_amd import _lib as L, geometry, mesh, align, texture, raster
    return L, geometry, mesh, align, texture, raster


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


@functools.lru_cache(maxsize=None)
def meshes():
    return B.meshes()


@functools.lru_cache(maxsize=None)
def tree_of(name):
    return B.build(*meshes()[name])


# ------------------------------------------------------------------------------------ 1. the sort
def sort_pairs(api, keys, values, begin, end, pattern=0xA5):
    lib = api[0].lib()
    n = len(keys)
    dk, dv = (dev(keys, np.uint32) if n else None), (None if values is None or n == 0 else dev(values, np.int32))
    ok, ov = torch.full((n,), -7, dtype=torch.int32, device="cuda"), torch.full((n,), -7, dtype=torch.int32, device="cuda")
    ws = buffer(lib.nrf_sort_workspace_bytes(n), pattern)
    status = lib.nrf_sort_pairs_u32(p(dk), p(dv), n, begin, end, p(ok) if n else None, p(ov) if n else None, p(ws), ws.numel(), None)
    assert status == 0, lib.nrf_last_error()
    torch.cuda.synchronize()
    return ok.cpu().numpy().view(np.uint32), ov.cpu().numpy()


@pytest.mark.parametrize("n", [0, 1, 63, 255, 256, 257, 65537])
def test_the_sort_is_the_stable_argsort(api, n):
    rng = np.random.default_rng(n)
    kinds = {"random": rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), "few": rng.integers(0, 5, n).astype(np.uint32) * np.uint32(0x01010101),
             "equal": np.full(n, 0xDEADBEEF, np.uint32), "descending": (np.uint32(0xFFFFFFFF) - np.arange(n, dtype=np.uint32) * np.uint32(7)),
             "top byte": (rng.integers(0, 256, n).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00ABCDEF)}
    payload = rng.integers(-(1 << 31), 1 << 31, n).astype(np.int32)
    for name, keys in kinds.items():
        for begin, end in ((0, 32), (8, 24), (3, 17), (0, 30), (24, 32), (5, 5), (31, 32)):
            masked = (keys.astype(np.uint64) >> np.uint64(begin)) & np.uint64((1 << (end - begin)) - 1)
            order = np.argsort(masked, kind="stable")
            for values, pattern in ((None, 0xA5), (payload, 0x5A)):
                got_k, got_v = sort_pairs(api, keys, values, begin, end, pattern)
                want_v = order.astype(np.int32) if values is None else values[order]
                assert np.array_equal(got_k, keys[order]) and np.array_equal(got_v, want_v), (name, n, begin, end, values is None)
            if (begin, end) == (0, 32):          # two runs over differently poisoned workspaces: the same bytes
                again = sort_pairs(api, keys, payload, begin, end, 0x00)
                assert np.array_equal(again[0], got_k) and np.array_equal(again[1], got_v)


# ------------------------------------------------------------------------------------ 2. the build
def build_bvh(api, verts, faces, pattern=0xA5, stats=None):
    """nrf_mesh_bvh_build over a poisoned buffer and workspace; the workspace is overwritten afterwards -> dict(dv, df, nv, nf, bvh): what a query takes"""
    lib = api[0].lib()
    verts, faces = np.asarray(verts, F32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)
    dv, df = (dev(verts, F32) if len(verts) else None), (dev(faces, np.int32) if len(faces) else None)
    g = dict(dv=dv, df=df, nv=len(verts), nf=len(faces), bvh=buffer(lib.nrf_mesh_bvh_bytes(len(faces)), pattern))
    assert g["bvh"].numel() == lib.nrf_mesh_bvh_bytes(len(faces)) == B.layout(len(faces))[2]
    ws = buffer(lib.nrf_mesh_bvh_workspace_bytes(len(faces)), pattern)
    status = lib.nrf_mesh_bvh_build(p(dv), g["nv"], p(df), g["nf"], p(g["bvh"]), g["bvh"].numel(), p(stats), p(ws), ws.numel(), None)
    assert status == 0, lib.nrf_last_error()
    ws.fill_(pattern ^ 0xFF)          # the workspace may go after the build
    return g


@pytest.mark.parametrize("name", MESHES)
def test_the_built_buffer_is_the_restated_tree(api, name):
    verts, faces = meshes()[name]
    want = tree_of(name)
    stats = torch.zeros((4,), dtype=torch.int32, device="cuda")
    g = build_bvh(api, verts, faces, 0xA5, stats)
    torch.cuda.synchronize()
    raw = g["bvh"].cpu().numpy()
    got = B.parse(raw, len(faces))
    assert B.same_tree(got, want) == [], name
    assert B.check_invariants(got, verts, faces) == want["height"]
    assert np.array_equal(stats.cpu().numpy().view(np.uint32), want["stats"])
    again = build_bvh(api, verts, faces, 0x3C)
    torch.cuda.synchronize()
    assert np.array_equal(again["bvh"].cpu().numpy(), raw), "two builds over differently poisoned buffers: the same bytes"


# ------------------------------------------------------------------------------------ 3. closest point
def closest_bvh(api, g, query, max_dist=INF, skip=(), order=None, stats=None, poison=-7.0):
    lib = api[0].lib()
    q = np.asarray(query, F32).reshape(-1, 3)
    n = len(q)
    dq = dev(q, F32) if n else None
    d2 = torch.full((n,), poison, device="cuda")
    face = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    uv = None if "uv" in skip else torch.full((n, 2), poison, device="cuda")
    pt = None if "point" in skip else torch.full((n, 3), poison, device="cuda")
    do = None if order is None else dev(order, np.int32)
    assert lib.nrf_bvh_query_workspace_bytes(n) == 0
    status = lib.nrf_bvh_closest_on_mesh(p(dq), n, p(g["dv"]), g["nv"], p(g["df"]), g["nf"], p(g["bvh"]), g["bvh"].numel(), p(do), max_dist, p(d2) if n else None,
                                         p(face) if n else None, p(uv), p(pt), p(stats), None, 0, None)
    assert status == 0, lib.nrf_last_error()
    torch.cuda.synchronize()
    h = lambda t: None if t is None else t.cpu().numpy()
    out = dict(d2=h(d2), face=h(face), uv=h(uv), point=h(pt))
    if stats is not None:
        out["stats"] = stats.cpu().numpy().view(np.uint32)
    return out


def same_closest(got, want, what):
    assert np.array_equal(bits(got["d2"]), bits(want["d2"])), f"{what}: d2 differs at {np.flatnonzero(bits(got['d2']) != bits(want['d2']))[:5]}"
    assert np.array_equal(got["face"], want["face"]), f"{what}: face differs at {np.flatnonzero(got['face'] != want['face'])[:5]}"
    for k in ("uv", "point"):
        if got[k] is not None:
            assert np.array_equal(bits(got[k]), bits(want[k])), f"{what}: {k}"
    if "stats" in got and "stats" in want:
        assert got["stats"].tolist() == [want["stats"][0], 0, 0, 0], f"{what}: stats {got['stats']} (entry 3 stays 0: there is no fallback)"


def make_mesh(api, verts, faces, **kw):
    v = dev(np.asarray(verts, F32).reshape(-1, 3), F32)
    return api[2].Mesh(v, dev(np.asarray(faces, np.int32).reshape(-1, 3), np.int32), torch.zeros_like(v), **kw)


@functools.lru_cache(maxsize=None)
def closest_case(name):
    """-> (verts, faces, queries, CR.closest of them): queries of every kind around the valid faces, far queries (the grid's fallback) and non-finite rows"""
    verts, faces = meshes()[name]
    cls = CR.face_classes(verts, faces)[0]
    rng = np.random.default_rng(len(name))
    unit = rng.standard_normal((120, 3))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    far = np.concatenate([unit[:60] * 100, unit[60:] * 10.0 ** rng.uniform(2, 6, (60, 1))]).astype(F32)
    if (cls == 0).any():
        keep = faces[cls == 0]
        used = np.unique(keep)
        near = CR.mesh_queries(verts[used], np.searchsorted(used, keep), 20, n_random=150, n_surface=150)[::3 if len(keep) > 600 else 1]
    else:
        near = np.concatenate([rng.uniform(-1, 1, (50, 3)), [[np.nan, 0, 0], [0, np.inf, 0]]]).astype(F32)
    q = np.concatenate([near, far]).astype(F32)
    return verts, faces, q, CR.closest(q, verts, faces)


@pytest.mark.parametrize("name", MESHES)
def test_closest_equals_the_restatement_and_the_grid(api, name):
    verts, faces, q, want = closest_case(name)
    g = build_bvh(api, verts, faces)
    got = closest_bvh(api, g, q, stats=torch.zeros((4,), dtype=torch.int32, device="cuda"))
    same_closest(got, want, name)
    assert want["stats"][0] >= 1 and (name in ("soup0", "invalid_only") or (want["face"][np.isfinite(q).all(-1)] >= 0).all())
    # the face grid of the same mesh, its fallback at work on the far queries
    gstats = torch.zeros((4,), dtype=torch.int32, device="cuda")
    grid = api[1].ClosestOnMesh(dev(q, F32), make_mesh(api, verts, faces), stats=gstats)
    same_closest(got, dict(d2=grid.Dist2.cpu().numpy(), face=grid.Face.cpu().numpy(), uv=grid.UV.cpu().numpy(), point=grid.Points.cpu().numpy()), name + " against the grid")
    # any order of service, and outputs left out
    n = len(q)
    codes = B.morton(q, tree_of(name)["lo"], tree_of(name)["hi"])
    for what, order in (("identity", np.arange(n)), ("reversed", np.arange(n)[::-1]), ("morton", np.argsort(codes, kind="stable"))):
        same_closest(closest_bvh(api, g, q, order=order), want, f"{name}, {what} order")
    bare = closest_bvh(api, g, q, skip=("uv", "point"))
    assert bare["uv"] is None and bare["point"] is None
    same_closest(bare, want, name + ", no uv or point")


def test_max_dist_at_a_floats_edge_regions_and_overflow(api):
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 3], [1, 0, 3], [0, 1, 3]], F32)
    faces = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    q = np.array([[0.25, 0.25, 0.5], [0.25, 0.25, 2.75], [0.25, 0.25, 1.5]], F32)          # d = 0.5, 0.25, 1.5 exactly
    g = build_bvh(api, verts, faces)
    for md, faces_found in ((0.5, [0, 1, -1]), (float(G.next_float(0.5, up=False)), [-1, 1, -1]), (0.6, [0, 1, -1]), (0.25, [-1, 1, -1]),
                            (float(G.next_float(0.25, up=False)), [-1, -1, -1]), (0.0, [-1, -1, -1]), (1.5, [0, 1, 0])):
        got = closest_bvh(api, g, q, max_dist=md)
        assert got["face"].tolist() == faces_found, md
        same_closest(got, CR.closest(q, verts, faces, max_dist=md), f"max_dist {md}")
    tri, one = np.stack(CR.TRIANGLE), np.array([[0, 1, 2]], np.int32)
    same_closest(closest_bvh(api, build_bvh(api, tri, one), CR.REGION_QUERIES), CR.closest(CR.REGION_QUERIES, tri, one), "one triangle, seven regions")
    verts, faces, _ = G.adversarial_mesh()          # invalid faces of every class, and a d2 that overflows to +inf with a valid face
    q = np.concatenate([CR.mesh_queries(verts[:4], faces[:4], 2, n_random=100, n_surface=100), np.array([[-3e19, -3e19, -3e19], [3e19, 1, 1], [0, 0, 2e19], [-250, -250, 1]], F32)])
    want = CR.closest(q, verts, faces)
    assert (np.isinf(want["d2"]) & (want["face"] >= 0)).any()
    stats = torch.zeros((4,), dtype=torch.int32, device="cuda")
    got = closest_bvh(api, build_bvh(api, verts, faces, stats=stats), q, stats=stats)
    assert got["stats"].tolist() == want["stats"].tolist()
    same_closest({k: v for k, v in got.items() if k != "stats"}, want, "adversarial")
    # ties across shared edges and vertices: the lowest face index
    verts, faces = B.sphere(2)
    want = CR.closest(verts, verts, faces)
    assert (want["d2"] == 0).all() and np.array_equal(want["face"], [np.flatnonzero((faces == v).any(-1)).min() for v in range(len(verts))])
    same_closest(closest_bvh(api, build_bvh(api, verts, faces), verts), want, "vertex queries")


# ------------------------------------------------------------------------------------ 4. ray casting
def cast_bvh(api, g, rays, cull=0, mode=0, skip=(), order=None, poison=-7.0):
    lib = api[0].lib()
    rays = np.ascontiguousarray(rays, F32)
    n = len(rays)
    dr = dev(rays, F32) if n else None
    closest = mode == 0
    t = torch.full((n,), poison, device="cuda") if closest else None
    face = torch.full((n,), -7, dtype=torch.int32, device="cuda") if closest else None
    uv = torch.full((n, 2), poison, device="cuda") if closest and "uv" not in skip else None
    pt = torch.full((n, 3), poison, device="cuda") if closest and "point" not in skip else None
    hit = None if closest and "hit" in skip else torch.full((n,), 77, dtype=torch.uint8, device="cuda")
    stats = torch.zeros((4,), dtype=torch.int32, device="cuda")
    do = None if order is None else dev(order, np.int32)
    status = lib.nrf_bvh_ray_cast_mesh(p(dr), n, rays.shape[1], p(g["dv"]), g["nv"], p(g["df"]), g["nf"], p(g["bvh"]), g["bvh"].numel(), p(do), cull, mode, p(t), p(face),
                                       p(uv), p(pt), p(hit), p(stats), None, 0, None)
    assert status == 0, lib.nrf_last_error()
    torch.cuda.synchronize()
    h = lambda x: None if x is None else x.cpu().numpy()
    return dict(t=h(t), face=h(face), uv=h(uv), point=h(pt), hit=h(hit), stats=stats.cpu().numpy().view(np.uint32))


def same_cast(api, g, rays, want, what, cull=0, order=None):
    got = cast_bvh(api, g, rays, cull, 0, order=order)
    for k in ("t", "uv", "point"):
        assert np.array_equal(bits(got[k]), bits(want[k])), f"{what}: {k} differs at {np.flatnonzero((bits(got[k]) != bits(want[k])).reshape(len(rays), -1).any(1))[:5]}"
    assert np.array_equal(got["face"], want["face"]) and np.array_equal(got["hit"], want["hit"]), what
    assert got["stats"].tolist() == [int(want["stats"][0]), 0, 0, 0], f"{what}: stats {got['stats']}"
    some = cast_bvh(api, g, rays, cull, 1, order=order)
    assert np.array_equal(some["hit"], np.isfinite(got["t"]).astype(np.uint8)) and some["stats"].tolist() == got["stats"].tolist(), f"{what}: any mode is isfinite(T)"
    return got


def grid_cast(api, rays, verts, faces, cull="none"):
    """RayCastMesh and Occluded over a FaceGrid of the mesh -> (RayCastResult, hit, stats [4])"""
    stats = torch.zeros((4,), dtype=torch.int32, device="cuda")
    grid = api[1].FaceGrid(make_mesh(api, verts, faces))
    res = api[1].RayCastMesh(dev(rays, F32), grid, cull=cull, stats=stats)
    return res, api[1].Occluded(dev(rays, F32), grid, cull=cull), stats.cpu().numpy()


@functools.lru_cache(maxsize=None)
def ray_case(name):
    verts, faces = meshes()[name]
    cls = CR.face_classes(verts, faces)[0]
    if (cls == 0).any():
        keep = faces[cls == 0]
        used = np.unique(keep)
        rays, _ = RR.mesh_rays(verts[used], np.searchsorted(used, keep), 30, n=60)
    else:
        rays, _ = RR.mesh_rays(*B.soup(3, 1), 30, n=20)
    far = rays[::4].copy()          # origins 1e3 and 1e6 times as far, aimed back at the mesh: the grid's far-origin fallback
    scale = np.where(np.arange(len(far)) % 2 == 0, F32(1e3), F32(1e6))[:, None]
    aim = far[:, :3] + far[:, 3:6]
    far[:, :3] = (far[:, :3] * scale).astype(F32)
    far[:, 3:6] = aim - far[:, :3]
    rays = np.concatenate([rays, far]).astype(F32)
    return verts, faces, rays, RR.cast(rays, verts, faces)


@pytest.mark.parametrize("name", MESHES)
def test_ray_cast_equals_the_restatement_and_the_grid(api, name):
    verts, faces, rays, want = ray_case(name)
    g = build_bvh(api, verts, faces)
    got = same_cast(api, g, rays, want, name)
    res, occ, gstats = grid_cast(api, rays, verts, faces)
    assert np.array_equal(bits(res.T), bits(got["t"])) and np.array_equal(res.Face.cpu().numpy(), got["face"]) and np.array_equal(bits(res.UV), bits(got["uv"])) and \
        np.array_equal(bits(res.Points), bits(got["point"])) and np.array_equal(occ.cpu().numpy(), got["hit"].astype(bool)), name + " against the grid"
    if tree_of(name)["n_valid"] > 1:
        assert gstats[3] > 0, "the far origins are rays the grid sends to its fallback"
    wide = np.zeros((len(rays), 11), F32)          # a wider row: the same rays, the rest ignored
    wide[:, :8], wide[:, 8:] = rays, 5.0
    same_cast(api, g, wide, want, name + ", stride 11")
    codes = B.morton(rays[:, :3], tree_of(name)["lo"], tree_of(name)["hi"])
    for what, order in (("reversed", np.arange(len(rays))[::-1]), ("morton", np.argsort(codes, kind="stable"))):
        same_cast(api, g, rays, want, f"{name}, {what} order", order=order)


@pytest.mark.parametrize("cull", [1, 2])
def test_cull_modes_and_a_box_that_does_not_hold_the_mesh(api, cull):
    verts, faces = B.sphere(2)
    rays, _ = RR.mesh_rays(verts, faces, 12, n=100, box=SPHERE_BOX)
    g = build_bvh(api, verts, faces)
    want = RR.cast(rays, verts, faces, cull=cull)
    got = same_cast(api, g, rays, want, f"cull {cull}", cull=cull)
    assert 50 < want["hit"].sum() < RR.cast(rays, verts, faces)["hit"].sum()
    # a grid whose box misses part of the mesh sends every open ray to its fallback; the BVH has no such premise
    lib = api[0].lib()
    small = api[1].FaceGrid(make_mesh(api, verts, faces), bbox=(-0.2, -0.2, -0.2, 0.3, 0.3, 0.3), cells=(4, 4, 4))
    stats = torch.zeros((4,), dtype=torch.int32, device="cuda")
    res = api[1].RayCastMesh(dev(rays, F32), small, cull={1: "back", 2: "front"}[cull], stats=stats)
    _, _, lo, hi, valid = RR.ray_parts(rays)
    assert stats[3].item() == int((valid & (lo <= hi)).sum()) > 0
    assert np.array_equal(bits(res.T), bits(got["t"])) and np.array_equal(res.Face.cpu().numpy(), got["face"])
    # the mesh shifted by 100 units under rays shifted with it
    moved, r = (verts + F32(100)).astype(F32), rays.copy()
    r[:, :3] += F32(100)
    same_cast(api, build_bvh(api, moved, faces), r, RR.cast(r, moved, faces, cull=cull), f"shifted by 100, cull {cull}", cull=cull)


# ------------------------------------------------------------------------------------ 5. the Python layer
def test_the_python_layer_equals_its_face_grid_results(api):
    L, Geo, M, A, X, Ras = api
    verts, faces = meshes()["ico1280"]
    colors = dev(np.abs(verts), F32)
    nrm = verts - np.array([0.1, -0.15, 0.2], F32)
    mesh = M.Mesh(dev(verts, F32), dev(faces, np.int32), dev(nrm / np.linalg.norm(nrm, axis=1, keepdims=True), F32), Colors=colors)
    grid, bvh = Geo.FaceGrid(mesh), Geo.MeshBVH(mesh)
    _, _, q, _ = closest_case("ico1280")
    rays = dev(ray_case("ico1280")[2], F32)
    dq = dev(q, F32)
    eq = lambda a, b: a is b or (a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8)))          # the same bytes (NaNs too)
    for coherent in (False, True):
        for kw in (dict(), dict(max_dist=0.3, uv=False)):
            a, b = Geo.ClosestOnMesh(dq, grid, **kw), Geo.ClosestOnMesh(dq, bvh, coherent=coherent, **kw)
            assert eq(a.Dist2, b.Dist2) and eq(a.Face, b.Face) and eq(a.UV, b.UV) and eq(a.Points, b.Points), ("ClosestOnMesh", coherent, kw)
        for cull in ("none", "back"):
            a, b = Geo.RayCastMesh(rays, grid, cull=cull), Geo.RayCastMesh(rays, bvh, cull=cull, coherent=coherent)
            assert eq(a.T, b.T) and eq(a.Face, b.Face) and eq(a.UV, b.UV) and eq(a.Points, b.Points), ("RayCastMesh", coherent, cull)
            assert eq(Geo.Occluded(rays, grid, cull=cull), Geo.Occluded(rays, bvh, cull=cull, coherent=coherent))
        o, d = rays[:, 0:3], rays[:, 3:6]
        assert eq(Geo.Visible(o, o + d, grid), Geo.Visible(o, o + d, bvh, coherent=coherent))
        assert eq(Geo.ClipRaysToMesh(rays, grid, 0.05, miss="empty"), Geo.ClipRaysToMesh(rays, bvh, 0.05, miss="empty", coherent=coherent))
        v2, f2 = B.sphere(2)
        other = M.Mesh(dev(v2, F32), dev(f2, np.int32), torch.zeros((len(v2), 3), device="cuda"))
        a, b = Geo.SurfaceDistance(other, mesh, to="surface", n_points=3000), Geo.SurfaceDistance(other, bvh, to="surface", n_points=3000, coherent=coherent)
        assert all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("Accuracy", "Completeness", "Chamfer", "ChamferSq", "Hausdorff", "Precision", "Recall", "FScore"))
        a, b = Geo.TransferAttributes(mesh, other, names=("Colors",), source="surface"), Geo.TransferAttributes(bvh, other, names=("Colors",), source="surface", coherent=coherent)
        assert eq(a.Colors, b.Colors) and a.Colors.abs().sum() > 0
    # ambient occlusion: the composition over the BVH equals the fused kernel over the grid, bad normals and slabs included
    pts, normals = mesh.Vertices.clone(), mesh.Normals.clone()
    normals[::2] = -normals[::2]          # every other point looks into the sphere: fully occluded; the others see open sky
    normals[3], normals[7, 0], pts[11, 1] = 0.0, float("nan"), float("inf")
    for k in (1, 16):
        sa, sb = torch.zeros((4,), dtype=torch.int32, device="cuda"), torch.zeros((4,), dtype=torch.int32, device="cuda")
        kw = dict(k=k, max_dist=2.0, offset=1e-3, seed=5, at=(pts, normals), index0=9)
        a, b = Geo.AmbientOcclusion(mesh, grid=grid, stats=sa, **kw), Geo.AmbientOcclusion(mesh, grid=bvh, stats=sb, **kw)
        assert eq(a, b) and sa[0] == sb[0] == 3 * k and (a == 0).sum() > 300 and (a == 1).sum() > 300, k
    old, Geo.AO_SLAB_RAYS = Geo.AO_SLAB_RAYS, 1000          # many slabs: index0 keeps the draws
    try:
        assert eq(Geo.AmbientOcclusion(mesh, grid=bvh, **kw), a)
    finally:
        Geo.AO_SLAB_RAYS = old
    assert np.array_equal(bits(bvh.Box), bits(np.concatenate([tree_of("ico1280")["lo"], tree_of("ico1280")["hi"]])))
    # three iterations of ICP against the BVH: the state and the history of the grid's run
    src = dev((verts[::3] * F32(1.02) + F32(0.01)).astype(F32), F32)
    for method in ("point", "plane"):
        a = A.RegisterICP(src, grid, iterations=3, max_dist=0.3, method=method)
        b = A.RegisterICP(src, bvh, iterations=3, max_dist=0.3, method=method)
        assert torch.equal(a.Transform.State, b.Transform.State) and torch.equal(a.History, b.History) and a.History.shape[0] == 3, method
    # a view by ray casting
    h, w, f = 24, 28, 30.0
    K = np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1]], F32)
    pose = np.array([[1, 0, 0, CENTRE[0] + 0.05], [0, 1, 0, CENTRE[1] - 0.03], [0, 0, 1, CENTRE[2] + 2.5]], F32)
    a, b = Ras.RayCastView(grid, pose, w, h, K), Ras.RayCastView(bvh, pose, w, h, K)
    assert eq(a.DepthMap, b.DepthMap) and eq(a.FaceMap, b.FaceMap) and eq(a.BaryMap, b.BaryMap) and (a.FaceMap >= 0).sum() > 50


# ------------------------------------------------------------------------------------ 6. refusals
def test_refusals_come_before_any_write(api):
    lib = api[0].lib()
    verts, faces = meshes()["soup257"]
    g = build_bvh(api, verts, faces)
    other = build_bvh(api, *meshes()["soup256"])
    q = dev(closest_case("soup257")[2][:64], F32)
    rays = dev(ray_case("soup257")[2][:64], F32)
    n = 64
    outs = dict(d2=torch.full((n,), -7.0, device="cuda"), face=torch.full((n,), -7, dtype=torch.int32, device="cuda"), uv=torch.full((n, 2), -7.0, device="cuda"),
                pt=torch.full((n, 3), -7.0, device="cuda"), hit=torch.full((n,), 77, dtype=torch.uint8, device="cuda"), codes=torch.full((n,), -7, dtype=torch.int32, device="cuda"))

    def intact():
        torch.cuda.synchronize()
        return all((v == (77 if k == "hit" else -7)).all().item() for k, v in outs.items())

    def closest(bvh=None, nbytes=None, nf=None, md=INF, q_=q, d2=outs["d2"], nq=n):
        b = g["bvh"] if bvh is None else bvh
        return lib.nrf_bvh_closest_on_mesh(p(q_), nq, p(g["dv"]), g["nv"], p(g["df"]), g["nf"] if nf is None else nf, b if isinstance(b, int) else p(b),
                                           b_bytes(b) if nbytes is None else nbytes, None, md, p(d2), p(outs["face"]), p(outs["uv"]), p(outs["pt"]), None, None, 0, None)

    def b_bytes(b):
        return g["bvh"].numel() if isinstance(b, int) else b.numel()

    def cast(bvh=None, nbytes=None, stride=8, cull=0, mode=0, t=outs["d2"], hit=None):
        b = g["bvh"] if bvh is None else bvh
        return lib.nrf_bvh_ray_cast_mesh(p(rays), n, stride, p(g["dv"]), g["nv"], p(g["df"]), g["nf"], b if isinstance(b, int) else p(b), b_bytes(b) if nbytes is None else nbytes,
                                         None, cull, mode, p(t), p(outs["face"]) if mode == 0 else None, None, None, p(hit), None, None, 0, None)

    def refused(status, name, code=INVALID_ARG):
        assert status == code and lib.nrf_last_error().decode().startswith(name), (status, lib.nrf_last_error())
        assert intact(), name

    base = g["bvh"].data_ptr()
    for status in (closest(nbytes=g["bvh"].numel() - 256), closest(bvh=other["bvh"]), closest(bvh=base + 8), closest(bvh=0), closest(md=-1.0), closest(md=float("nan")),
                   closest(q_=None), closest(d2=None), closest(nq=-1), closest(nf=1 << 31)):
        refused(status, "nrf_bvh_closest_on_mesh")
    for status in (cast(nbytes=g["bvh"].numel() + 256), cast(bvh=other["bvh"]), cast(bvh=base + 32), cast(bvh=0), cast(stride=7), cast(stride=65), cast(cull=3), cast(mode=2),
                   cast(t=None), cast(mode=1, hit=None), cast(mode=1, hit=outs["hit"])):          # any mode with a d_t
        refused(status, "nrf_bvh_ray_cast_mesh")
    refused(lib.nrf_bvh_point_codes(p(q), n, 3, p(other["bvh"]), other["bvh"].numel(), g["nf"], p(outs["codes"]), None), "nrf_bvh_point_codes")
    refused(lib.nrf_bvh_point_codes(p(q), n, 2, p(g["bvh"]), g["bvh"].numel(), g["nf"], p(outs["codes"]), None), "nrf_bvh_point_codes")
    # the build: sizes, alignment, a short workspace -- the buffer keeps its poison
    target = buffer(lib.nrf_mesh_bvh_bytes(g["nf"]), 0x77)
    ws = buffer(lib.nrf_mesh_bvh_workspace_bytes(g["nf"]), 0x77)
    for args, code in (((p(target), target.numel() - 64, None, p(ws), ws.numel()), INVALID_ARG), ((p(target) + 16, target.numel(), None, p(ws), ws.numel()), INVALID_ARG),
                       ((None, target.numel(), None, p(ws), ws.numel()), INVALID_ARG), ((p(target), target.numel(), None, None, ws.numel()), INVALID_ARG),
                       ((p(target), target.numel(), None, p(ws) + 4, ws.numel()), INVALID_ARG), ((p(target), target.numel(), None, p(ws), ws.numel() - 256), WORKSPACE)):
        status = lib.nrf_mesh_bvh_build(p(g["dv"]), g["nv"], p(g["df"]), g["nf"], *args, None)
        assert status == code and lib.nrf_last_error().decode().startswith("nrf_mesh_bvh_build"), (args, status, lib.nrf_last_error())
    torch.cuda.synchronize()
    assert (target == 0x77).all() and (ws == 0x77).all()
    # the sort
    keys = torch.zeros((n,), dtype=torch.int32, device="cuda")
    sws = buffer(lib.nrf_sort_workspace_bytes(n), 0x77)
    for args, code in (((p(keys), None, n, 0, 33, p(outs["codes"]), p(outs["face"]), p(sws), sws.numel()), INVALID_ARG),
                       ((p(keys), None, n, 9, 8, p(outs["codes"]), p(outs["face"]), p(sws), sws.numel()), INVALID_ARG),
                       ((p(keys), None, n, 0, 32, p(keys), p(outs["face"]), p(sws), sws.numel()), INVALID_ARG),
                       ((p(keys), None, n, 0, 32, p(outs["codes"]), None, p(sws), sws.numel()), INVALID_ARG),
                       ((p(keys), None, n, 0, 32, p(outs["codes"]), p(outs["face"]), p(sws), sws.numel() - 256), WORKSPACE)):
        refused(lib.nrf_sort_pairs_u32(*args, None), "nrf_sort_pairs_u32", code)
    # a buffer of the right size that was never built (or built for another F): the head disagrees, nothing is read further and nothing written
    blank = buffer(g["bvh"].numel(), 0x00)
    assert closest(bvh=blank) == 0 and cast(bvh=blank) == 0 and lib.nrf_bvh_point_codes(p(q), n, 3, p(blank), blank.numel(), g["nf"], p(outs["codes"]), None) == 0
    assert intact()
    # and empty inputs are valid and launch nothing
    assert closest(nq=0, q_=None, d2=None) == 0 and lib.nrf_sort_pairs_u32(None, None, 0, 0, 32, None, None, p(sws), sws.numel(), None) == 0 and intact()
