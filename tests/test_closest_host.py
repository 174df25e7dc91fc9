"""Closest point on a mesh without a GPU: the definition (tests/closest_ref.py, the numpy restatement the GPU tests compare nrf_closest_on_mesh with bit for bit)
pinned on an analytic sphere and on one triangle's seven regions; the header, the binding, the constants, the sizes and every refusal of every entry (they come
before any device call)."""
import ctypes as C
import os
import re

import numpy as np

import closest_ref as CR
import geometry_ref as G
import raster_ref as R
import tsdf_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
INVALID_ARG, WORKSPACE = 1, 4
CENTRE = np.asarray(T.SPHERE["centre"], np.float64)
NAMES = [("nrf_face_grid_workspace_bytes", ("z", "liii")), ("nrf_face_grid_bytes", ("z", "liiill")), ("nrf_face_grid_count", ("i", "plplpiiippppzp")),
         ("nrf_face_grid_build", ("i", "plplpiiillpzpzp")), ("nrf_closest_on_mesh_workspace_bytes", ("z", "l")),
         ("nrf_closest_on_mesh", ("i", "plplplpiiillpzfppppppzp"))]


def sphere_bounds(verts, faces):
    """(r_in, r_out): the mesh lies between the spheres of these radii about CENTRE (as tests/test_geometry_host.py takes them)"""
    return R.face_plane_distances(verts, faces, CENTRE).min(), np.linalg.norm(verts.astype(np.float64) - CENTRE, axis=1).max()


def test_header_binding_and_constants_agree():
    from nerfpp_amd import _lib, geometry, texture
    hdr = open(os.path.join(ROOT, "include", "nerfpp_hip.h")).read()
    m = re.search(r"#define\s+NRF_FG_MAX_FACE_CELLS\s+(\d+)", hdr)
    assert m and int(m[1]) == 64 == geometry.FG_MAX_FACE_CELLS == CR.FG_MAX_FACE_CELLS
    at = _lib.SYMBOLS.index("nrf_density_grad")
    assert _lib.SYMBOLS[at + 1:at + 7] == [n for n, _ in NAMES], "directly after nrf_density_grad, in the header's order"
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    for name, sig in NAMES:
        assert _lib.SIGNATURES[name] == sig and hasattr(lib, name) and re.search(rf"NRF_API (size_t|int) {name}\(", hdr), name
    for word in ("WHY THE STOP STAYS EXACT", "Ericson", "P < lo ? lo : (P > hi ? hi : P)"):
        assert word in hdr, word
    for name in ("FaceGrid", "ClosestOnMesh", "ClosestResult"):
        assert hasattr(geometry, name), name
    import inspect
    assert inspect.signature(geometry.SurfaceDistance).parameters["to"].default == "points"
    assert inspect.signature(geometry.TransferAttributes).parameters["source"].default == "vertex"
    assert {"attribute", "max_dist"} <= set(inspect.signature(texture.BakeTexture).parameters)


def test_workspace_sizes_and_refusals_need_no_gpu():
    """Every bad argument of the header is refused before anything touches the device, so the whole list is checked here over pointers that are never dereferenced."""
    from nerfpp_amd import _lib
    lib = _lib.lib()
    fake = C.c_void_p(256)
    big = 1 << 40
    box = np.array([0, 0, 0, 1, 1, 1], F32)
    pb = lambda a: a.ctypes.data_as(C.c_void_p)
    nan, inf = float("nan"), float("inf")
    boxes = [np.array(b, F32) for b in ([0, 0, 0, 1, 0, 1], [0, 0, 0, 1, 1, -1], [0, nan, 0, 1, 1, 1], [0, 0, 0, inf, 1, 1], [-inf, 0, 0, 1, 1, 1],
                                        [-3e38, 0, 0, 3e38, 1, 1], [0, 0, 0, 1, 1e-42, 1])]

    def refused(name, status, fn, cases):
        for kw in cases:
            assert fn(**kw) == status, (name, kw)
            assert lib.nrf_last_error().startswith(name.encode()), (kw, lib.nrf_last_error())

    ws_size, grid_size, q_size = lib.nrf_face_grid_workspace_bytes, lib.nrf_face_grid_bytes, lib.nrf_closest_on_mesh_workspace_bytes
    assert ws_size(512, 4, 5, 6) >= 2 * 120 * 4 + 8 + 8 + 8 and ws_size(0, 1, 1, 1) > 0 and ws_size(512, 4, 5, 6) == ws_size(7, 6, 5, 4)
    for bad in ((-1, 1, 1, 1), (2 ** 31, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, 1025, 1, 1), (1, 1, 1025, 1), (1, 1, 1, 1025), (1, 1024, 1024, 65)):
        assert ws_size(*bad) == 0, bad
        assert grid_size(*bad, 0, 0) == 0, bad
    assert grid_size(512, 4, 5, 6, 3000, 2) >= 64 + 121 * 4 + 3000 * 4 + 2 * 4 and grid_size(0, 1, 1, 1, 0, 0) > 0
    assert grid_size(512, 4, 5, 6, 3000, 2) > grid_size(512, 4, 5, 6, 1000, 2)
    for bad in ((-1, 0), (2 ** 32, 0), (0, -1), (0, 513)):
        assert grid_size(512, 4, 5, 6, *bad) == 0, bad
    assert grid_size(512, 4, 5, 6, 2 ** 32 - 1, 512) > 2 ** 34
    assert q_size(0) > 0 and q_size(1000) >= 4000 + 4 and q_size(-1) == 0 and q_size(2 ** 31) == 0

    mesh_cases = [dict(nv=-1), dict(nv=2 ** 31), dict(nf=-1), dict(nf=2 ** 31), dict(nx=0), dict(ny=0), dict(nz=-1), dict(nx=1025), dict(ny=1025), dict(nz=1025),
                  dict(nx=1024, ny=1024, nz=65), dict(faces=None), dict(verts=None), dict(b=None), dict(ws=None), dict(ws=C.c_void_p(260))] + [dict(b=pb(b)) for b in boxes]

    def count(verts=fake, nv=4, faces=fake, nf=2, b=pb(box), nx=2, ny=2, nz=2, n_refs=fake, n_large=fake, ws=fake, ws_bytes=big):
        return lib.nrf_face_grid_count(verts, nv, faces, nf, b, nx, ny, nz, n_refs, n_large, None, ws, ws_bytes, None)

    refused("nrf_face_grid_count", INVALID_ARG, count, mesh_cases + [dict(n_refs=None), dict(n_large=None)])
    refused("nrf_face_grid_count", WORKSPACE, count, [dict(ws_bytes=ws_size(2, 2, 2, 2) - 1), dict(ws_bytes=0)])

    good = grid_size(2, 2, 2, 2, 10, 1)

    def build(verts=fake, nv=4, faces=fake, nf=2, b=pb(box), nx=2, ny=2, nz=2, n_refs=10, n_large=1, grid=fake, grid_bytes=good, ws=fake, ws_bytes=big):
        return lib.nrf_face_grid_build(verts, nv, faces, nf, b, nx, ny, nz, n_refs, n_large, grid, grid_bytes, ws, ws_bytes, None)

    grid_cases = [dict(n_refs=-1), dict(n_refs=2 ** 32), dict(n_large=-1), dict(n_large=3), dict(grid=None), dict(grid=C.c_void_p(260)), dict(grid_bytes=good - 1),
                  dict(grid_bytes=good + 256), dict(grid_bytes=0), dict(n_refs=1000), dict(nx=64)]          # the last two: a buffer of another grid's size
    refused("nrf_face_grid_build", INVALID_ARG, build, mesh_cases + grid_cases)
    refused("nrf_face_grid_build", WORKSPACE, build, [dict(ws_bytes=ws_size(2, 2, 2, 2) - 1), dict(ws_bytes=0)])

    def query(q=fake, nq=3, verts=fake, nv=4, faces=fake, nf=2, b=pb(box), nx=2, ny=2, nz=2, n_refs=10, n_large=1, grid=fake, grid_bytes=good, md=inf, d2=fake, face=fake,
              ws=fake, ws_bytes=big):
        return lib.nrf_closest_on_mesh(q, nq, verts, nv, faces, nf, b, nx, ny, nz, n_refs, n_large, grid, grid_bytes, md, d2, face, None, None, None, ws, ws_bytes, None)

    refused("nrf_closest_on_mesh", INVALID_ARG, query, mesh_cases + grid_cases + [dict(nq=-1), dict(nq=2 ** 31), dict(q=None), dict(d2=None), dict(face=None), dict(md=-1.0),
                                                                                  dict(md=nan), dict(md=-inf)])
    refused("nrf_closest_on_mesh", WORKSPACE, query, [dict(ws_bytes=q_size(3) - 1), dict(ws_bytes=0)])


def test_a_query_outside_the_sphere_is_as_far_as_its_shells_allow():
    """The mesh lies between the spheres of radii r_in and r_out about CENTRE (the bounds tests/test_geometry_host.py uses), so a query at radius rho outside it is
    between rho - r_out and rho - r_in from the surface; fp32 moves the distance by far less than 1e-5 at these magnitudes."""
    verts, faces = R.octa_sphere(T.SPHERE["centre"], T.SPHERE["radius"])
    r_in, r_out = sphere_bounds(verts, faces)
    rng = np.random.default_rng(11)
    d = rng.standard_normal((400, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    for rho in (0.75, 1.0, 3.0):
        q = (CENTRE + rho * d).astype(F32)
        out = CR.closest(q, verts, faces)
        dist = np.sqrt(out["d2"].astype(np.float64))
        print(f"rho {rho}: {dist.min():.6f} .. {dist.max():.6f} within [{rho - r_out:.6f}, {rho - r_in:.6f}]")
        assert (out["face"] >= 0).all() and dist.min() >= rho - r_out - 1e-5 and dist.max() <= rho - r_in + 1e-5
        # the point lies on its face and realises the distance
        tri = verts[faces[out["face"]]].astype(np.float64)
        u, v = out["uv"][:, :1].astype(np.float64), out["uv"][:, 1:].astype(np.float64)
        assert np.abs((1 - u - v) * tri[:, 0] + u * tri[:, 1] + v * tri[:, 2] - out["point"]).max() < 1e-6
        assert np.abs(np.linalg.norm(q.astype(np.float64) - out["point"], axis=1) - dist).max() < 1e-6
        # and no vertex is nearer than the surface
        assert (G.nearest(q, verts)[0] >= out["d2"]).all()


def test_one_triangle_reaches_all_seven_regions():
    """The shared set of queries reaches every region, so the GPU comparison over it cannot pass with a region untested; each against the float64 closest point"""
    r = CR.closest_on_triangle(CR.REGION_QUERIES, *CR.TRIANGLE)
    assert r["region"].tolist() == list(range(7)) * 2 and len(CR.REGIONS) == 7
    a, b, c = (x.astype(np.float64) for x in CR.TRIANGLE)
    q = CR.REGION_QUERIES.astype(np.float64)
    want = {0: lambda p: a, 1: lambda p: b, 3: lambda p: c,
            2: lambda p: a + np.clip((p - a) @ (b - a) / ((b - a) @ (b - a)), 0, 1) * (b - a),
            4: lambda p: a + np.clip((p - a) @ (c - a) / ((c - a) @ (c - a)), 0, 1) * (c - a),
            5: lambda p: b + np.clip((p - b) @ (c - b) / ((c - b) @ (c - b)), 0, 1) * (c - b),
            6: lambda p: np.array([p[0], p[1], 0.0])}
    for k in range(len(q)):
        p = want[int(r["region"][k])](q[k])
        assert np.abs(r["p"][k] - p).max() < 1e-6 and abs(r["d2"][k] - ((q[k] - p) ** 2).sum()) < 1e-5, k
        assert np.abs((1 - r["v"][k] - r["w"][k]) * a + r["v"][k] * b + r["w"][k] * c - p).max() < 1e-6, k


def test_vertices_edge_midpoints_and_centroids():
    a, b, c = (np.array(x, F32) for x in ([0.5, -1, 2], [1.5, 0, 2.5], [0, 1, 1]))
    half = F32(0.5)
    cases = [(a, 0, (0, 0)), (b, 1, (1, 0)), (c, 3, (0, 1)), (half * (a + b), 2, (0.5, 0)), (half * (a + c), 4, (0, 0.5)), (half * (b + c), 5, (0.5, 0.5)),
             (((a.astype(np.float64) + b + c) / 3).astype(F32), 6, (1 / 3, 1 / 3))]
    for q, region, uv in cases:
        r = CR.closest_on_triangle(q, a, b, c)
        assert int(r["region"]) == region and abs(r["v"] - uv[0]) < 1e-6 and abs(r["w"] - uv[1]) < 1e-6 and r["d2"] < 1e-12, (region, r)
        assert np.abs(r["p"] - q).max() < 1e-6
    # the closed regions in their fixed order: a vertex is its vertex region, an edge midpoint its edge region, exactly
    assert [int(CR.closest_on_triangle(q, a, b, c)["d2"] == 0) for q, _, _ in cases[:3]] == [1, 1, 1]


def test_the_clamp_matters():
    """The stop rule's proof needs P inside the face's coordinate box.  A bounded random search finds pairs whose UNCLAMPED P leaves it by a rounding error (edge AB,
    v just below 1: a + v * fl(b - a) rounds past b); the clamped P never does, and the clamp moves d2 by rounding errors only."""
    a, b, c, q, region = CR.search_clamp_cases()
    print(f"{len(a)} of 100000 searched pairs leave the box before the clamp; regions {np.bincount(region, minlength=7).tolist()}")
    assert len(a) >= 1
    r = CR.closest_on_triangle(q, a, b, c)
    lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
    assert ((r["raw"] < lo) | (r["raw"] > hi)).any(-1).all() and ((r["p"] >= lo) & (r["p"] <= hi)).all()
    assert np.abs(r["p"].astype(np.float64) - r["raw"]).max() < 1e-6


def test_invalid_faces_never_win_and_are_counted():
    verts, faces, kinds = G.adversarial_mesh()
    q = CR.mesh_queries(verts[:4], faces[:4], 2, n_random=50, n_surface=50)
    out = CR.closest(q, verts, faces)
    assert out["stats"].tolist() == [4, 3, 3, 0], "face 13 (finite corners, an area that overflows) is a face here"
    assert not np.isin(out["face"], kinds["bad"] + kinds["nonfinite"][:3]).any()
    fin = np.isfinite(q).all(-1)
    assert (out["face"][fin] >= 0).all() and (out["face"][~fin] == -1).all() and np.isinf(out["d2"][~fin]).all() and (out["uv"][~fin] == 0).all()
    # a NaN vertex in the array does not matter where no face uses it
    only = CR.closest(q, verts, faces[:4])
    assert only["stats"].tolist() == [4, 0, 0, 0] and (only["d2"] >= out["d2"]).all()
    # max_dist: at the distance itself the face still counts, just below it it does not
    d = np.sqrt(out["d2"][fin].astype(np.float64)).min()
    k = int(np.flatnonzero(fin)[np.argmin(out["d2"][fin])])
    exact = F32(np.sqrt(out["d2"][k]))
    if F32(exact * exact) == out["d2"][k]:
        assert CR.closest(q[k:k + 1], verts, faces, max_dist=exact)["face"][0] == out["face"][k]
    assert CR.closest(q[k:k + 1], verts, faces, max_dist=G.next_float(F32(d * 2)))["face"][0] == out["face"][k]
    far = CR.closest(q[:8], verts, faces, max_dist=0.0)
    assert ((far["face"] == -1) | (far["d2"] == 0)).all()
