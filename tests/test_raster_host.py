"""The mesh rasteriser without a GPU: the definition (tests/raster_ref.py, the numpy restatement the GPU tests compare nrf_raster_mesh with bit for bit) pinned on
shared edges, a closed mesh, an analytic sphere, ties and permutations; the header, the binding and the refusals of the C entry (they come before any device call)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import raster_ref as R
import tsdf_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
INVALID_ARG = 1


@pytest.fixture(scope="module")
def sphere():
    """The octahedron subdivided three times onto tsdf_ref.SPHERE, seen at 48 x 56 from sphere_views' poses 0 and 1, with and without culling"""
    from nerfpp_amd import scene
    s = T.SPHERE
    verts, faces = R.octa_sphere(s["centre"], s["radius"])
    views = T.sphere_views(scene.pose_spherical, scene.lego_K)[:2]
    out = [{cull: R.rasterize(verts, faces, None, s["h"], s["w"], v["K"], v["c2w"], cull=cull) for cull in (0, 1)} for v in views]
    return dict(verts=verts, faces=faces, views=views, out=out)


def test_header_binding_and_constants_agree():
    from nerfpp_amd import _lib, raster
    hdr = open(os.path.join(ROOT, "include", "nerfpp_hip.h")).read()
    for name, value in (("SUBPIXEL", 256), ("GUARD", 16384), ("MAX_ATTR", 8), ("WIDE_PIXELS", raster.WIDE_PIXELS)):
        m = re.search(rf"#define\s+NRF_RASTER_{name}\s+(\d+)", hdr)
        assert m and int(m[1]) == value == getattr(raster, name), name
    assert (R.SUBPIXEL, R.GUARD, R.MAX_ATTR) == (raster.SUBPIXEL, raster.GUARD, raster.MAX_ATTR)
    assert re.search(r"NRF_API size_t nrf_raster_workspace_bytes\(", hdr) and re.search(r"NRF_API int nrf_raster_mesh\(", hdr)
    assert _lib.SIGNATURES["nrf_raster_workspace_bytes"] == ("z", "llii")
    assert _lib.SIGNATURES["nrf_raster_mesh"] == ("i", "plplpiiippfippppppzp")
    at = _lib.SYMBOLS.index("nrf_tsdf_sample_color")
    assert _lib.SYMBOLS[at + 1:at + 3] == ["nrf_raster_workspace_bytes", "nrf_raster_mesh"], "in the header's order"
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "nrf_raster_mesh") and hasattr(lib, "nrf_raster_workspace_bytes")
    import nerfpp_amd
    assert "raster" in nerfpp_amd.__all__ and nerfpp_amd.raster is raster


def test_workspace_size_and_refusals_need_no_gpu():
    """Every bad argument of the header is refused before anything touches the device, so the whole list is checked here; the GPU test repeats it over live buffers."""
    from nerfpp_amd import _lib
    lib = _lib.lib()
    size = lib.nrf_raster_workspace_bytes
    assert size(258, 512, 48, 56) >= 258 * 16 + 48 * 56 * 8 + 512 * 4 + 4
    assert size(0, 0, 1, 1) > 0 and size(258, 512, 48, 56) == size(258, 512, 56, 48)
    for bad in ((-1, 1, 4, 4), (1, -1, 4, 4), (1, 2 ** 31 - 1, 4, 4), (2 ** 31, 1, 4, 4), (1, 1, 0, 4), (1, 1, 4, 0), (1, 1, 16385, 4), (1, 1, 4, 16385)):
        assert size(*bad) == 0, bad
    assert size(1, 2 ** 31 - 2, 16384, 16384) > 2 ** 31
    K = np.array([[8, 0, 3], [0, 8, 2], [0, 0, 1]], F32)
    pose = R.LATTICE_POSE.copy()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(256)          # never dereferenced: every call below is refused

    def call(verts=fake, nv=4, faces=fake, nf=2, attr=None, n_attr=0, h=4, w=4, k=p(K), m=p(pose), near=1e-3, cull=0, depth=fake, out=None, ws=fake, ws_bytes=1 << 40):
        return lib.nrf_raster_mesh(verts, nv, faces, nf, attr, n_attr, h, w, k, m, near, cull, depth, None, None, out, None, ws, ws_bytes, None)

    nan, inf = float("nan"), float("inf")
    bad = [dict(verts=None), dict(faces=None), dict(k=None), dict(m=None), dict(depth=None), dict(h=0), dict(w=0), dict(h=-3), dict(h=16385), dict(w=16385),
           dict(n_attr=-1), dict(n_attr=9, attr=fake, out=fake), dict(n_attr=3), dict(n_attr=3, attr=fake), dict(n_attr=3, out=fake),
           dict(near=0.0), dict(near=-1.0), dict(near=nan), dict(near=inf), dict(cull=2), dict(cull=-1), dict(nf=-1), dict(nf=2 ** 31 - 1), dict(nv=-1), dict(nv=2 ** 31),
           dict(ws=None), dict(ws_bytes=size(4, 2, 4, 4) - 1), dict(ws_bytes=0)]
    for kw in bad:
        assert call(**kw) == INVALID_ARG, kw
        assert lib.nrf_last_error().startswith(b"nrf_raster_mesh"), (kw, lib.nrf_last_error())


@pytest.mark.parametrize("spacing", [0.25, 0.375, 0.5])
def test_shared_edges_cover_every_pixel_exactly_once(spacing):
    """9 x 9 vertices on z = -2 at 1, 1.5 and 2 pixels apart, so vertices and edges pass exactly through pixel centres; diagonals alternate and each face's winding is
    random.  The top-left rule gives every pixel centre of the half-open rectangle [u_min, u_max) x [v_min, v_max) to exactly one face, and nothing outside it."""
    verts, faces = R.lattice_mesh(spacing)
    h, w = R.LATTICE_H, R.LATTICE_W
    out = R.rasterize(verts, faces, None, h, w, R.LATTICE_K, R.LATTICE_POSE)
    u0, v0, px = 1, 1, 4 * spacing          # u = 4 x + 3, v = 2 - 4 y
    assert px * 8 == int(px * 8)
    u1, v1 = u0 + int(px * 8), v0 + int(px * 8)
    j, i = np.mgrid[0:h, 0:w]
    want = ((i >= u0) & (i < u1) & (j >= v0) & (j < v1)).astype(np.int64)
    assert want.sum() == (min(u1, w) - u0) * (min(v1, h) - v0) > 0
    assert np.array_equal(out["count"], want)
    assert np.array_equal(out["face"] >= 0, want > 0) and np.array_equal(out["depth"], np.where(want > 0, F32(2), F32(0)))
    assert out["stats"].tolist() == [len(faces), 0, 0, 0]
    # culling keeps the faces whose random winding is counter-clockwise seen from +z (the camera's side): each pixel then has its face or none
    culled = R.rasterize(verts, faces, None, h, w, R.LATTICE_K, R.LATTICE_POSE, cull=1)
    assert 0 < culled["stats"][0] < len(faces) and culled["stats"][0] + culled["stats"][2] == len(faces)
    kept = culled["face"] >= 0
    assert np.array_equal(culled["face"][kept], out["face"][kept]) and 0 < kept.sum() < want.sum()


def test_a_closed_mesh_is_covered_twice_and_once_when_culled(sphere):
    assert sphere["verts"].shape == (258, 3) and sphere["faces"].shape == (512, 3)
    import mesh_ref as M
    assert M.edge_check(sphere["faces"]) == (True, True) and M.signed_volume(sphere["verts"], sphere["faces"]) > 0, "closed, outward"
    hits = []
    for o in sphere["out"]:
        both, front = o[0], o[1]
        covered = both["count"] > 0
        assert set(np.unique(both["count"])) == {0, 2}, "a ray that enters leaves"
        assert np.array_equal(front["count"], covered.astype(np.int64))
        for k in ("depth", "face", "bary"):
            assert np.array_equal(both[k], front[k]), f"the nearest face is a front face: {k}"
        assert both["stats"].tolist() == [512, 0, 0, 0] and front["stats"][0] + front["stats"][2] == 512 and front["stats"][2] > 100
        b = both["bary"][covered]
        assert (b >= 0).all() and np.abs(b.sum(-1) - 1).max() <= 2e-7
        hits.append(int(covered.sum()))
    print("hit pixels", hits)
    assert hits == [536, 641]


def test_depth_lies_between_the_inscribed_and_the_circumscribed_sphere(sphere):
    """The mesh lies between the spheres of radius r_in (the smallest distance of a face's plane from the centre) and r_out (the largest vertex distance), so does its
    silhouette, and -- away from the silhouette, where a ray meets both -- its depth, up to the snapping allowance eps = 1.34 sqrt(2) depth / (512 min(fx, fy)): a vertex
    moves by at most sqrt(2)/512 pixel, and inside the core of radius 0.8 r_in the incidence is bounded by tan(theta) <= 1.34."""
    s = T.SPHERE
    c = np.asarray(s["centre"], np.float64)
    r_out = np.linalg.norm(sphere["verts"].astype(np.float64) - c, axis=1).max()
    r_in = R.face_plane_distances(sphere["verts"], sphere["faces"], c).min()
    print(f"r_in {r_in:.5f} r_out {r_out:.5f}")
    assert abs(r_in - 0.68931) < 1e-4 and abs(r_out - s["radius"]) < 1e-6
    for v, o in zip(sphere["views"], sphere["out"]):
        depth = o[0]["depth"]
        hit = depth > 0
        d_out, a_out = T.sphere_depth(s["h"], s["w"], v["K"], v["c2w"], r_out, c)
        d_in, a_in = T.sphere_depth(s["h"], s["w"], v["K"], v["c2w"], r_in, c)
        _, a_core = T.sphere_depth(s["h"], s["w"], v["K"], v["c2w"], 0.8 * r_in, c)
        assert not (hit & (a_out == 0)).any() and not ((a_in > 0) & ~hit).any()
        core = a_core > 0
        assert core.sum() > 200 and hit[core].all()
        eps = 1.34 * np.sqrt(2.0) * depth.astype(np.float64) / (512.0 * min(v["K"][0, 0], v["K"][1, 1]))
        assert eps[core].max() <= 1.8e-4
        lo, hi = (depth - d_out)[core].min(), (d_in - depth)[core].min()
        print(f"margins without eps: {lo:.2e} {hi:.2e}")
        assert (depth[core] >= d_out[core] - eps[core]).all() and (depth[core] <= d_in[core] + eps[core]).all()


def test_ties_permutations_and_statistics(sphere):
    s = T.SPHERE
    v = sphere["views"][0]
    verts, faces = sphere["verts"], sphere["faces"]
    base = sphere["out"][0][0]
    # two coincident faces: the lower index wins, wherever the copy stands
    rng = np.random.default_rng(2)
    where = rng.permutation(1024)                      # row k of the doubled list is face where[k] % 512
    lowest = np.full(512, 1024)
    np.minimum.at(lowest, where % 512, np.arange(1024))
    o = R.rasterize(verts, faces[where % 512], None, s["h"], s["w"], v["K"], v["c2w"])
    assert np.array_equal(o["depth"].view(np.uint32), base["depth"].view(np.uint32)) and (o["count"] == 2 * base["count"]).all()
    hit = base["face"] >= 0
    assert np.array_equal(o["face"] >= 0, hit) and np.array_equal(o["face"][hit], lowest[base["face"][hit]])
    # a permutation of the face list: the same depth bits, and the face map follows it (the sphere has no exact depth ties between different faces)
    perm = np.random.default_rng(3).permutation(len(faces))
    o = R.rasterize(verts, faces[perm], None, s["h"], s["w"], v["K"], v["c2w"])
    assert np.array_equal(o["depth"].view(np.uint32), base["depth"].view(np.uint32))
    assert np.array_equal(np.where(o["face"] >= 0, perm[np.maximum(o["face"], 0)], -1), base["face"])
    assert np.array_equal(o["bary"], base["bary"])
    # statistics: one face of each kind added to the sphere
    behind = np.asarray(v["c2w"], F32)[:, 3] + np.asarray(v["c2w"], F32)[:, 2]               # one unit along the camera's +z: it looks down -z
    extra_v = np.concatenate([verts, np.stack([behind, np.array([np.nan, 0, 0], F32)])])
    extra_f = np.concatenate([faces, np.array([[0, 1, 258], [0, 1, 259], [0, 0, 1], [5, 5, 5], [0, 1, 260], [-1, 0, 1]], np.int32)])
    o = R.rasterize(extra_v, extra_f, None, s["h"], s["w"], v["K"], v["c2w"])
    assert o["stats"].tolist() == [512, 2, 2, 2] and int(o["stats"].sum()) == len(extra_f)
    assert np.array_equal(o["depth"], base["depth"]) and np.array_equal(o["face"], base["face"])
    # attributes: a constant comes back as the constant up to rounding, and the vertex positions interpolate to the point the ray hits
    at = np.concatenate([np.full((258, 1), 0.75, F32), verts], 1)
    o = R.rasterize(verts, faces, at, s["h"], s["w"], v["K"], v["c2w"])
    hit = o["face"] >= 0
    assert np.abs(o["attr"][hit][:, 0] - 0.75).max() <= 2e-7 and (o["attr"][~hit] == 0).all()
    c2w = np.asarray(v["c2w"], np.float64)
    j, i = np.nonzero(hit)
    d = np.stack([(i - v["K"][0, 2]) / v["K"][0, 0], -(j - v["K"][1, 2]) / v["K"][1, 1], -np.ones(len(i))], -1) @ c2w[:, :3].T
    world = c2w[:, 3] + d * o["depth"][hit][:, None].astype(np.float64)
    # perspective-correct: the interpolated position is the point of the true triangle whose projection is the pixel centre moved by a convex combination of the
    # corners' snapping errors (<= sqrt(2)/512 pixel), at the interpolated depth
    tol = float(o["depth"].max()) * np.sqrt(2.0) / 512.0 / float(min(v["K"][0, 0], v["K"][1, 1])) + 1e-5
    print(f"position error {np.abs(world - o['attr'][hit][:, 1:]).max():.2e} <= {tol:.2e}")
    assert np.abs(world - o["attr"][hit][:, 1:]).max() <= tol
