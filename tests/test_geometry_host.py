"""Geometry in space without a GPU: the definition (tests/geometry_ref.py, the numpy restatement the GPU tests compare nrf_mesh_sample_*, nrf_nearest_points and
nrf_distance_stats with bit for bit) pinned on an analytic sphere; the header, the binding, the constants, the workspace sizes and every refusal of every entry (they
come before any device call)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import geometry_ref as G
import raster_ref as R
import tsdf_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
INVALID_ARG, WORKSPACE = 1, 4
CENTRE = np.asarray(T.SPHERE["centre"], np.float64)
SEEDS = (0, 1, 2)
DENSITY = 3400.0          # about 20 k points on the sphere of radius 0.7


def sphere_bounds(verts, faces):
    """(r_in, r_out): the mesh lies between the spheres of these radii about CENTRE (as tests/test_raster_host.py takes them)"""
    return R.face_plane_distances(verts, faces, CENTRE).min(), np.linalg.norm(verts.astype(np.float64) - CENTRE, axis=1).max()


@pytest.fixture(scope="module")
def sphere():
    verts, faces = R.octa_sphere(T.SPHERE["centre"], T.SPHERE["radius"])
    return dict(verts=verts, faces=faces, samples={s: G.sample(verts, faces, DENSITY, s) for s in SEEDS})


def test_header_binding_and_constants_agree():
    from nerfpp_amd import _lib, geometry
    hdr = open(os.path.join(ROOT, "include", "nerfpp_hip.h")).read()
    for name, value in (("SAMPLE_MAX_PER_FACE", 65536), ("NN_MAX_DIM", 1024), ("NN_MAX_RINGS", geometry.NN_MAX_RINGS), ("STATS_MAX_TAU", 4)):
        m = re.search(rf"#define\s+NRF_{name}\s+(\d+)", hdr)
        assert m and int(m[1]) == value == getattr(geometry, name) == getattr(G, name), name
    assert re.search(r"#define\s+NRF_NN_MAX_CELLS\s+\(1 << 26\)", hdr) and geometry.NN_MAX_CELLS == G.NN_MAX_CELLS == 1 << 26
    rng = open(os.path.join(ROOT, "include", "nrf_rng.h")).read()
    ids = dict(re.findall(r"(NRF_RNG_\w+)\s*=\s*(\d+)", rng))
    assert ids["NRF_RNG_SURFACE_COUNT"] == "10" and ids["NRF_RNG_SURFACE_UV"] == "11" and ids["NRF_RNG_NOISE_FINE"] == "9" and len(set(ids.values())) == len(ids) == 11
    assert (_lib.NRF_RNG_SURFACE_COUNT, _lib.NRF_RNG_SURFACE_UV) == (G.RNG_SURFACE_COUNT, G.RNG_SURFACE_UV) == (10, 11) and _lib.NRF_RNG_NOISE_FINE == 9
    want = [("nrf_mesh_sample_workspace_bytes", ("z", "ll")), ("nrf_mesh_sample_count", ("i", "plplfqppppzp")), ("nrf_mesh_sample_emit", ("i", "plplqlppppzp")),
            ("nrf_nearest_points_workspace_bytes", ("z", "lliii")), ("nrf_nearest_points", ("i", "plplpiiifppppzp")),
            ("nrf_distance_stats_workspace_bytes", ("z", "l")), ("nrf_distance_stats", ("i", "plpippzp"))]
    at = _lib.SYMBOLS.index("nrf_raster_mesh")
    assert _lib.SYMBOLS[at + 1:at + 8] == [n for n, _ in want], "in the header's order"
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    for name, sig in want:
        assert _lib.SIGNATURES[name] == sig and hasattr(lib, name) and re.search(rf"NRF_API (size_t|int) {name}\(", hdr), name
    import nerfpp_amd
    assert "geometry" in nerfpp_amd.__all__ and nerfpp_amd.geometry is geometry


def test_the_random_streams_are_the_c_ones():
    """nrf_rng_fill is the library's own generator: the restatement's uniforms on the two new streams equal it where a GPU is not needed -- the first values, computed
    from the header's formula by hand in Python integers"""
    def u32(seed, stream, idx):
        m = (1 << 64) - 1
        x = (seed + idx * 0x9E3779B97F4A7C15) & m
        x ^= (stream * 0xD1B54A32D192ED03) & m
        x ^= x >> 30
        x = (x * 0xBF58476D1CE4E5B9) & m
        x ^= x >> 27
        x = (x * 0x94D049BB133111EB) & m
        x ^= x >> 31
        return x >> 32
    for seed in (0, 7, 2 ** 63 + 5):
        for stream in (10, 11):
            idx = np.array([0, 1, 2, 1000, 2 ** 33 + 1], np.uint64)
            assert G.rng_u32(seed, stream, idx).tolist() == [u32(seed, stream, int(i)) for i in idx]
            u = G.rng_uniform(seed, stream, idx)
            assert u.dtype == F32 and (u >= 0).all() and (u < 1).all()


def test_workspace_sizes_and_refusals_need_no_gpu():
    """Every bad argument of the header is refused before anything touches the device, so the whole list is checked here; the GPU test repeats it over live buffers."""
    from nerfpp_amd import _lib
    lib = _lib.lib()
    fake = C.c_void_p(256)          # never dereferenced: every call below is refused
    big = 1 << 40
    box = np.array([0, 0, 0, 1, 1, 1], F32)
    pb = lambda a: a.ctypes.data_as(C.c_void_p)
    nan, inf = float("nan"), float("inf")

    def refused(name, status, fn, cases):
        for kw in cases:
            assert fn(**kw) == status, (name, kw)
            assert lib.nrf_last_error().startswith(name.encode()), (kw, lib.nrf_last_error())

    # sampling
    size = lib.nrf_mesh_sample_workspace_bytes
    assert size(258, 512) >= 32 + 2 * 512 * 4 + 2 * 2 * 8 and size(0, 0) > 0 and size(10, 512) == size(258, 512)
    for bad in ((-1, 1), (1, -1), (2 ** 31, 1), (1, 2 ** 31)):
        assert size(*bad) == 0, bad
    assert size(2 ** 31 - 1, 2 ** 31 - 1) > 2 ** 34

    def count(verts=fake, nv=4, faces=fake, nf=2, density=1.0, n=fake, area=fake, ws=fake, ws_bytes=big):
        return lib.nrf_mesh_sample_count(verts, nv, faces, nf, density, 0, n, area, None, ws, ws_bytes, None)

    refused("nrf_mesh_sample_count", INVALID_ARG, count, [dict(nv=-1), dict(nv=2 ** 31), dict(nf=-1), dict(nf=2 ** 31), dict(n=None), dict(area=None), dict(faces=None), dict(verts=None),
                                                         dict(density=-1.0), dict(density=nan), dict(density=inf), dict(ws=None), dict(ws=C.c_void_p(260))])
    refused("nrf_mesh_sample_count", WORKSPACE, count, [dict(ws_bytes=size(4, 2) - 1), dict(ws_bytes=0)])

    def emit(verts=fake, nv=4, faces=fake, nf=2, n=5, pts=fake, ws=fake, ws_bytes=big):
        return lib.nrf_mesh_sample_emit(verts, nv, faces, nf, 0, n, pts, None, None, ws, ws_bytes, None)

    refused("nrf_mesh_sample_emit", INVALID_ARG, emit, [dict(nv=-1), dict(nv=2 ** 31), dict(nf=-1), dict(nf=2 ** 31), dict(n=-1), dict(n=2 ** 31), dict(pts=None), dict(faces=None),
                                                       dict(verts=None), dict(nf=0), dict(nv=0), dict(ws=None), dict(ws=C.c_void_p(260))])
    refused("nrf_mesh_sample_emit", WORKSPACE, emit, [dict(ws_bytes=size(4, 2) - 1), dict(ws_bytes=0)])

    # nearest points
    size = lib.nrf_nearest_points_workspace_bytes
    assert size(100, 1000, 4, 5, 6) >= 121 * 4 + 120 * 4 + 1000 * 16 + 100 * 4 + 4 and size(0, 0, 1, 1, 1) > 0
    assert size(100, 1000, 4, 5, 6) == size(100, 1000, 6, 5, 4)
    for bad in ((-1, 1, 1, 1, 1), (1, -1, 1, 1, 1), (2 ** 31, 1, 1, 1, 1), (1, 2 ** 31, 1, 1, 1), (1, 1, 0, 1, 1), (1, 1, 1, 0, 1), (1, 1, 1, 1, 0), (1, 1, 1025, 1, 1),
                (1, 1, 1, 1025, 1), (1, 1, 1, 1, 1025), (1, 1, 1024, 1024, 65)):
        assert size(*bad) == 0, bad
    assert size(1, 1, 1024, 1024, 64) > 2 ** 29 and size(1, 1, 1024, 1, 1) > 0

    def nearest(q=fake, nq=3, t=fake, nt=5, b=pb(box), nx=2, ny=2, nz=2, md=inf, d2=fake, idx=fake, ws=fake, ws_bytes=big):
        return lib.nrf_nearest_points(q, nq, t, nt, b, nx, ny, nz, md, d2, idx, None, ws, ws_bytes, None)

    boxes = [np.array(b, F32) for b in ([0, 0, 0, 1, 0, 1], [0, 0, 0, 1, 1, -1], [0, nan, 0, 1, 1, 1], [0, 0, 0, inf, 1, 1], [-inf, 0, 0, 1, 1, 1],
                                        [-3e38, 0, 0, 3e38, 1, 1], [0, 0, 0, 1, 1e-42, 1])]
    refused("nrf_nearest_points", INVALID_ARG, nearest,
            [dict(nq=-1), dict(nq=2 ** 31), dict(nt=-1), dict(nt=2 ** 31), dict(nx=0), dict(ny=0), dict(nz=-1), dict(nx=1025), dict(ny=1025), dict(nz=1025),
             dict(nx=1024, ny=1024, nz=65), dict(q=None), dict(d2=None), dict(idx=None), dict(t=None), dict(b=None), dict(md=-1.0), dict(md=nan), dict(md=-inf), dict(ws=None),
             dict(ws=C.c_void_p(264))] + [dict(b=pb(b)) for b in boxes])
    refused("nrf_nearest_points", WORKSPACE, nearest, [dict(ws_bytes=size(3, 5, 2, 2, 2) - 1), dict(ws_bytes=0)])

    # statistics
    size = lib.nrf_distance_stats_workspace_bytes
    assert size(0) == size(1) == size(4096) > 0 and size(4097) >= 2 * 8 * 8 and size(-1) == 0 and size(2 ** 40) == 0
    taus = np.array([0.1, 0.2, 0.3, 0.4, 0.5], F32)

    def stats(d2=fake, n=10, t=pb(taus), n_tau=2, out=fake, ws=fake, ws_bytes=big):
        return lib.nrf_distance_stats(d2, n, t, n_tau, out, ws, ws_bytes, None)

    bad_taus = [np.array(t, F32) for t in ([0.1, -0.1], [nan, 0.1], [0.1, inf])]
    refused("nrf_distance_stats", INVALID_ARG, stats, [dict(n=-1), dict(n=2 ** 40), dict(n_tau=-1), dict(n_tau=5), dict(out=None), dict(d2=None), dict(t=None), dict(ws=None),
                                                      dict(ws=C.c_void_p(260))] + [dict(t=pb(t)) for t in bad_taus])
    refused("nrf_distance_stats", WORKSPACE, stats, [dict(ws_bytes=size(10) - 1), dict(ws_bytes=0)])


def test_samples_of_the_sphere_lie_in_its_shell(sphere):
    """A sample is a convex combination of its face's corners: it lies inside the circumscribed sphere (r_out) and beyond every face plane (r_in).  The three fp32
    operations per component move a point of norm < 1 by less than 3 * 2^-24 * sqrt(3) < 4e-7."""
    r_in, r_out = sphere_bounds(sphere["verts"], sphere["faces"])
    assert abs(r_in - 0.68931) < 1e-4 and abs(r_out - 0.7) < 1e-6
    for seed, (c, pts, face, uv) in sphere["samples"].items():
        rad = np.linalg.norm(pts.astype(np.float64) - CENTRE, axis=1)
        print(f"seed {seed}: {len(pts)} points, radius {rad.min():.6f} .. {rad.max():.6f}")
        assert len(pts) == c["n_points"] > 15000 and rad.min() >= r_in - 4e-7 and rad.max() <= r_out + 4e-7
        assert (uv >= 0).all() and (uv.sum(-1) <= 1).all() and np.array_equal(np.bincount(face, minlength=512), c["count"])
        assert c["stats"].tolist() == [0, 0, 0] and (np.diff(face) >= 0).all()
        # the point is the barycentric combination the (u, v) pair states
        tri = sphere["verts"][sphere["faces"][face]].astype(np.float64)
        u, v = uv[:, :1].astype(np.float64), uv[:, 1:].astype(np.float64)
        assert np.abs((1 - u - v) * tri[:, 0] + u * tri[:, 1] + v * tri[:, 2] - pts).max() < 4e-7


def test_the_count_follows_area_times_density(sphere):
    """n_f is floor(a) + Bernoulli(frac(a)): the total has mean area * density and a variance below the sum of frac (1 - frac) <= area * density, so 4 sqrt(area *
    density) is beyond four standard deviations.  The area of the sphere's mesh is a little under 4 pi r^2."""
    for seed, (c, *_) in sphere["samples"].items():
        mean = c["total_area"] * DENSITY
        print(f"seed {seed}: {c['n_points']} points, area * density {mean:.1f}, bound {4 * np.sqrt(mean):.1f}")
        assert abs(c["n_points"] - mean) <= 4 * np.sqrt(mean)
        assert 0.98 * 4 * np.pi * 0.49 < c["total_area"] < 4 * np.pi * 0.49
        area, valid, _ = G.face_areas(sphere["verts"], sphere["faces"])
        assert valid.all() and abs(c["total_area"] - area.astype(np.float64).sum()) < 1e-12
        assert np.abs(c["count"] - area * F32(DENSITY)).max() < 1
    zero = G.sample_count(sphere["verts"], sphere["faces"], 0.0, 0)
    assert zero["n_points"] == 0 and zero["total_area"] == sphere["samples"][0][0]["total_area"]


def test_degenerate_and_invalid_faces_get_no_points():
    verts, faces, kinds = G.adversarial_mesh()
    for density in (1.0, 50.0):
        c, pts, face, uv = G.sample(verts, faces, density, 3)
        for k in ("zero", "bad", "nonfinite"):
            assert (c["count"][kinds[k]] == 0).all(), k
        assert c["count"][kinds["clamped"]].tolist() == [G.SAMPLE_MAX_PER_FACE]
        assert c["stats"].tolist() == [3, 4, 1] and np.isfinite(pts).all() and len(pts) == c["n_points"]
        assert not np.isin(face, kinds["zero"] + kinds["bad"] + kinds["nonfinite"]).any()
    assert np.isfinite(c["total_area"]) and c["total_area"] > 1.8e5


def test_nearest_and_statistics_of_the_restatement():
    rng = np.random.default_rng(5)
    t = rng.uniform(-1, 1, (300, 3)).astype(F32)
    q = rng.uniform(-1, 1, (100, 3)).astype(F32)
    t[17] = t[3]                                             # a duplicate: the lower index wins
    q[0] = t[17]
    t[40, 1] = np.nan
    q[5, 2] = np.inf
    d2, idx, st = G.nearest(q, t)
    assert idx[0] == 3 and d2[0] == 0 and idx[5] == -1 and np.isinf(d2[5]) and st.tolist() == [1, 1]
    ok = np.isfinite(q).all(-1)
    dd = ((q[:, None].astype(np.float64) - np.where(np.isfinite(t), t, 1e9)[None]) ** 2).sum(-1)
    assert np.array_equal(idx[ok], dd.argmin(1)[ok]) and np.abs(d2[ok] - dd.min(1)[ok]).max() < 1e-6
    near = float(np.sqrt(np.sort(d2[ok])[20]))
    d2m, idxm, _ = G.nearest(q, t, max_dist=near)
    assert (idxm >= 0).sum() == 21 and np.array_equal(idxm[idxm >= 0], idx[idxm >= 0]) and np.isinf(d2m[idxm < 0]).all()
    taus = (0.05, near, 0.5)
    s = G.distance_stats(d2, taus)
    d = np.sqrt(d2[ok].astype(np.float64))
    assert s[0] == ok.sum() and abs(s[1] - d.sum()) < 1e-5 and abs(s[2] - d2[ok].astype(np.float64).sum()) < 1e-5 and abs(s[3] - d.max()) < 1e-7
    assert s[4:].tolist() == [(np.sqrt(d2[ok]) <= F32(x)).sum() for x in taus] and s[5] == 21, "an entry exactly at tau is within it"
    assert G.distance_stats(np.zeros(0, F32), (0.1,)).tolist() == [0, 0, 0, 0, 0]
    assert np.array_equal(G.distance_stats(d2m, taus)[4:], [min(s[4], 21), 21, 21])


def test_two_spheres_are_as_far_apart_as_their_shells(sphere):
    """A point of the 0.70 mesh has radius <= 0.70, a point of the 0.75 mesh has radius >= r_in(0.75): no directed distance is below the gap, and -- each mesh being
    sampled at about 20 k points -- none is far above the 0.05 the spheres are apart plus a sample spacing."""
    verts_b, faces_b = R.octa_sphere(T.SPHERE["centre"], 0.75)
    r_in_b, _ = sphere_bounds(verts_b, faces_b)
    gap = r_in_b - 0.70
    assert 0.038 < gap < 0.039
    pa = sphere["samples"][0][1][::8]
    pb = G.sample(verts_b, faces_b, DENSITY, 0)[1][::8]
    d_ab, d_ba = np.sqrt(G.nearest(pa, pb)[0]), np.sqrt(G.nearest(pb, pa)[0])
    print(f"gap {gap:.5f}; a->b {d_ab.min():.5f} .. {d_ab.max():.5f}; b->a {d_ba.min():.5f} .. {d_ba.max():.5f}")
    assert min(d_ab.min(), d_ba.min()) >= gap - 1e-6 and max(d_ab.max(), d_ba.max()) < 0.12
    s = G.surface_distance(pa, pb, taus=(0.03, 0.2))
    assert s["Precision"].tolist() == [0, 1] and s["Recall"].tolist() == [0, 1] and s["FScore"].tolist() == [0, 1]
    assert gap <= s["Accuracy"] <= s["Hausdorff"] and gap <= s["Completeness"] <= s["Hausdorff"] == max(d_ab.max(), d_ba.max())
    assert s["Chamfer"] == 0.5 * (s["Accuracy"] + s["Completeness"]) and s["ChamferSq"] >= 2 * gap * gap
    same = G.surface_distance(pa, pa, taus=(0.0, 0.01))
    assert same["Chamfer"] == 0 and same["Hausdorff"] == 0 and same["FScore"].tolist() == [1, 1]
