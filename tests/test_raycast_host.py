"""Ray casting on a mesh without a GPU: the definition (tests/raycast_ref.py, the numpy restatement the GPU tests compare nrf_ray_cast_mesh, nrf_hemisphere_dirs and
nrf_mesh_ambient_occlusion with bit for bit) pinned on an analytic sphere, on one triangle's vertices, edges and centroid, on the -0.0f rule and on the consistency
rule; the header, the binding, the constants, the sizes and every refusal of every entry (they come before any device call)."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np

import closest_ref as CR
import geometry_ref as G
import raster_ref as R
import raycast_ref as RC
import smooth_ref as S
import tsdf_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
INVALID_ARG, WORKSPACE = 1, 4
CENTRE = np.asarray(T.SPHERE["centre"], np.float64)
NAMES = [("nrf_ray_cast_workspace_bytes", ("z", "l")), ("nrf_ray_cast_mesh", ("i", "pliplplpiiillpziipppppppzp")), ("nrf_hemisphere_dirs", ("i", "pliqlppp")),
         ("nrf_mesh_ambient_occlusion", ("i", "ppliffqlplplpiiillpzpppzp"))]


def test_header_binding_and_constants_agree():
    from nerfpp_amd import _lib, geometry, raster, texture
    hdr = open(os.path.join(ROOT, "include", "nerfpp_hip.h")).read()
    rng = open(os.path.join(ROOT, "include", "nrf_rng.h")).read()

    def define(name):
        m = re.search(rf"#define\s+{name}\s+\(?(-?[\d.e+-]+)f?\)?", hdr)
        assert m, name
        return float(m[1])
    assert define("NRF_RC_CLOSEST") == 0 == geometry.RC_CLOSEST == RC.CLOSEST == _lib.NRF_RC_CLOSEST and define("NRF_RC_ANY") == 1 == geometry.RC_ANY == RC.ANY == _lib.NRF_RC_ANY
    for k, name in enumerate(("none", "back", "front")):
        assert define("NRF_RC_CULL_" + name.upper()) == k == geometry.RC_CULL[name] == (RC.CULL_NONE, RC.CULL_BACK, RC.CULL_FRONT)[k]
    assert define("NRF_RC_TAU_LOG2") == -12 == geometry.RC_TAU_LOG2 == RC.TAU_LOG2
    assert define("NRF_RC_MAX_STEPS") == 1024 == geometry.RC_MAX_STEPS == RC.MAX_STEPS and float(F32(1024)) == 1024, "(float)k is exact"
    assert define("NRF_RC_MAX_STRIDE") == 64 == geometry.RC_MAX_STRIDE == RC.MAX_STRIDE
    assert define("NRF_HEMI_ATTEMPTS") == 8 == geometry.HEMI_ATTEMPTS == RC.HEMI_ATTEMPTS and define("NRF_HEMI_MAX_K") == 65536 == geometry.HEMI_MAX_K == RC.HEMI_MAX_K
    assert re.search(r"#define\s+NRF_HEMI_MAX_INDEX\s+\(\(int64_t\)1 << 40\)", hdr) and geometry.HEMI_MAX_INDEX == RC.HEMI_MAX_INDEX == 1 << 40
    assert define("NRF_HEMI_MIN_LEN2") == 2.0 ** -20 == geometry.HEMI_MIN_LEN2 == float(RC.HEMI_MIN_LEN2)
    assert define("NRF_RNG_HEMI_DIR") == 12 == RC.RNG_HEMI_DIR == _lib.NRF_RNG_HEMI_DIR
    assert "12" not in dict(re.findall(r"(NRF_RNG_\w+)\s*=\s*(\d+)", rng)).values(), "a stream of its own: none of nrf_rng.h's ids"
    at = _lib.SYMBOLS.index("nrf_closest_on_mesh")
    assert _lib.SYMBOLS[at + 1:at + 5] == [n for n, _ in NAMES], "directly after nrf_closest_on_mesh, in the header's order"
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    for name, sig in NAMES:
        assert _lib.SIGNATURES[name] == sig and hasattr(lib, name) and re.search(rf"NRF_API (size_t|int) {name}\(", hdr), name
    for word in ("Ray casting on a mesh", "WHY THE WALK CANNOT MISS", "t = t + 0.0f", "The clip loses nothing", "FALLBACK", "HEMISPHERE DIRECTIONS", "AMBIENT OCCLUSION"):
        assert word in hdr, word
    for mod, names in ((geometry, ("RayCastMesh", "RayCastResult", "Occluded", "Visible", "HemisphereDirections", "AmbientOcclusion", "ClipRaysToMesh")),
                       (texture, ("BakeAmbientOcclusion",)), (raster, ("RayCastView",))):
        for name in names:
            assert hasattr(mod, name), name
    assert inspect.signature(texture.SaveOBJ).parameters["occlusion"].default is None
    p = inspect.signature(geometry.RayCastMesh).parameters
    assert p["near"].default == 0.0 and p["far"].default == float("inf") and p["cull"].default == "none" and p["uv"].default is True and p["points"].default is True
    assert inspect.signature(geometry.AmbientOcclusion).parameters["k"].default == 64 == inspect.signature(texture.BakeAmbientOcclusion).parameters["k"].default
    assert inspect.signature(geometry.ClipRaysToMesh).parameters["miss"].default == "keep"
    srcs = open(os.path.join(ROOT, "nerfpp_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\braycast\.hip\b", srcs, re.M) and re.search(r"^HDRS = .*\bface_grid\.h\b", srcs, re.M)


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
                                        [-3e38, 0, 0, 3e38, 1, 1], [0, 0, 0, 1, 1e-42, 1], [-3.4e38, 0, 0, -3.3e38, 1, 1])]          # the last: finite, its widening is not

    def refused(name, status, fn, cases):
        for kw in cases:
            assert fn(**kw) == status, (name, kw)
            assert lib.nrf_last_error().startswith(name.encode()), (kw, lib.nrf_last_error())

    size = lib.nrf_ray_cast_workspace_bytes
    assert size(0) >= 8 and size(1000) >= 4000 + 8 and size(-1) == 0 and size(2 ** 31) == 0
    good = lib.nrf_face_grid_bytes(2, 2, 2, 2, 10, 1)
    mesh_cases = [dict(nv=-1), dict(nv=2 ** 31), dict(nf=-1), dict(nf=2 ** 31), dict(nx=0), dict(ny=0), dict(nz=-1), dict(nx=1025), dict(ny=1025), dict(nz=1025),
                  dict(nx=1024, ny=1024, nz=65), dict(faces=None), dict(verts=None), dict(b=None), dict(ws=None), dict(ws=C.c_void_p(260))] + [dict(b=pb(b)) for b in boxes]
    grid_cases = [dict(n_refs=-1), dict(n_refs=2 ** 32), dict(n_large=-1), dict(n_large=3), dict(grid=None), dict(grid=C.c_void_p(260)), dict(grid_bytes=good - 1),
                  dict(grid_bytes=good + 256), dict(grid_bytes=0), dict(n_refs=1000), dict(nx=64)]

    def cast(rays=fake, n=3, stride=8, verts=fake, nv=4, faces=fake, nf=2, b=pb(box), nx=2, ny=2, nz=2, n_refs=10, n_large=1, grid=fake, grid_bytes=good, cull=0, mode=0,
             t=fake, face=fake, uv=None, point=None, hit=None, ws=fake, ws_bytes=big):
        return lib.nrf_ray_cast_mesh(rays, n, stride, verts, nv, faces, nf, b, nx, ny, nz, n_refs, n_large, grid, grid_bytes, cull, mode, t, face, uv, point, hit, None, ws,
                                     ws_bytes, None)

    any_ok = dict(mode=1, t=None, face=None, hit=fake)
    refused("nrf_ray_cast_mesh", INVALID_ARG, cast,
            mesh_cases + grid_cases + [dict(n=-1), dict(n=2 ** 31), dict(stride=7), dict(stride=0), dict(stride=65), dict(rays=None), dict(cull=-1), dict(cull=3),
                                       dict(mode=-1), dict(mode=2), dict(t=None), dict(face=None), dict(mode=1), dict(any_ok, hit=None), dict(any_ok, t=fake),
                                       dict(any_ok, face=fake), dict(any_ok, uv=fake), dict(any_ok, point=fake)])
    refused("nrf_ray_cast_mesh", WORKSPACE, cast, [dict(ws_bytes=size(3) - 1), dict(ws_bytes=0), dict(any_ok, ws_bytes=size(3) - 1)])

    def dirs(normals=fake, n=3, k=4, index0=0, out=fake):
        return lib.nrf_hemisphere_dirs(normals, n, k, 7, index0, out, None, None)

    refused("nrf_hemisphere_dirs", INVALID_ARG, dirs, [dict(n=-1), dict(n=2 ** 31), dict(k=0), dict(k=-1), dict(k=65537), dict(index0=-1), dict(index0=(1 << 40) - 2),
                                                       dict(n=2 ** 20, k=2 ** 11), dict(normals=None), dict(out=None)])
    assert dirs(n=0, normals=None, out=None) == 0 and dirs(n=0, index0=1 << 40) == 0

    def ao(points=fake, normals=fake, n=3, k=4, offset=0.0, md=1.0, index0=0, verts=fake, nv=4, faces=fake, nf=2, b=pb(box), nx=2, ny=2, nz=2, n_refs=10, n_large=1,
           grid=fake, grid_bytes=good, out=fake, ws=fake, ws_bytes=big):
        return lib.nrf_mesh_ambient_occlusion(points, normals, n, k, offset, md, 7, index0, verts, nv, faces, nf, b, nx, ny, nz, n_refs, n_large, grid, grid_bytes, out, None,
                                              ws, ws_bytes, None)

    refused("nrf_mesh_ambient_occlusion", INVALID_ARG, ao,
            mesh_cases + grid_cases + [dict(n=-1), dict(n=2 ** 31), dict(k=0), dict(k=65537), dict(index0=-1), dict(index0=(1 << 40) - 2), dict(offset=nan), dict(offset=inf),
                                       dict(md=-1.0), dict(md=nan), dict(md=-inf), dict(points=None), dict(normals=None), dict(out=None), dict(n=2 ** 30, k=2 ** 9)])
    refused("nrf_mesh_ambient_occlusion", WORKSPACE, ao, [dict(ws_bytes=size(3) - 1), dict(ws_bytes=0)])
    # n == 0 is valid and launches nothing, over pointers that are never dereferenced
    assert cast(n=0, rays=None, t=None, face=None) == 0 and ao(n=0, points=None, normals=None, out=None) == 0


@functools.lru_cache(maxsize=None)
def sphere_case(level):
    verts, faces = R.octa_sphere(T.SPHERE["centre"], T.SPHERE["radius"], level)
    rays, kinds = RC.mesh_rays(verts, faces, 10 + level)
    return verts, faces, rays, kinds, RC.cast(rays, verts, faces)


def test_a_sphere_seen_from_outside_is_hit_between_its_shells():
    """The mesh lies between the spheres of radii r_in and r_out about CENTRE, so a unit ray from radius rho aimed at the centre hits it at rho - r_out <= T <=
    rho - r_in; from inside the same with r - rho; culling the back faces changes nothing outside and removes everything inside."""
    verts, faces = R.octa_sphere(T.SPHERE["centre"], T.SPHERE["radius"], 3)
    r_in, r_out = R.face_plane_distances(verts, faces, CENTRE).min(), np.linalg.norm(verts.astype(np.float64) - CENTRE, axis=1).max()
    rng = np.random.default_rng(11)
    u = rng.standard_normal((300, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    for rho in (0.9, 2.0, 30.0):
        rays = RC.pack(CENTRE + rho * u, -u)
        out = RC.cast(rays, verts, faces)
        t = out["t"].astype(np.float64)
        print(f"rho {rho}: T {t.min():.6f} .. {t.max():.6f} within [{rho - r_out:.6f}, {rho - r_in:.6f}]")
        assert (out["face"] >= 0).all() and t.min() >= rho - r_out - 1e-5 * rho and t.max() <= rho - r_in + 1e-5 * rho
        tri = verts[faces[out["face"]]].astype(np.float64)
        v, w = out["uv"][:, :1].astype(np.float64), out["uv"][:, 1:].astype(np.float64)
        assert np.abs((1 - v - w) * tri[:, 0] + v * tri[:, 1] + w * tri[:, 2] - out["point"]).max() < 1e-6
        assert np.abs(rays[:, :3].astype(np.float64) + t[:, None] * rays[:, 3:6] - out["point"]).max() < 1e-5 * rho
        back = RC.cast(rays, verts, faces, cull=RC.CULL_BACK)
        assert np.array_equal(back["t"], out["t"]) and np.array_equal(back["face"], out["face"]), "the faces are counter-clockwise seen from outside"
        front = RC.cast(rays, verts, faces, cull=RC.CULL_FRONT)
        assert (front["face"] >= 0).all() and (front["t"].astype(np.float64) >= rho + r_in - 1e-5 * rho).all(), "only the far side is left"
    inside = RC.cast(RC.pack(CENTRE + 0.1 * u, u[::-1].copy()), verts, faces)
    assert (inside["face"] >= 0).all() and inside["t"].min() >= r_in - 0.1 - 1e-5 and inside["t"].max() <= r_out + 0.1 + 1e-5
    assert (RC.cast(RC.pack(CENTRE + 0.1 * u, u[::-1].copy()), verts, faces, cull=RC.CULL_BACK)["face"] == -1).all()
    # a finite far before the surface, at it and beyond it
    rays = RC.pack(CENTRE + 2.0 * u, -u)
    t = RC.cast(rays, verts, faces)["t"]
    for far, hits in ((t, True), (np.nextafter(t, F32(0)), False), (t + F32(0.5), True)):
        rays[:, 7] = far
        assert (RC.cast(rays, verts, faces)["hit"] == hits).all()
    rays[:, 6], rays[:, 7] = np.nextafter(t, F32(9)), np.inf          # near just behind the first hit: the far side
    assert (RC.cast(rays, verts, faces)["t"] > t + F32(1)).all()


def test_vertices_edge_midpoints_and_centroids_and_the_lowest_face_of_a_tie():
    a, b, c = (np.array(x, F32) for x in ([0.5, -1, 2], [1.5, 0, 2.5], [0, 1, 1]))
    half = F32(0.5)
    o = np.array([0.25, 0.5, 9.0], F32)
    cases = [(a, (0, 0)), (b, (1, 0)), (c, (0, 1)), (half * (a + b), (0.5, 0)), (half * (a + c), (0, 0.5)), (half * (b + c), (0.5, 0.5)),
             (((a.astype(np.float64) + b + c) / 3).astype(F32), (1 / 3, 1 / 3))]
    for target, uv in cases:
        r = RC.candidate(o, target - o, F32(0), RC.INF, a, b, c)
        assert r["ok"] and abs(r["v"] - uv[0]) < 2e-6 and abs(r["w"] - uv[1]) < 2e-6 and abs(r["t"] - 1) < 2e-6 and np.abs(r["p"] - target).max() < 2e-6, (uv, r)
    # on the mesh: a ray aimed exactly at a vertex or an edge midpoint reports the lowest face among those that accept it at the smallest t
    verts, faces, rays, kinds, want = sphere_case(2)
    ta, tb, tc = (verts[faces[:, k]] for k in range(3))
    checked = 0
    for name in ("vertex", "edge"):
        for k in range(kinds[name].start, kinds[name].stop, 5):
            o_, d_, lo, hi, _ = RC.ray_parts(rays[k:k + 1])
            r = RC.candidate(o_, d_, lo, hi, ta, tb, tc)
            if not r["ok"].any():
                assert want["face"][k] == -1
                continue
            tmin = r["t"][r["ok"]].min()
            tied = np.flatnonzero(r["ok"] & (r["t"] == tmin))
            assert want["face"][k] == tied.min() and want["t"][k] == tmin
            checked += len(tied) > 1
    print(f"{checked} rays of the sample tie exactly between two or more faces")
    assert checked > 0, "the lowest-face rule is exercised on a real mesh, not on the constructed case alone"
    # an exact tie by construction: two faces share the edge x = 0, the ray meets it head-on in exact arithmetic
    v4 = np.array([[0, -1, 0], [0, 1, 0], [1, 0, 0], [-1, 0, 0]], F32)
    for f2 in (np.array([[0, 1, 2], [1, 0, 3]], np.int32), np.array([[1, 0, 3], [0, 1, 2]], np.int32)):
        out = RC.cast(RC.pack([[0, 0.25, 2]], [[0, 0, -1]]), v4, f2)
        assert out["t"][0] == 2 and out["face"][0] == 0, "both faces accept at t = 2: the lower index wins whichever face it is"


def test_a_ray_that_starts_in_a_faces_plane_needs_the_minus_zero_rule():
    """o on the face, d leaving it towards a second face behind: t of the first face is -0.0f before the rule for half of the directions, and as bits -0.0f is above
    every positive t, so without `t + 0.0f` the face behind would win"""
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, -1], [1, 0, -1], [0, 1, -1]], F32)
    faces = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    rays = RC.pack([[0.25, 0.25, 0]] * 2, [[0, 0, -1], [0, 0, 1]])
    a, b, c = (verts[faces[0, k]] for k in range(3))
    raw = []
    with np.errstate(all="ignore"):
        for d in rays[:, 3:6]:
            ab, ac, tv = b - a, c - a, rays[0, :3] - a
            p = RC._cross(d, ac)
            inv = F32(1) / RC._dot(ab, p)
            raw.append(RC._dot(ac, RC._cross(tv, ab)) * inv)
    assert any(np.signbit(x) and x == 0 for x in raw), "the unruled t is -0.0f for one of the two directions"
    out = RC.cast(rays, verts, faces)
    assert out["face"].tolist() == [0, 0] and out["t"].tolist() == [0, 0] and not np.signbit(out["t"]).any()
    assert np.uint32(0x80000000) > F32(1).view(np.uint32), "the key of -0.0f lies above that of 1.0f"
    # the shared set holds such rays too, so the GPU comparison cannot skip the rule
    _, _, rays, kinds, want = sphere_case(2)
    s = kinds["plane"]
    assert (want["t"][s] == 0).sum() >= 20 and not np.signbit(want["t"]).any()


def test_the_consistency_rule_rejects_nothing_on_the_ordinary_sets():
    """|Pu - P|_inf / max(|o|_inf, |Pu|_inf) over every candidate that passes the other tests: far below 2^-12 on every kind of ray but those that lie IN a face's
    plane, whose det is a rounding error and whose t means nothing -- the only hits the rule removes"""
    worst = 0.0
    for level in (1, 2, 3):
        verts, faces, rays, kinds, _ = sphere_case(level)
        for shift in (0.0, 100.0):
            for name, s in kinds.items():
                if name in ("plane", "invalid", "empty"):
                    continue
                r = rays[s].copy()
                r[:, :3] += F32(shift)
                out = RC.cast(r, (verts + F32(shift)).astype(F32), faces)
                assert out["rejected"] == 0, (level, shift, name)
                worst = max(worst, out["ratio"])
    print(f"worst ratio on the ordinary sets 2^{np.log2(worst):.1f}")
    assert worst <= 2.0 ** RC.TAU_LOG2          # what "nothing rejected" means; the printed margin is what the header quotes
    verts, faces, rays, kinds, _ = sphere_case(3)
    for tau_log2 in (-14, -16):
        assert RC.cast(rays[kinds["outside"]], verts, faces, tau_log2=tau_log2)["rejected"] == 0
    plane = RC.cast(rays[kinds["plane"]], verts, faces)
    print(f"in-plane rays: {plane['rejected']} candidates rejected, worst ratio 2^{np.log2(max(plane['ratio'], 1e-30)):.1f}")
    # grazing rays: tangent to the sphere within 0.5 % of its radius
    rng = np.random.default_rng(5)
    u = rng.standard_normal((1000, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    tang = np.cross(u, rng.standard_normal((1000, 3)))
    tang /= np.linalg.norm(tang, axis=1, keepdims=True)
    o = CENTRE + T.SPHERE["radius"] * rng.uniform(0.995, 1.0, (1000, 1)) * u - 3 * tang
    graze = RC.cast(RC.pack(o, tang), verts, faces)
    print(f"grazing rays: {int(graze['hit'].sum())} hits, {graze['rejected']} rejected, worst ratio 2^{np.log2(max(graze['ratio'], 1e-30)):.1f}")
    assert graze["rejected"] == 0 and graze["hit"].sum() > 100


def test_hemisphere_directions_are_unit_cosine_weighted_and_slab_free():
    rng = np.random.default_rng(0)
    n = (rng.standard_normal((1500, 3)) * 10.0 ** rng.uniform(-3, 3, (1500, 1))).astype(F32)
    d, bad = RC.hemisphere_dirs(n, 32, seed=3, index0=5)
    nh, ok = RC.unit_normals(n)
    cos = (d.astype(np.float64) * nh[:, None].astype(np.float64)).sum(-1)
    assert bad == 0 and ok.all() and np.abs(np.linalg.norm(d.astype(np.float64), axis=-1) - 1).max() < 3e-7 and cos.min() >= 0
    assert abs(cos.mean() - 2 / 3) < 0.005, "the cosine law: E[cos] = 2 / 3 (a uniform hemisphere gives 1 / 2)"
    assert abs((cos ** 2).mean() - 1 / 2) < 0.005, "E[cos^2] = 1 / 2"
    # a pure function of (seed, index0 + i, j): a slab of the list draws what the whole list does, and k does not move direction j
    part, _ = RC.hemisphere_dirs(n[100:200], 32, seed=3, index0=105)
    fewer, _ = RC.hemisphere_dirs(n, 7, seed=3, index0=5)
    assert np.array_equal(part.view(np.uint32), d[100:200].view(np.uint32)) and np.array_equal(fewer.view(np.uint32), d[:, :7].view(np.uint32))
    assert not np.array_equal(RC.hemisphere_dirs(n, 32, seed=4, index0=5)[0], d)
    # bad normals: zeros, counted
    z, bad = RC.hemisphere_dirs(np.array([[0, 0, 0], [np.nan, 0, 1], [np.inf, 0, 0], [3e19, 3e19, 0], [1e-30, 0, 0], [0, 0, 2]], F32), 4)
    assert bad == 5 and (z[:5] == 0).all() and np.abs(np.linalg.norm(z[5], axis=-1) - 1).max() < 3e-7


def test_ambient_occlusion_of_a_convex_sphere_and_invalid_faces():
    verts, faces = R.octa_sphere(T.SPHERE["centre"], T.SPHERE["radius"], 2)
    out_n = (verts.astype(np.float64) - CENTRE).astype(F32)
    ao, invalid = RC.ambient_occlusion(verts, out_n, 16, 1e-3, 5.0, verts, faces, seed=1)
    assert invalid == 0 and (ao == 1).all(), "nothing lies above a convex surface"
    ao, invalid = RC.ambient_occlusion(verts, -out_n, 16, 1e-3, 5.0, verts, faces, seed=1)
    assert invalid == 0 and (ao == 0).all(), "inside, every ray meets the far side within max_dist"
    ao, invalid = RC.ambient_occlusion(verts[:3], np.zeros((3, 3), F32), 16, 1e-3, 5.0, verts, faces)
    assert invalid == 48 and (ao == 1).all()
    # invalid faces never win
    v, f, kinds = G.adversarial_mesh()
    rays, _ = RC.mesh_rays(v[:4], f[:4], 2, n=60)
    out = RC.cast(rays, v, f)
    assert out["stats"].tolist() == [7, 3, 3, 0] and not np.isin(out["face"], kinds["bad"] + kinds["nonfinite"][:3]).any() and (out["face"] >= 0).sum() > 100
    v, f = S.dirty()
    rays, _ = RC.mesh_rays(v[:5], f[:3], 4, n=60)
    out = RC.cast(rays, v, f)
    assert out["stats"].tolist() == [7, 3, 5, 0] and (out["face"] >= 0).sum() > 50
    valid = CR.face_classes(v, f)[0] == 0
    assert valid[out["face"][out["face"] >= 0]].all()


def test_clip_rays_arithmetic():
    rays = RC.pack(np.zeros((4, 3)), np.ones((4, 3)), near=[0.0, 0.5, 0.0, 0.2], far=[9.0, 0.875, np.inf, 3.0])
    t = np.array([1.0, 0.75, np.inf, 2.0], F32)
    keep = RC.clip_rays(rays, t, 0.25)
    assert keep[:, 6].tolist() == [0.75, 0.5, 0.0, 1.75] and keep[:, 7].tolist() == [1.25, 0.875, np.inf, 2.25]
    empty = RC.clip_rays(rays, t, 0.25, miss="empty")
    assert empty[2, 6:8].tolist() == [1, 0] and np.array_equal(empty[[0, 1, 3]], keep[[0, 1, 3]]) and np.array_equal(keep[:, :6], rays[:, :6])
