"""The mesh rasteriser on the MI355X: nrf_raster_mesh against the numpy restatement (tests/raster_ref.py) bit for bit -- depth, face, barycentrics, attributes and
statistics -- on shared edges, a closed mesh, an adversarial mesh and meshes that take both face kernels; the permutation and run-to-run guarantees, the refusals,
and the Python layer built on it: RenderMesh, RenderMeshView, VisibleFaces, FilterVisible and EvaluateMesh."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import raster_ref as R
import tsdf_ref as T

pytestmark = pytest.mark.gpu

INVALID_ARG = 1
F32 = np.float32
K_SPHERE = np.array([[70.0, 0, 29.3], [0, 62.5, 22.6], [0, 0, 1]], F32)          # fx != fy, principal point off-centre
IDENTITY = R.LATTICE_POSE


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from nerfpp_amd import _lib as L, mesh, raster, scene
    return L, raster, mesh, scene


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, F32).view(np.uint32)


def ptr(a):
    return np.ascontiguousarray(a, F32).ctypes.data_as(C.c_void_p)


def run(api, verts, faces, attr, h, w, K, c2w, near=1e-3, cull=0, skip=(), stats=None, workspace=None):
    """The C entry itself -> dict of numpy arrays (None for the outputs named in `skip`: they are passed as NULL); stats: a device tensor to add to"""
    lib = api[0].lib()
    dv = torch.from_numpy(np.ascontiguousarray(verts, F32).reshape(-1, 3)).cuda()
    df = torch.from_numpy(np.ascontiguousarray(faces, np.int32).reshape(-1, 3)).cuda()
    n_attr = 0 if attr is None else int(np.asarray(attr).reshape(len(verts), -1).shape[1])
    da = None if n_attr == 0 else torch.from_numpy(np.ascontiguousarray(attr, F32).reshape(len(verts), n_attr)).cuda()
    depth = torch.full((h, w), -7.0, device="cuda")
    face = None if "face" in skip else torch.full((h, w), -7, dtype=torch.int32, device="cuda")
    bary = None if "bary" in skip else torch.full((h, w, 3), -7.0, device="cuda")
    out = None if n_attr == 0 else torch.full((h, w, n_attr), -7.0, device="cuda")
    if stats is None and "stats" not in skip:
        stats = torch.zeros((4,), dtype=torch.int32, device="cuda")
    need = int(lib.nrf_raster_workspace_bytes(len(dv), len(df), h, w))
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda") if workspace is None else workspace
    p = lambda t: None if t is None else t.data_ptr()
    status = lib.nrf_raster_mesh(p(dv), len(dv), p(df), len(df), p(da), n_attr, h, w, ptr(np.asarray(K, F32).reshape(9)), ptr(np.asarray(c2w, F32)[:3, :4].reshape(12)),
                                 near, cull, p(depth), p(face), p(bary), p(out), p(stats), p(ws), ws.numel(), None)
    assert status == 0, lib.nrf_last_error()
    torch.cuda.synchronize()
    n = lambda t: None if t is None else t.cpu().numpy()
    return dict(depth=n(depth), face=n(face), bary=n(bary), attr=n(out), stats=None if stats is None else n(stats).view(np.uint32))


def assert_equal(got, want, what=""):
    for k in ("depth", "bary", "attr"):
        if got[k] is not None:
            assert np.array_equal(bits(got[k]), bits(want[k])), f"{what}: {k}"
    if got["face"] is not None:
        assert np.array_equal(got["face"], want["face"]), f"{what}: face"
    if got["stats"] is not None:
        assert np.array_equal(got["stats"], want["stats"]), f"{what}: stats {got['stats']} != {want['stats']}"


def attributes(n_verts, seed=7):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n_verts, 8)).astype(F32)


def sliced(ref, n_attr):
    """The reference of 8 attributes serves every smaller count: a channel does not depend on the others"""
    return dict(ref, attr=None if n_attr == 0 else ref["attr"][..., :n_attr])


@functools.lru_cache(maxsize=None)
def scene_case(name):
    from nerfpp_amd import scene
    s = T.SPHERE
    if name == "sphere":
        verts, faces = R.octa_sphere(s["centre"], s["radius"])
        return verts, faces, s["h"], s["w"], K_SPHERE, scene.pose_spherical(67.0, -35.0, 4.0)
    verts, faces = R.lattice_mesh(float(name))
    return verts, faces, R.LATTICE_H, R.LATTICE_W, R.LATTICE_K, IDENTITY


@functools.lru_cache(maxsize=None)
def reference(name, cull):
    verts, faces, h, w, K, c2w = scene_case(name)
    return R.rasterize(verts, faces, attributes(len(verts)), h, w, K, c2w, cull=cull)


# ------------------------------------------------------------------------------------ 1. against the restatement
@pytest.mark.parametrize("n_attr", [0, 1, 3, 8])
@pytest.mark.parametrize("cull", [0, 1])
@pytest.mark.parametrize("name", ["sphere", "0.25", "0.375", "0.5"])
def test_equals_the_restatement_bit_for_bit(api, name, cull, n_attr):
    verts, faces, h, w, K, c2w = scene_case(name)
    want = sliced(reference(name, cull), n_attr)
    assert (want["face"] >= 0).sum() >= 20 and want["stats"][0] > 0 and (cull == 0 or want["stats"][2] > 0)
    attr = None if n_attr == 0 else attributes(len(verts))[:, :n_attr]
    assert_equal(run(api, verts, faces, attr, h, w, K, c2w, cull=cull), want, f"{name} cull {cull} attr {n_attr}")


@pytest.mark.parametrize("skip", ["face", "bary", "stats", ("face", "bary", "stats")])
def test_optional_outputs_may_be_null(api, skip):
    verts, faces, h, w, K, c2w = scene_case("sphere")
    skip = (skip,) if isinstance(skip, str) else skip
    for n_attr in (0, 3):
        got = run(api, verts, faces, None if n_attr == 0 else attributes(len(verts))[:, :n_attr], h, w, K, c2w, skip=skip)
        assert all(got[k] is None for k in skip)
        assert_equal(got, sliced(reference("sphere", 0), n_attr), f"without {skip}, {n_attr} attributes")


# ------------------------------------------------------------------------------------ 2. the adversarial mesh
ADV_H, ADV_W, ADV_NEAR = 20, 24, 0.5
ADV_K = np.array([[8.0, 0, 11.25], [0, 7.25, 9.5], [0, 0, 1]], F32)


def adversarial():
    """Camera at the origin looking down -z (identity pose): a point (x, y, -zd) lands at u = 8 x / zd + 11.25, v = 9.5 - 7.25 y / zd.  -> (verts, faces, the vertex ids
    by name)"""
    rng = np.random.default_rng(11)
    v, f, ids = [], [], {}

    def add(name, *p):
        ids[name] = len(v)
        v.append(p)
        return ids[name]
    # a cloud of ordinary triangles over the image, depths 1 .. 3
    for _ in range(60):
        zd = rng.uniform(1.0, 3.0, 3)
        u, vv = rng.uniform(-2, ADV_W + 2, 3), rng.uniform(-2, ADV_H + 2, 3)
        base = len(v)
        for k in range(3):
            v.append(((u[k] - 11.25) / 8.0 * zd[k], -(vv[k] - 9.5) / 7.25 * zd[k], -zd[k]))
        f.append((base, base + 1, base + 2))
    a, b = 0, 1                                                            # two ordinary vertices to hang the special ones on
    f.append((a, b, add("behind", 0.3, 0.2, 1.0)))                         # zd = -1
    f.append((a, b, add("at_near", 0.1, 0.1, -0.5)))                       # zd == near_z exactly: clipped (zd > near_z is required)
    f.append((a, b, add("past_near", 0.1, 0.1, float(np.nextafter(F32(-0.5), F32(-1))))))          # the next float: drawn
    f.append((a, b, add("nan", np.nan, 0.0, -1.0)))
    f.append((a, b, add("inf", np.inf, 0.0, -1.0)))
    f.append((a, b, add("ninf", 0.0, -np.inf, -1.0)))
    x_in, x_neg = F32(2046.59375), F32(-2049.40625)                        # 8 x + 11.25 == +-16384 exactly at zd = 1

    def first_beyond(x, towards):
        """the first float past x whose u, formed in fp32, leaves [-16384, 16384]"""
        while abs(F32(8) * x + F32(11.25)) <= F32(16384):
            x = np.nextafter(x, F32(towards))
        return float(x)
    f.append((a, b, add("u_in", float(x_in), 0.0, -1.0)))
    f.append((a, b, add("u_out", first_beyond(x_in, 1e9), 0.0, -1.0)))
    f.append((a, b, add("u_neg_in", float(x_neg), 0.0, -1.0)))
    f.append((a, b, add("u_neg_out", first_beyond(x_neg, -1e9), 0.0, -1.0)))
    f += [(a, a, b), (b, b, b)]                                            # zero area by repeated indices
    c0 = add("col0", -1.0, 0.5, -2.0); c1 = add("col1", 0.0, 0.5, -2.0); c2 = add("col2", 1.0, 0.5, -2.0)
    f.append((c0, c1, c2))                                                 # zero area by three collinear vertices
    f += [(a, b, -1), (len(v) + 40, a, b)]                                 # bad indices (the second is fixed to V below)
    o = [add("off%d" % k, 20.0 + k, 3.0 * k, -2.0) for k in range(3)]      # u = 91 .. 99: wholly right of the image
    f.append(tuple(o))
    p = add("on_centre", (5 - 11.25) / 8.0, -(7 - 9.5) / 7.25 * 1.0, -1.0)          # u = 5, v = 7 exactly
    f += [(p, a, b), (b, p, c1)]
    f += [f[3], f[3], f[7][::-1]]                                          # coincident duplicates, one with the other winding
    verts = np.array(v, F32)
    faces = np.array(f, np.int64)
    faces[faces == len(v) + 40] = len(v)
    return verts, faces.astype(np.int32), ids


def test_adversarial_mesh_equals_the_restatement(api):
    verts, faces, ids = adversarial()
    X, Y, zd, ok = R.project(verts, ADV_K, IDENTITY, ADV_NEAR)
    expect = dict(behind=False, at_near=False, past_near=True, nan=False, inf=False, ninf=False, u_in=True, u_out=False, u_neg_in=True, u_neg_out=False, on_centre=True)
    assert {k: bool(ok[ids[k]]) for k in expect} == expect
    assert zd[ids["at_near"]] == F32(ADV_NEAR) and X[ids["u_in"]] == 16384 * 256 and X[ids["u_neg_in"]] == -16384 * 256
    assert (X[ids["on_centre"]], Y[ids["on_centre"]]) == (5 * 256, 7 * 256)
    attr = attributes(len(verts))[:, :3]
    for cull in (0, 1):
        want = R.rasterize(verts, faces, attr, ADV_H, ADV_W, ADV_K, IDENTITY, near_z=ADV_NEAR, cull=cull)
        print(cull, want["stats"], int((want["face"] >= 0).sum()))
        assert (want["stats"] > 0).all() and want["stats"][3] == 2 and want["stats"][1] == 7 and int(want["stats"].sum()) == len(faces)
        assert_equal(run(api, verts, faces, attr, ADV_H, ADV_W, ADV_K, IDENTITY, near=ADV_NEAR, cull=cull), want, f"adversarial, cull {cull}")
    wide = R.bbox_pixels(verts, faces, ADV_H, ADV_W, ADV_K, IDENTITY, ADV_NEAR)
    assert (wide > 256).any() and ((wide > 0) & (wide <= 256)).any(), "the faces that reach to u = +-16384 take the wide kernel"


def test_one_pixel_image_and_empty_face_list(api):
    verts, faces, _ = adversarial()
    K1 = np.array([[8.0, 0, 0.25], [0, 7.25, 0.5], [0, 0, 1]], F32)
    want = R.rasterize(verts, faces, None, 1, 1, K1, IDENTITY, near_z=ADV_NEAR)
    assert want["face"][0, 0] >= 0
    assert_equal(run(api, verts, faces, None, 1, 1, K1, IDENTITY, near=ADV_NEAR), want, "1 x 1")
    for v in (verts, verts[:0]):
        got = run(api, v, faces[:0], None if len(v) == 0 else attributes(len(v))[:, :2], 5, 7, ADV_K, IDENTITY)
        assert (got["depth"] == 0).all() and (got["face"] == -1).all() and (got["bary"] == 0).all() and (got["stats"] == 0).all(), "F = 0 writes the background"
        assert got["attr"] is None or (got["attr"] == 0).all()
    # every face bad: V = 0 with faces
    got = run(api, verts[:0], faces, None, 5, 7, ADV_K, IDENTITY)
    assert (got["face"] == -1).all() and got["stats"].tolist() == [0, 0, 0, len(faces)]


# ------------------------------------------------------------------------------------ 3. both kernels
def from_screen(u, v, zd, K):
    return (u - K[0, 2]) / K[0, 0] * zd, -(v - K[1, 2]) / K[1, 1] * zd, -zd


def quad_and_cloud(quad_zd, n=1500, seed=5):
    """64 x 48: a cloud of sub-pixel triangles at depths 1.5 .. 2.5 and a full-screen quad of two triangles at quad_zd, the quad's faces in the middle of the list"""
    h, w = 48, 64
    K = np.array([[60.0, 0, 31.5], [0, 55.0, 24.25], [0, 0, 1]], F32)
    rng = np.random.default_rng(seed)
    v, f = [], []
    for _ in range(n):
        u0, v0, zd = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(1.5, 2.5)
        for k in range(3):
            v.append(from_screen(u0 + rng.uniform(-0.6, 0.6), v0 + rng.uniform(-0.6, 0.6), zd + rng.uniform(-0.05, 0.05), K))
        f.append((len(v) - 3, len(v) - 2, len(v) - 1))
    q = len(v)
    for u0, v0 in ((-3.0, -2.0), (w + 2.0, -2.0), (w + 2.0, h + 1.0), (-3.0, h + 1.0)):
        v.append(from_screen(u0, v0, quad_zd, K))
    f[n // 2:n // 2] = [(q, q + 1, q + 2), (q, q + 2, q + 3)]
    return np.array(v, F32), np.array(f, np.int32), h, w, K


@pytest.mark.parametrize("quad_zd", [3.0, 1.0, 2.0])
def test_full_screen_faces_among_sub_pixel_faces(api, quad_zd):
    """The quad behind, in front of and inside the cloud: its two faces take the wide kernel, the cloud the scan of one lane per face, on one z-buffer.  The permuted
    face list gives the same depth bits."""
    raster = api[1]
    verts, faces, h, w, K = quad_and_cloud(quad_zd)
    area = R.bbox_pixels(verts, faces, h, w, K, IDENTITY)
    assert (area > raster.WIDE_PIXELS).sum() == 2 and area.max() == h * w and (area[area <= raster.WIDE_PIXELS] <= 9).all()
    attr = attributes(len(verts))[:, :3]
    want = R.rasterize(verts, faces, attr, h, w, K, IDENTITY)
    quad = np.isin(want["face"], np.nonzero(area > raster.WIDE_PIXELS)[0])
    hidden = len(faces) - len(np.unique(want["face"]))          # faces that own no pixel
    print(quad_zd, float(quad.mean()), hidden)
    assert (want["face"] >= 0).all() and (quad.all() if quad_zd == 1.0 else 0 < quad.mean() < 1), quad.mean()
    assert_equal(run(api, verts, faces, attr, h, w, K, IDENTITY), want, f"quad at {quad_zd}")
    perm = np.random.default_rng(9).permutation(len(faces))
    got = run(api, verts, faces[perm], attr, h, w, K, IDENTITY)
    assert np.array_equal(bits(got["depth"]), bits(want["depth"])), "the order of the faces does not matter"
    assert_equal(got, R.rasterize(verts, faces[perm], attr, h, w, K, IDENTITY), "permuted")


def test_faces_at_the_threshold_between_the_kernels(api):
    """Clamped bounding boxes of WIDE_PIXELS - 1, WIDE_PIXELS and WIDE_PIXELS + 1 pixels.  257 is prime, so that box is one row of a 300 x 4 image (with 255 x 1 and
    256 x 1 beside it); 15 x 17, 16 x 16 and 43 x 6 stand in a 64 x 48 image, one of them clamped by the image's edge."""
    raster = api[1]
    assert raster.WIDE_PIXELS == 256
    K = np.array([[50.0, 0, 0.0], [0, 50.0, 0.0], [0, 0, 1]], F32)

    def tri(u0, v0, nu, nv, zd):
        """a right triangle whose box covers the pixel columns u0 .. u0 + nu - 1 and rows v0 .. v0 + nv - 1"""
        lo_u, hi_u, lo_v, hi_v = u0 - 0.25, u0 + nu - 0.75, v0 - 0.25, v0 + nv - 0.75
        return [from_screen(lo_u, lo_v, zd, K), from_screen(hi_u, lo_v, zd * 1.25, K), from_screen(lo_u, hi_v, zd * 0.75, K)]
    for (h, w), boxes, areas in (((4, 300), [(3, 0, 255, 1), (2, 1, 256, 1), (1, 2, 257, 1), (0, 3, 300, 1)], [255, 256, 257, 300]),
                                ((48, 64), [(2, 3, 15, 17), (20, 5, 16, 16), (-5, 30, 48, 6), (50, 40, 30, 30)], [255, 256, 258, 14 * 8])):
        verts = np.array([p for k, b in enumerate(boxes) for p in tri(*b, zd=2.0 + 0.1 * k)], F32)
        faces = np.arange(len(verts), dtype=np.int32).reshape(-1, 3)
        assert R.bbox_pixels(verts, faces, h, w, K, IDENTITY).tolist() == areas
        attr = attributes(len(verts))[:, :1]
        want = R.rasterize(verts, faces, attr, h, w, K, IDENTITY)
        assert set(np.unique(want["face"])) >= {0, 1, 2, 3}
        assert_equal(run(api, verts, faces, attr, h, w, K, IDENTITY), want, f"{h} x {w}")


# ------------------------------------------------------------------------------------ 4. repeatability
def test_two_runs_agree_and_statistics_accumulate(api):
    verts, faces, h, w, K = quad_and_cloud(2.0, n=3000, seed=6)
    attr = attributes(len(verts))
    stats = torch.zeros((4,), dtype=torch.int32, device="cuda")
    a = run(api, verts, faces, attr, h, w, K, IDENTITY, cull=0, stats=stats)
    once = a["stats"].copy()
    b = run(api, verts, faces, attr, h, w, K, IDENTITY, cull=0, stats=stats)
    for k in ("depth", "bary", "attr"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert np.array_equal(a["face"], b["face"])
    assert int(once.sum()) == len(faces) and np.array_equal(b["stats"], 2 * once), "d_stats is added to"


# ------------------------------------------------------------------------------------ 5. refusals
def test_c_entry_refuses_bad_arguments_and_touches_nothing(api):
    lib = api[0].lib()
    verts, faces, h, w, K, c2w = scene_case("sphere")
    dv, df = torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda()
    da = torch.from_numpy(attributes(len(verts))[:, :3].copy()).cuda()
    need = int(lib.nrf_raster_workspace_bytes(len(verts), len(faces), h, w))
    depth, bary, out = torch.full((h, w), 7.0, device="cuda"), torch.full((h, w, 3), 7.0, device="cuda"), torch.full((h, w, 3), 7.0, device="cuda")
    face, stats = torch.full((h, w), 7, dtype=torch.int32, device="cuda"), torch.full((4,), 7, dtype=torch.int32, device="cuda")
    ws = torch.full((need,), 7, dtype=torch.uint8, device="cuda")
    k9, m12 = np.ascontiguousarray(K.reshape(9)), np.ascontiguousarray(np.asarray(c2w, F32).reshape(12))
    P = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(verts=dv.data_ptr(), nv=len(verts), faces=df.data_ptr(), nf=len(faces), attr=da.data_ptr(), n_attr=3, h=h, w=w, k=P(k9), m=P(m12), near=1e-3, cull=0,
             depth=depth.data_ptr(), out=out.data_ptr(), ws=ws.data_ptr(), ws_bytes=need):
        return lib.nrf_raster_mesh(verts, nv, faces, nf, attr, n_attr, h, w, k, m, near, cull, depth, face.data_ptr(), bary.data_ptr(), out, stats.data_ptr(), ws, ws_bytes,
                                   None)

    nan, inf = float("nan"), float("inf")
    bad = [dict(verts=None), dict(faces=None), dict(k=None), dict(m=None), dict(depth=None), dict(h=0), dict(w=0), dict(h=-1), dict(h=16385), dict(w=16385),
           dict(n_attr=-1), dict(n_attr=9), dict(attr=None), dict(out=None), dict(near=0.0), dict(near=-0.5), dict(near=nan), dict(near=inf), dict(cull=2), dict(cull=-1),
           dict(nf=-1), dict(nf=2 ** 31 - 1), dict(nv=-1), dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0)]
    for kw in bad:
        assert call(**kw) == INVALID_ARG, kw
        assert lib.nrf_last_error().startswith(b"nrf_raster_mesh"), kw
    torch.cuda.synchronize()
    assert (depth == 7).all() and (bary == 7).all() and (out == 7).all() and (face == 7).all() and (stats == 7).all() and (ws == 7).all(), "nothing was launched"
    assert call() == 0, "the same arguments unedited are fine, right after a refusal"
    torch.cuda.synchronize()
    want = sliced(reference("sphere", 0), 3)
    got = dict(depth=depth.cpu().numpy(), face=face.cpu().numpy(), bary=bary.cpu().numpy(), attr=out.cpu().numpy(), stats=(stats.cpu().numpy() - 7).view(np.uint32))
    assert_equal(got, want, "after the refusals")


# ------------------------------------------------------------------------------------ 6. the Python layer
def sphere_mesh(api, radius=None, centre=None):
    s = T.SPHERE
    verts, faces = R.octa_sphere(s["centre"] if centre is None else centre, s["radius"] if radius is None else radius)
    c = np.asarray(s["centre"] if centre is None else centre, F32)
    normals = (verts - c) / np.linalg.norm(verts - c, axis=1, keepdims=True).astype(F32)
    colors = np.random.default_rng(4).uniform(0.0, 1.0, verts.shape).astype(F32)
    m = api[2].Mesh(torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda(), torch.from_numpy(normals.astype(F32)).cuda(), torch.from_numpy(colors).cuda())
    return m, verts, faces, normals.astype(F32), colors


def test_render_mesh_and_render_mesh_view_equal_the_restatement(api):
    L, raster, mesh, scene = api
    from nerfpp_amd.dataset import View
    s = T.SPHERE
    m, verts, faces, normals, colors = sphere_mesh(api)
    pose = scene.pose_spherical(67.0, -35.0, 4.0)
    for cull in ("none", "back"):
        want = R.rasterize(verts, faces, np.concatenate([colors, normals], 1), s["h"], s["w"], K_SPHERE, pose, cull=int(cull == "back"))
        got = raster.RenderMesh(m, pose, s["w"], s["h"], K_SPHERE, cull=cull)
        assert isinstance(got, raster.MeshRender) and got.RelevancyMap is None and got.FaceMap.dtype == torch.int32
        assert np.array_equal(bits(got.DepthMap), bits(want["depth"])) and np.array_equal(got.FaceMap.cpu().numpy(), want["face"])
        assert np.array_equal(bits(got.BaryMap), bits(want["bary"])) and np.array_equal(bits(got.RGBMap), bits(want["attr"][..., :3]))
        assert np.array_equal(got.AccMap.cpu().numpy(), (want["face"] >= 0).astype(F32))
        assert np.array_equal(got.Stats.cpu().numpy().view(np.uint32), want["stats"])
        n = want["attr"][..., 3:]
        n = n / np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), 1e-8)
        assert np.abs(got.NormalMap.cpu().numpy() - n).max() <= 1e-6
    # a relevancy column rides along; attrs picks what is interpolated
    m.Relevancy = torch.from_numpy(attributes(len(verts))[:, :2].copy()).cuda()
    got = raster.RenderMesh(m, pose, s["w"], s["h"], K_SPHERE, attrs=("Relevancy",))
    want = R.rasterize(verts, faces, attributes(len(verts))[:, :2], s["h"], s["w"], K_SPHERE, pose)
    assert got.RGBMap is None and got.NormalMap is None and np.array_equal(bits(got.RelevancyMap), bits(want["attr"]))
    with pytest.raises(L.NrfError, match="cull"):
        raster.RenderMesh(m, pose, s["w"], s["h"], K_SPHERE, cull="front")
    # RenderMeshView: the dims and K of RenderViewDims
    from nerfpp_amd import renderer as RR
    view = View(s["h"], s["w"], K_SPHERE, pose)
    for factor in (0, 2):
        rp = scene.lego_render_params(s["bbox"], RenderFactor=factor)
        h1, w1, k1 = RR.RenderViewDims(s["h"], s["w"], K_SPHERE, factor)
        assert (h1, w1) == ((24, 28) if factor else (48, 56))
        got = raster.RenderMeshView(m, view, rp, attrs=())
        assert got.DepthMap.shape == (h1, w1) and got.RGBMap is None
        want = R.rasterize(verts, faces, None, h1, w1, k1, pose)
        assert np.array_equal(bits(got.DepthMap), bits(want["depth"])) and np.array_equal(got.FaceMap.cpu().numpy(), want["face"])
    assert torch.equal(raster.RenderMeshView(m, view, attrs=()).DepthMap, raster.RenderMeshView(m, view, scene.lego_render_params(s["bbox"]), attrs=()).DepthMap)


def test_visible_faces_and_filter_visible_drop_a_nested_sphere(api):
    L, raster, mesh, scene = api
    from nerfpp_amd.dataset import View
    s = T.SPHERE
    outer, verts, faces, normals, colors = sphere_mesh(api)
    views = [View(s["h"], s["w"], v["K"], v["c2w"]) for v in T.sphere_views(scene.pose_spherical, scene.lego_K)]

    def ref_visible(verts, faces):
        seen = np.zeros(len(faces), bool)
        for v in views:
            fm = R.rasterize(verts, faces, None, v.H, v.W, v.K, v.Pose)["face"]
            seen[fm[fm >= 0]] = True
        return seen
    want = ref_visible(verts, faces)
    got = raster.VisibleFaces(outer, views)
    assert got.dtype == torch.bool and got.shape == (512,) and np.array_equal(got.cpu().numpy(), want) and 100 < want.sum() <= 512
    # a smaller sphere inside: no camera sees it
    iv, ifc = R.octa_sphere(s["centre"], 0.4)
    v2, f2 = np.concatenate([iv, verts]), np.concatenate([ifc, faces + len(iv)])          # the inner sphere first: its faces have the lower indices
    both = mesh.Mesh(torch.from_numpy(v2).cuda(), torch.from_numpy(f2).cuda(), torch.from_numpy(np.concatenate([normals[:len(iv)] * 0 + 1, normals])).cuda(),
                     torch.from_numpy(np.concatenate([colors[:len(iv)], colors])).cuda())
    want2 = ref_visible(v2, f2)
    assert not want2[:512].any() and np.array_equal(want2[512:], want)
    kept = raster.FilterVisible(both, views)
    sub_v, sub_f, _, old = T.submesh(v2, f2, v2, want2)
    assert np.array_equal(bits(kept.Vertices), bits(sub_v)) and np.array_equal(kept.Faces.cpu().numpy(), sub_f)
    assert (old >= len(iv)).all() and np.array_equal(bits(kept.Colors), bits(np.concatenate([colors[:len(iv)], colors])[old]))


def test_evaluate_mesh_equals_its_parts_composed_by_hand(api):
    """The 24^3 scene of test_tsdf_gpu's FuseViews test: every number of EvaluateMesh(ExtractMeshTSDF(...)) is the same quantity formed here from RenderMesh,
    RenderView and metrics.  IoU > 0 and a finite depth error are a sanity check, not a quality bar."""
    L, raster, mesh, scene = api
    from nerfpp_amd import metrics, renderer as RR, tsdf
    sc = scene.make_hash_scene(mode="ngp", log2_t=14)
    r = sc["renderer"]
    views = tsdf.OrbitViews(4, 24, 24, scene.lego_K(24, 24), 4.0)
    rp = scene.lego_render_params(sc["bbox"], n_samples=16, n_importance=16)
    m = tsdf.ExtractMeshTSDF(r, views, rp, resolution=24, min_component_faces=0)
    assert m.Faces.shape[0] > 0 and m.Colors is not None
    got = raster.EvaluateMesh(m, r, views, rp)
    assert set(got) == {k for n in ("psnr", "ssim", "depth_error", "iou") for k in (n, "mean_" + n)}
    assert all(v.dtype == torch.float64 and v.is_cuda for v in got.values()) and all(got[n].shape == (4,) for n in ("psnr", "ssim", "depth_error", "iou"))
    white = torch.ones((3,), device="cuda")
    for i, v in enumerate(views):
        o = RR.RenderView(r, v.Pose, v.W, v.H, v.K, rp).Outputs
        mr = raster.RenderMesh(m, v.Pose, v.W, v.H, v.K, attrs=("Colors",))
        rgb = mr.RGBMap + (1.0 - mr.AccMap)[..., None] * white          # lego_render_params renders over white
        rgb_r, acc_r, depth_r = o.RGBMap.reshape(24, 24, 3), o.AccMap.reshape(24, 24), o.DepthMap.reshape(24, 24)
        a, b = mr.AccMap > 0, acc_r >= 0.5
        both = a & b
        err = (mr.DepthMap - depth_r / acc_r).abs().to(torch.float64)[both]
        assert torch.equal(got["psnr"][i], metrics.PSNR(rgb, rgb_r)) and torch.equal(got["ssim"][i], metrics.SSIM(rgb, rgb_r))
        assert float(got["iou"][i]) == float(both.sum()) / float((a | b).sum())
        assert abs(float(got["depth_error"][i]) - float(err.sum() / both.sum())) <= 1e-12
    for n in ("psnr", "ssim", "depth_error", "iou"):
        assert torch.equal(got["mean_" + n], got[n].mean())
    print({k: v.tolist() for k, v in got.items()})
    assert float(got["mean_iou"]) > 0 and np.isfinite(float(got["mean_depth_error"]))
    black = raster.EvaluateMesh(m, r, views[:1], rp, background=(0.0, 0.0, 0.0))
    assert set(black) == set(got) and float(black["iou"][0]) == float(got["iou"][0])
    with pytest.raises(L.NrfError, match="NDC"):
        raster.EvaluateMesh(m, r, views, scene.lego_render_params(sc["bbox"], n_samples=16, n_importance=16, Ndc=True))
    with pytest.raises(L.NrfError, match="LeRF"):
        raster.EvaluateMesh(m, scene.make_lerf_scene(log2_t=14)["renderer"], views, rp)
