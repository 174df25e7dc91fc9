"""Depth fusion on the MI355X: nrf_tsdf_integrate, nrf_tsdf_observed and nrf_tsdf_sample_color against the numpy restatement (tests/tsdf_ref.py) bit for bit, the
batching and run-to-run guarantees, the refusals, and the Python layers built on them: TSDFVolume, Extract, FuseViews and ExtractMeshTSDF."""
import ctypes as C

import numpy as np
import pytest
import torch

import components_ref as CR
import mesh_ref as M
import tsdf_ref as R

pytestmark = pytest.mark.gpu

INVALID_ARG = 1
F32 = np.float32
BOX = np.array([-1.0, -0.8, -0.5, 1.2, 0.7, 0.6], F32)          # not cubic, not centred
H, W = 7, 11
K = np.array([[9.5, 0, 5.3], [0, 7.25, 3.6], [0, 0, 1]], F32)          # fx != fy, principal point off-centre
TRUNC, ACC_MIN, MAX_WEIGHT = 0.3, 0.5, 2.0


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from nerfpp_amd import _lib as L, mesh, scene, tsdf
    return L, tsdf, mesh, scene


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, F32).view(np.uint32)


def make_views(pose_spherical, n, seed=1):
    """View 1 sits inside the box (voxels lie behind it), view 3 looks away from it; the others orbit at 2.5.  Depth is a plane plus noise with NaN, +inf, 0 and
    negative pixels written in; acc is drawn from {0, 0.3, 0.5, 0.9, 1, NaN} (0.5 == acc_min takes the solid branch)."""
    views = []
    for i in range(n):
        rng = np.random.default_rng(seed * 1000 + i)
        c2w = pose_spherical(40.0 * i + 10.0, -20.0 if i % 2 else 30.0, 0.3 if i == 1 else 2.5)
        if i == 3:
            c2w = c2w.copy()
            c2w[:, 0] *= -1          # half a turn about the camera's y axis: the box is behind it
            c2w[:, 2] *= -1
        y, x = np.mgrid[0:H, 0:W].astype(F32)
        depth = (F32(2.0) + F32(0.6) * x / F32(W) + rng.uniform(-0.3, 0.3, (H, W)).astype(F32)).astype(F32)
        flat = depth.reshape(-1)
        flat[rng.choice(H * W, 8, replace=False)] = np.array([np.nan, np.nan, np.inf, np.inf, 0.0, 0.0, -1.5, -0.25], F32)
        acc = rng.choice(np.array([0.0, 0.3, 0.5, 0.9, 1.0, 1.0, 1.0, np.nan], F32), (H, W)).astype(F32)
        rgb = rng.uniform(0.05, 1.0, (H, W, 3)).astype(F32)
        views.append(dict(depth=depth, acc=acc, rgb=rgb, K=K, c2w=c2w))
    return views


class Device:
    """A volume and a list of views on the device, driven through the C entry itself (so NULL images and every parameter are the test's to choose)."""

    def __init__(self, api, nx, ny, nz, colors=True):
        self.L, self.T = api[0], api[1]
        self.n = (nx, ny, nz)
        self.tsdf = torch.ones((nz, ny, nx), device="cuda")
        self.weight = torch.zeros((nz, ny, nx), device="cuda")
        self.color = torch.zeros((4, nz, ny, nx), device="cuda") if colors else None
        self.keep = []

    def records(self, views):
        recs = []
        for v in views:
            r = self.T.TsdfView()
            t = {k: (None if v.get(k) is None else torch.from_numpy(np.ascontiguousarray(v[k], F32)).cuda()) for k in ("depth", "acc", "rgb")}
            self.keep.append(t)
            r.d_depth, r.d_acc, r.d_rgb = (None if t[k] is None else t[k].data_ptr() for k in ("depth", "acc", "rgb"))
            r.h, r.w = v["depth"].shape
            r.K = (C.c_float * 9)(*np.asarray(v["K"], F32).reshape(9).tolist())
            r.c2w = (C.c_float * 12)(*np.asarray(v["c2w"], F32)[:3, :4].reshape(12).tolist())
            recs.append(r)
        return recs

    def integrate(self, views, bbox=BOX, trunc=TRUNC, acc_min=ACC_MIN, max_weight=MAX_WEIGHT, carve=1, recs=None):
        recs = self.records(views) if recs is None else recs
        arr = (self.T.TsdfView * max(len(recs), 1))(*recs)
        bb = np.ascontiguousarray(bbox, F32)
        return self.L.lib().nrf_tsdf_integrate(self.tsdf.data_ptr(), self.weight.data_ptr(), None if self.color is None else self.color.data_ptr(), *self.n,
                                               bb.ctypes.data_as(C.c_void_p), C.cast(arr, C.c_void_p), len(recs), trunc, acc_min, max_weight, carve, None)

    def assert_equals(self, tsdf, weight, color):
        torch.cuda.synchronize()
        assert np.array_equal(bits(self.tsdf), bits(tsdf)), "tsdf"
        assert np.array_equal(bits(self.weight), bits(weight)), "weight"
        if color is not None:
            for p, name in enumerate("rgbw"):
                assert np.array_equal(bits(self.color[p]), bits(color[p])), f"colour plane {name}"


def strip(views, *keys):
    return [{k: (None if k in keys else x) for k, x in v.items()} for v in views]


# ------------------------------------------------------------------------------------ 1. integrate
@pytest.mark.parametrize("n_views", [1, 3, 17, 33])
@pytest.mark.parametrize("lattice", [(13, 9, 6), (16, 5, 4)])
def test_integrate_equals_the_restatement_bit_for_bit(api, lattice, n_views):
    """nx once no multiple of 4 (vector body + scalar tail) and once one; 17 and 33 views cross the 16-view launch limit once and twice; max_weight = 2."""
    views = make_views(api[3].pose_spherical, n_views)
    tsdf, weight, color = R.new_volume(*lattice)
    counts = {}
    R.integrate(tsdf, weight, color, BOX, views, TRUNC, ACC_MIN, MAX_WEIGHT, True, counts)
    print(lattice, n_views, counts)
    empty = [k for k in (R.CLASSES if n_views >= 3 else ("updated", "carved", "outside")) if counts[k] == 0]
    assert not empty, f"the case exercises no voxel-view pair of {empty}"
    dev = Device(api, *lattice)
    assert dev.integrate(views) == 0
    dev.assert_equals(tsdf, weight, color)


def test_integrate_rows_longer_than_a_wave(api):
    """nx = 261: two 256-wide chunks per row, the second a single scalar-tail voxel; rows of odd length start at addresses that are only 4-byte aligned."""
    lattice = (261, 3, 2)
    views = make_views(api[3].pose_spherical, 3)
    tsdf, weight, color = R.new_volume(*lattice)
    counts = {}
    R.integrate(tsdf, weight, color, BOX, views, TRUNC, ACC_MIN, MAX_WEIGHT, True, counts)
    assert counts["updated"] > 0 and weight[:, :, 256:].max() > 0, "the last chunk is touched"
    dev = Device(api, *lattice)
    assert dev.integrate(views) == 0
    dev.assert_equals(tsdf, weight, color)


@pytest.mark.parametrize("variant", ["no_acc", "no_rgb", "no_color", "no_carve"])
@pytest.mark.parametrize("lattice", [(13, 9, 6), (16, 5, 4)])
def test_integrate_variants_equal_the_restatement(api, lattice, variant):
    views = make_views(api[3].pose_spherical, 3)
    views = strip(views, "acc") if variant == "no_acc" else strip(views, "rgb") if variant == "no_rgb" else views
    carve = variant != "no_carve"
    tsdf, weight, color = R.new_volume(*lattice, colors=variant != "no_color")
    counts = {}
    R.integrate(tsdf, weight, color, BOX, views, TRUNC, ACC_MIN, MAX_WEIGHT, carve, counts)
    assert counts["updated"] > 0 and (counts["carved"] > 0) == (variant not in ("no_acc", "no_carve"))
    dev = Device(api, *lattice, colors=variant != "no_color")
    assert dev.integrate(views, carve=int(carve)) == 0
    dev.assert_equals(tsdf, weight, color)
    if variant == "no_rgb":
        assert float(dev.color.abs().max()) == 0.0, "no image, no colour"
    if variant == "no_acc":
        # one view with an acc image among views without: per view, not per call
        mixed = strip(make_views(api[3].pose_spherical, 3), "acc")
        mixed[2] = make_views(api[3].pose_spherical, 3)[2]
        tsdf, weight, color = R.new_volume(*lattice)
        R.integrate(tsdf, weight, color, BOX, mixed, TRUNC, ACC_MIN, MAX_WEIGHT, True)
        dev = Device(api, *lattice)
        assert dev.integrate(mixed) == 0
        dev.assert_equals(tsdf, weight, color)


def test_boundary_sdf_equal_to_minus_trunc_is_updated(api):
    """Box +-1 with 9^3 points, identity rotation, camera at (0, 0, 3), constant depth 2.5, trunc 0.5: exact in fp32.  The plane z = 0 has sdf == -trunc, is updated and
    gets s = -1; the plane z = -0.25 is skipped."""
    box = np.array([-1, -1, -1, 1, 1, 1], F32)
    view = dict(depth=np.full((8, 8), 2.5, F32), rgb=np.full((8, 8, 3), 0.25, F32), K=np.array([[8, 0, 4], [0, 8, 4], [0, 0, 1]], F32),
                c2w=np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 3]], F32))
    tsdf, weight, color = R.new_volume(9, 9, 9)
    R.integrate(tsdf, weight, color, box, [view], 0.5, 0.5, 64.0, True)
    dev = Device(api, 9, 9, 9)
    assert dev.integrate([view], bbox=box, trunc=0.5, max_weight=64.0) == 0
    dev.assert_equals(tsdf, weight, color)
    t, w = dev.tsdf.cpu().numpy(), dev.weight.cpu().numpy()
    assert (w[4] == 1).all() and (t[4] == -1).all(), "z = 0: every voxel of the plane projects into the image, sdf == -trunc"
    assert (w[3] == 0).all() and (t[3] == 1).all() and (w[:3] == 0).all(), "z = -0.25 and below: sdf < -trunc"
    assert (t[5][w[5] > 0] == -0.5).all() and (w[5] > 0).any()


def test_one_call_over_17_views_equals_17_calls_and_two_runs_agree(api):
    views = make_views(api[3].pose_spherical, 17, seed=2)
    one = Device(api, 13, 9, 6)
    recs = one.records(views)
    assert one.integrate(None, recs=recs) == 0
    again = Device(api, 13, 9, 6)
    assert again.integrate(None, recs=recs) == 0
    each = Device(api, 13, 9, 6)
    for r in recs:
        assert each.integrate(None, recs=[r]) == 0
    torch.cuda.synchronize()
    for name in ("tsdf", "weight", "color"):
        a, b, c = (bits(getattr(d, name)) for d in (one, again, each))
        assert np.array_equal(a, b), f"two runs, {name}"
        assert np.array_equal(a, c), f"17 calls, {name}"
    assert float(one.weight.max()) == MAX_WEIGHT


# ------------------------------------------------------------------------------------ 2. observed, sample_color
def test_observed_and_sample_color_equal_the_restatement(api):
    L, T = api[0], api[1]
    nx, ny, nz = 13, 9, 6
    views = make_views(api[3].pose_spherical, 3)[:1]          # one orbit view: part of the lattice stays unobserved
    tsdf, weight, color = R.new_volume(nx, ny, nz)
    R.integrate(tsdf, weight, color, BOX, views, TRUNC, ACC_MIN, MAX_WEIGHT, False)
    assert 0.05 < (weight > 0).mean() < 0.95 and 0 < (color[3] > 0).sum() < (weight > 0).sum()
    lat = M.lattice_points(BOX, nx, ny, nz).reshape(-1, 3)
    step = (BOX[3:] - BOX[:3]) / (np.array([nx, ny, nz]) - 1).astype(F32)
    rng = np.random.default_rng(5)
    unseen = lat[weight.reshape(-1) == 0]
    corners = np.array([[BOX[0 + 3 * (c & 1)], BOX[1 + 3 * (c >> 1 & 1)], BOX[2 + 3 * (c >> 2)]] for c in range(8)], F32)
    special = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [5, 5, 5], [-5, 0.1, 0.2], [1e30, 0, 0], [0, -3e38, 0], [3e38, 3e38, 3e38]], F32)
    pts = np.concatenate([lat, corners, special, unseen + F32(0.9) * step * np.array([1, 0, 0], F32), unseen - F32(0.6) * step,
                          lat + (F32(0.5) * step).astype(F32), rng.uniform(BOX[:3] - 0.3, BOX[3:] + 0.3, (500, 3)).astype(F32)]).astype(F32)
    want_ok = R.observed(weight, BOX, pts)
    want_rgb = R.sample_color(color, BOX, pts)
    assert 0 < want_ok.sum() < len(pts) and not want_ok[len(lat) + 8:len(lat) + 11].any()
    assert (want_rgb == 0).all(-1).any() and (want_rgb > 0).all(-1).any(), "den == 0 gives 0"
    vol = T.TSDFVolume(BOX, (nx, ny, nz), trunc=4.0 * float(step.max()))
    vol.weight.copy_(torch.from_numpy(weight)); vol.color.copy_(torch.from_numpy(color))
    d_pts = torch.from_numpy(pts).cuda()
    ok, rgb = vol.Observed(d_pts), vol.SampleColor(d_pts)
    assert ok.dtype == torch.bool and np.array_equal(ok.cpu().numpy(), want_ok)
    assert np.array_equal(bits(rgb), bits(want_rgb))
    assert torch.equal(vol.Observed(d_pts), ok) and torch.equal(vol.SampleColor(d_pts), rgb)
    assert vol.Observed(d_pts[:0]).shape == (0,) and vol.SampleColor(d_pts[:0]).shape == (0, 3)
    with pytest.raises(L.NrfError):
        T.TSDFVolume(BOX, (nx, ny, nz), trunc=4.0 * float(step.max()), colors=False).SampleColor(d_pts)


# ------------------------------------------------------------------------------------ 3. the sphere of the host test
def test_sphere_volume_and_extract_equal_the_host_pipeline(api, tmp_path):
    L, T, mesh, scene = api
    s = R.SPHERE
    views = R.sphere_views(scene.pose_spherical, scene.lego_K)
    tsdf, weight, color = R.fuse_sphere(views)
    vol = T.TSDFVolume(s["bbox"], s["n"], trunc=float(F32(s["trunc_steps"]) * F32(R.sphere_step())), max_weight=s["max_weight"], acc_min=s["acc_min"])
    dev = [{k: (torch.from_numpy(x).cuda() if k in ("depth", "acc", "rgb") else x) for k, x in v.items()} for v in views]
    vol.IntegrateViews([(v["depth"], v["K"], v["c2w"], v["acc"], v["rgb"]) for v in dev[:2]])
    vol.Integrate(dev[2]["depth"], dev[2]["K"], dev[2]["c2w"], acc=dev[2]["acc"], rgb=dev[2]["rgb"])
    vol.IntegrateViews([dict(depth=v["depth"], K=v["K"], pose=v["c2w"], acc=v["acc"], rgb=v["rgb"]) for v in dev[3:]])
    for name, want in (("tsdf", tsdf), ("weight", weight), ("color", color)):
        assert np.array_equal(bits(getattr(vol, name)), bits(want)), name
    assert torch.equal(vol.Field(), -vol.tsdf)
    got = vol.Extract()
    v, f, n = R.extract(tsdf, weight, s["bbox"])
    assert isinstance(got, mesh.Mesh) and got.Faces.dtype == torch.int32
    assert np.array_equal(bits(got.Vertices), bits(v)) and np.array_equal(got.Faces.cpu().numpy(), f)
    assert np.abs(got.Normals.cpu().numpy() - n).max() <= 1e-6
    assert np.array_equal(bits(got.Colors), bits(R.sample_color(color, s["bbox"], v)))
    assert float(got.Colors.min()) >= 0.0 and float(got.Colors.max()) <= 1.0 and float(got.Colors.max()) > 0.5
    assert M.edge_check(f) == (True, True) and R.radial_error(v).max() <= 1.5
    # the rest of the mesh tool chain takes it
    labels, k = mesh.MeshComponents(got)
    assert k == 1 == CR.mesh_components(f, len(v))[1]
    kept = vol.Extract(keep_largest=1, min_component_faces=10)
    assert torch.equal(kept.Faces, got.Faces) and torch.equal(kept.Colors, got.Colors)
    assert mesh.FilterComponents(got, min_faces=len(f) + 1).Faces.shape[0] == 0
    mesh.SavePLY(str(tmp_path / "sphere.ply"), got)
    pv, pf = M.read_ply(str(tmp_path / "sphere.ply"))
    assert len(pv) == len(v) and np.array_equal(pf["idx"], f) and "red" in pv.dtype.names
    vol.Reset()
    assert float(vol.tsdf.min()) == 1.0 and float(vol.weight.max()) == 0.0 and float(vol.color.max()) == 0.0
    assert vol.Extract().Faces.shape[0] == 0, "an empty volume has no surface"


# ------------------------------------------------------------------------------------ 4. end to end on a network
def test_fuse_views_on_a_network_equals_the_restatement_of_its_renders(api):
    L, T, mesh, scene = api
    from nerfpp_amd import renderer as RR
    sc = scene.make_hash_scene(mode="ngp", log2_t=14)
    r = sc["renderer"]
    views = T.OrbitViews(4, 24, 24, scene.lego_K(24, 24), 4.0)
    for factor in (0, 2):
        rp = scene.lego_render_params(sc["bbox"], n_samples=16, n_importance=16, RenderFactor=factor)
        vol = T.FuseViews(r, views, rp, resolution=24)
        assert (vol.nx, vol.ny, vol.nz) == (24, 24, 24) and np.array_equal(vol.bbox, sc["bbox"])
        assert vol.trunc == float(F32(5) * (F32(3.0) / F32(23)))
        recs = []
        for v in views:
            h1, w1, k1 = RR.RenderViewDims(v.H, v.W, v.K, factor)
            assert (h1, w1) == ((12, 12) if factor else (24, 24))
            o = RR.RenderView(r, v.Pose, v.W, v.H, v.K, rp).Outputs
            recs.append(dict(depth=o.DepthMap.cpu().numpy().reshape(h1, w1), acc=o.AccMap.cpu().numpy().reshape(h1, w1),
                             rgb=o.RGBMap.cpu().numpy().reshape(h1, w1, 3), K=k1, c2w=v.Pose))
        tsdf, weight, color = R.new_volume(24, 24, 24)
        counts = {}
        R.integrate(tsdf, weight, color, sc["bbox"], recs, vol.trunc, 0.5, 64.0, True, counts)
        print(factor, counts)
        assert counts["updated"] + counts["carved"] > 0
        for name, want in (("tsdf", tsdf), ("weight", weight), ("color", color)):
            assert np.array_equal(bits(getattr(vol, name)), bits(want)), (factor, name)
        # a volume handed in is fused into, and its own parameters hold
        mine = T.TSDFVolume(sc["bbox"], 24, carve=False, colors=False)
        assert T.FuseViews(r, views[:2], rp, volume=mine) is mine
        t2, w2, _ = R.new_volume(24, 24, 24, colors=False)
        R.integrate(t2, w2, None, sc["bbox"], recs[:2], mine.trunc, 0.5, 64.0, False)
        assert np.array_equal(bits(mine.tsdf), bits(t2)) and np.array_equal(bits(mine.weight), bits(w2))
    rp = scene.lego_render_params(sc["bbox"], n_samples=16, n_importance=16)
    m = T.ExtractMeshTSDF(r, views, rp, resolution=24, min_component_faces=0)
    assert isinstance(m, mesh.Mesh) and m.Colors is not None and m.Colors.shape == m.Vertices.shape and m.Normals.shape == m.Vertices.shape
    if m.Vertices.shape[0]:
        assert float(m.Colors.min()) >= 0.0 and float(m.Colors.max()) <= 1.0 and int(m.Faces.max()) < m.Vertices.shape[0]
    with pytest.raises(L.NrfError, match="NDC"):
        T.FuseViews(r, views, scene.lego_render_params(sc["bbox"], n_samples=16, n_importance=16, Ndc=True), resolution=24)
    with pytest.raises(L.NrfError, match="LeRF"):
        T.FuseViews(scene.make_lerf_scene(log2_t=14)["renderer"], views, rp, resolution=24)


# ------------------------------------------------------------------------------------ 5. refusals
def test_c_entries_refuse_bad_arguments_and_touch_nothing(api):
    L = api[0]
    lib = L.lib()
    views = make_views(api[3].pose_spherical, 1)
    dev = Device(api, 13, 9, 6)
    rec = dev.records(views)[0]
    arr = (api[1].TsdfView * 1)(rec)
    bb = np.ascontiguousarray(BOX)
    t, w, c = dev.tsdf.data_ptr(), dev.weight.data_ptr(), dev.color.data_ptr()

    def call(tsdf=t, weight=w, n=(13, 9, 6), bbox=bb, views=arr, n_views=1, trunc=TRUNC, acc_min=ACC_MIN, max_weight=MAX_WEIGHT):
        return lib.nrf_tsdf_integrate(tsdf, weight, c, *n, None if bbox is None else bbox.ctypes.data_as(C.c_void_p), C.cast(views, C.c_void_p), n_views, trunc, acc_min,
                                      max_weight, 1, None)

    def edited(**kw):
        r = api[1].TsdfView.from_buffer_copy(rec)
        for k, v in kw.items():
            setattr(r, k, v)
        return (api[1].TsdfView * 2)(rec, r)

    inverted, flat = bb.copy(), bb.copy()
    inverted[4] = -2.0
    flat[5] = flat[2]
    nan, inf = float("nan"), float("inf")
    bad = [dict(tsdf=None), dict(weight=None), dict(bbox=None), dict(bbox=inverted), dict(bbox=flat), dict(n=(1, 9, 6)), dict(n=(13, 1, 6)), dict(n=(13, 9, 0)),
           dict(trunc=0.0), dict(trunc=-0.3), dict(trunc=nan), dict(trunc=inf), dict(acc_min=0.0), dict(acc_min=-1.0), dict(acc_min=nan), dict(acc_min=inf),
           dict(max_weight=0.5), dict(max_weight=nan), dict(n_views=-1), dict(views=None),
           dict(views=edited(d_depth=None), n_views=2), dict(views=edited(h=0), n_views=2), dict(views=edited(w=0), n_views=2), dict(views=edited(w=-3), n_views=2)]
    for kw in bad:
        assert call(**kw) == INVALID_ARG, kw
        assert lib.nrf_last_error().startswith(b"nrf_tsdf_integrate"), kw
    assert call(n_views=0) == 0 and call(n_views=0, views=None) == 0
    torch.cuda.synchronize()
    assert float(dev.tsdf.min()) == 1.0 and float(dev.weight.max()) == 0.0 and float(dev.color.abs().max()) == 0.0, "nothing was launched"
    assert call() == 0 and float(dev.weight.max()) == 1.0, "the same arguments unedited are fine"
    # the two queries
    pts = torch.zeros((4, 3), device="cuda")
    ok = torch.full((4,), 7, dtype=torch.uint8, device="cuda")
    rgb = torch.full((4, 3), 7.0, device="cuda")
    b = bb.ctypes.data_as(C.c_void_p)
    assert lib.nrf_tsdf_observed(w, 13, 9, 1, b, pts.data_ptr(), 4, ok.data_ptr(), None) == INVALID_ARG
    assert lib.nrf_tsdf_observed(w, 13, 9, 6, inverted.ctypes.data_as(C.c_void_p), pts.data_ptr(), 4, ok.data_ptr(), None) == INVALID_ARG
    assert lib.nrf_tsdf_observed(None, 13, 9, 6, b, pts.data_ptr(), 4, ok.data_ptr(), None) == INVALID_ARG
    assert lib.nrf_tsdf_observed(w, 13, 9, 6, b, pts.data_ptr(), -1, ok.data_ptr(), None) == INVALID_ARG
    assert lib.nrf_tsdf_sample_color(c, 1, 9, 6, b, pts.data_ptr(), 4, rgb.data_ptr(), None) == INVALID_ARG
    assert lib.nrf_tsdf_sample_color(None, 13, 9, 6, b, pts.data_ptr(), 4, rgb.data_ptr(), None) == INVALID_ARG
    assert lib.nrf_tsdf_sample_color(c, 13, 9, 6, b, pts.data_ptr(), 4, None, None) == INVALID_ARG
    assert lib.nrf_tsdf_observed(w, 13, 9, 6, b, None, 0, None, None) == 0 and lib.nrf_tsdf_sample_color(c, 13, 9, 6, b, None, 0, None, None) == 0
    torch.cuda.synchronize()
    assert (ok == 7).all() and (rgb == 7.0).all()
