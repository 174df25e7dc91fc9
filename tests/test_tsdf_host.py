"""Depth fusion without a GPU: the definition (tests/tsdf_ref.py, the numpy restatement the GPU tests compare nrf_tsdf_* with bit for bit) pinned on an analytic
sphere through the existing mesh_ref.isosurface, the carve rule, the refusals of TSDFVolume and the poses of OrbitViews."""
import ctypes as C
import os

import numpy as np
import pytest

import components_ref as CR
import mesh_ref as M
import tsdf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sphere():
    from nerfpp_amd import scene
    views = R.sphere_views(scene.pose_spherical, scene.lego_K)
    tsdf, weight, _ = R.fuse_sphere(views, carve=True, colors=False)
    return dict(views=views, tsdf=tsdf, weight=weight)


def test_entry_points_declared_and_exported():
    from nerfpp_amd import _lib
    names = ("nrf_tsdf_integrate", "nrf_tsdf_observed", "nrf_tsdf_sample_color")
    assert all(n in _lib.SYMBOLS for n in names)
    hdr = open(os.path.join(ROOT, "include", "nerfpp_hip.h")).read()
    assert "} nrf_tsdf_view;" in hdr
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, n) for n in names)
    from nerfpp_amd.tsdf import TsdfView
    assert C.sizeof(TsdfView) == 120 and TsdfView.K.offset == 32 and TsdfView.c2w.offset == 68          # three pointers, h, w, K[9], c2w[12], padded to 8


def test_the_filtered_zero_level_of_a_fused_sphere_is_the_sphere(sphere):
    """6 views of 48 x 56, 33^3 lattice points, trunc = 4 steps: the filtered mesh is closed, one piece, and on the sphere (mean <= 0.25 step, max <= 1.5 steps; the
    model gives 0.16 and 1.08).  Unfiltered, the zero level also holds the sheet between the observed band behind the surface and the never-observed interior, more
    than 3 steps off: the observed filter is what this test is about."""
    s = R.SPHERE
    assert sphere["weight"].max() <= s["n_views"] and (sphere["weight"] == 0).any() and (sphere["tsdf"] < 0).any()
    v, f, n = R.extract(sphere["tsdf"], sphere["weight"], s["bbox"])
    assert len(f) > 1000
    assert M.edge_check(f) == (True, True), "closed, consistently wound"
    assert CR.mesh_components(f, len(v))[1] == 1
    assert M.euler(v, f) == 2
    assert M.signed_volume(v, f) > 0, "outward"
    err = R.radial_error(v)
    print(f"filtered: {len(f)} faces, mean {err.mean():.3f} max {err.max():.3f} steps")
    assert err.mean() <= 0.25 and err.max() <= 1.5
    va, fa, _ = R.extract(sphere["tsdf"], sphere["weight"], s["bbox"], filtered=False)
    assert len(fa) > len(f) and R.radial_error(va).max() > 3.0


def test_without_carving_the_surface_stays_open(sphere):
    """carve off: the voxels only background rays cross are never observed, the band around the silhouettes ends in mid air and the filtered mesh has open edges."""
    s = R.SPHERE
    tsdf, weight, _ = R.fuse_sphere(sphere["views"], carve=False, colors=False)
    assert (weight > 0).sum() < (sphere["weight"] > 0).sum()
    _, f, _ = R.extract(tsdf, weight, s["bbox"])
    assert len(f) > 0 and M.edge_check(f)[0] is False


def test_restatement_on_a_hand_checked_voxel():
    """One camera at (0, 0, 3) looking down -z, constant depth 2.5, trunc 0.5 on the 9^3 lattice of the box +-1: every quantity is exact in fp32."""
    tsdf, weight, color = R.new_volume(9, 9, 9)
    K = np.array([[8, 0, 4], [0, 8, 4], [0, 0, 1]], np.float32)
    c2w = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 3]], np.float32)
    view = dict(depth=np.full((8, 8), 2.5, np.float32), rgb=np.full((8, 8, 3), 0.25, np.float32), K=K, c2w=c2w)
    counts = {}
    R.integrate(tsdf, weight, color, [-1, -1, -1, 1, 1, 1], [view], 0.5, 0.5, 64.0, True, counts)
    # the voxel (0, 0, z) projects to u = v = 4 exactly: zd = 3 - z, sdf = z - 0.5
    col = lambda a: a[:, 4, 4]
    assert col(tsdf).tolist() == [1, 1, 1, 1, -1, -0.5, 0, 0.5, 1], "z = -0.25 and below are skipped (sdf < -trunc), z = 0 has sdf == -trunc and is updated"
    assert col(weight).tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 1]
    assert col(color[3]).tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 1] and col(color[0]).tolist() == [0, 0, 0, 0, 0.25, 0.25, 0.25, 0.25, 0.25]
    assert counts["below_trunc"] > 0 and counts["outside"] > 0 and counts["behind"] == 0
    pts = np.array([[0, 0, 0.5], [0, 0, 0.0], [0, 0, 0.26], [np.nan, 0, 0.5], [0, 0, 9.0]], np.float32)
    assert R.observed(weight, [-1, -1, -1, 1, 1, 1], pts).tolist() == [True, False, True, False, True]
    assert R.sample_color(color, [-1, -1, -1, 1, 1, 1], pts[:2]).tolist() == [[0.25] * 3] * 2, "corners without a colour take no part"
    assert R.sample_color(color, [-1, -1, -1, 1, 1, 1], np.array([[0, 0, -0.6]], np.float32)).tolist() == [[0.0] * 3], "den == 0 gives 0"


def test_volume_refuses_a_thin_band_and_bad_shapes():
    from nerfpp_amd import _lib as L
    from nerfpp_amd.tsdf import TSDFVolume
    box = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
    step = np.float32(3.0) / np.float32(32)
    with pytest.raises(L.NrfError, match="trunc"):
        TSDFVolume(box, 33, trunc=float(np.float32(3.99) * step))
    with pytest.raises(L.NrfError, match="trunc"):
        TSDFVolume(box, (65, 33, 65), trunc=float(np.float32(4) * step) * 0.5)          # the LARGEST axis step counts
    with pytest.raises(L.NrfError, match="trunc"):
        TSDFVolume(box, 33, trunc=float("nan"))
    for bad in (1, (33, 33), (33, 1, 33)):
        with pytest.raises(L.NrfError, match="resolution"):
            TSDFVolume(box, bad)
    with pytest.raises(L.NrfError, match="bbox"):
        TSDFVolume(box[:5], 33)
    with pytest.raises(L.NrfError, match="box"):
        TSDFVolume([-1, -1, -1, 1, -1, 1], 33)
    with pytest.raises(L.NrfError, match="max_weight"):
        TSDFVolume(box, 33, max_weight=0.5)
    with pytest.raises(L.NrfError, match="acc_min"):
        TSDFVolume(box, 33, acc_min=0.0)
    # what passes, on the host: 4 steps exactly, and the default of 5
    v = TSDFVolume(box, 33, trunc=float(np.float32(4) * step), colors=False, device="cpu")
    assert v.tsdf.shape == (33, 33, 33) and float(v.tsdf.min()) == 1.0 and float(v.weight.max()) == 0.0 and v.color is None
    v = TSDFVolume(box, (9, 33, 17), device="cpu")
    assert v.trunc == float(np.float32(5) * (np.float32(3.0) / np.float32(8))) and v.color.shape == (4, 17, 33, 9)
    v.tsdf.fill_(0.5); v.weight.fill_(2.0); v.color.fill_(1.0)
    v.Reset()
    assert float(v.tsdf.min()) == 1.0 and float(v.weight.max()) == 0.0 and float(v.color.max()) == 0.0
    assert bool((v.Field() == -1.0).all())


def test_orbit_views_are_pose_spherical():
    from nerfpp_amd import scene
    from nerfpp_amd.tsdf import OrbitViews
    K = scene.lego_K(20, 30)
    views = OrbitViews(5, 20, 30, K, 4.0)
    assert len(views) == 5
    for i, v in enumerate(views):
        assert (v.H, v.W) == (20, 30) and np.array_equal(v.K, K) and v.K.dtype == np.float32
        assert np.array_equal(v.Pose, scene.pose_spherical(360.0 * i / 5, -30.0 if i % 2 == 0 else 30.0, 4.0))
    high = OrbitViews(3, 8, 8, K, 2.5, elevations=(10.0,))
    assert all(np.array_equal(v.Pose, scene.pose_spherical(120.0 * i, 10.0, 2.5)) for i, v in enumerate(high))
