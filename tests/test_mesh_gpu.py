"""Mesh export on the MI355X: the density lattice against RunNetwork(F32) and the C oracle, the isosurface against the numpy restatement (tests/mesh_ref.py)
bit for bit, determinism, non-finite lattices, and ExtractMesh's colours."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mesh_ref as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from nerfpp_amd import _lib as L, mesh, scene
    return L, mesh, scene


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.uint32)


_SCENES = {}


def _scene(scene, kind):
    if kind not in _SCENES:
        _SCENES[kind] = scene.make_classic_scene() if kind == "classic" else scene.make_hash_scene(mode=kind)
    return _SCENES[kind]


def _run_network_sigma(sc, pts):
    p = torch.from_numpy(pts.reshape(-1, 1, 3)).cuda()
    vd = torch.zeros((p.shape[0], 3), device="cuda", dtype=torch.float32)
    return sc["renderer"].RunNetwork(p, vd)[:, 0, 3]


@pytest.mark.parametrize("kind", ["cu", "ngp", "classic"])
def test_density_grid_equals_run_network_f32(api, kind):
    L, mesh, scene = api
    sc = _scene(scene, kind)
    box = sc["bbox"] * np.float32(1.15)                # pokes outside the hash box: masked zeros there
    nx, ny, nz = 33, 17, 9
    ref = _run_network_sigma(sc, M.lattice_points(box, nx, ny, nz))
    for slab in (None, 1, 997):
        g = mesh.DensityGrid(sc["renderer"], box, (nx, ny, nz), slab_points=slab)
        assert g.shape == (nz, ny, nx)
        assert (_bits(g).reshape(-1) == _bits(ref)).all(), (kind, slab)
    if kind != "classic":
        outside = (np.abs(M.lattice_points(box, nx, ny, nz)) > sc["bbox"][3]).any(-1).reshape(-1)
        assert outside.any() and (g.reshape(-1).cpu().numpy()[outside] == 0).all()
        assert (g.cpu().numpy() != 0).any()


def test_density_grid_equals_oracle(api):
    L, mesh, scene = api
    from oracle import capi as O
    sc = _scene(scene, "ngp")
    cfg = sc["cfg"]
    box = sc["bbox"] * np.float32(1.1)
    g = mesh.DensityGrid(sc["renderer"], box, 9).cpu().numpy().reshape(-1)
    pts = M.lattice_points(box, 9, 9, 9).reshape(-1, 3)
    feats, keep = O.hash_ngp(pts, sc["table"], sc["bbox"], cfg["n_levels"], cfg["n_feat"], cfg["log2_t"], cfg["base"], cfg["finest"])
    x = np.concatenate([feats, O.sh_libtorch(np.zeros_like(pts), cfg["sh_degree"])], 1)
    raw = O.mlp_small(sc["mlp_blob"], x, 32, 16)
    raw[~keep, 3] = 0.0
    assert (g.view(np.uint32) == raw[:, 3].view(np.uint32)).all()


def _gpu_isosurface(mesh, f, box, iso):
    v, fc, n = mesh.Isosurface(torch.from_numpy(np.ascontiguousarray(f, np.float32)).cuda(), box, iso)
    return v.cpu().numpy(), fc.cpu().numpy(), n.cpu().numpy()


def _assert_same(mesh, f, box, iso):
    v, fc, n = _gpu_isosurface(mesh, f, box, iso)
    rv, rf, rn, _ = M.isosurface(f, box, iso)
    assert v.shape == rv.shape and fc.shape == rf.shape
    assert (v.view(np.uint32) == rv.view(np.uint32)).all()
    assert (fc == rf).all()
    assert np.abs(n - rn).max(initial=0.0) <= 1e-6
    return v, fc


def test_isosurface_equals_restatement(api):
    L, mesh, scene = api
    rng = np.random.default_rng(11)
    box = np.array([-1.0, -0.5, -0.25, 1.0, 0.75, 0.5], np.float32)
    # analytic sphere on a non-cubic lattice
    p = M.lattice_points(box, 40, 31, 23).astype(np.float64)
    v, fc = _assert_same(mesh, (0.3 - np.linalg.norm(p - [0.1, 0.1, 0.1], axis=-1)).astype(np.float32), box, 0.0)
    assert len(fc) > 0 and M.edge_check(fc) == (True, True)
    # uniform noise: all 16 tetrahedron cases
    noise = rng.uniform(0, 1, (19, 23, 29)).astype(np.float32)
    assert set(np.unique(M.tet_cases(noise, 0.5))) == set(range(16))
    _assert_same(mesh, noise, box, 0.5)
    # many values exactly at the level (degenerate triangles kept)
    steps = rng.integers(0, 5, (17, 13, 11)).astype(np.float32)
    assert (steps == 2.0).mean() > 0.1
    _assert_same(mesh, steps, box, 2.0)
    # the smallest lattice
    _assert_same(mesh, rng.uniform(-1, 1, (2, 2, 2)).astype(np.float32), box, 0.0)
    # the density lattice of the synthetic hash scene
    sc = _scene(scene, "cu")
    g = mesh.DensityGrid(sc["renderer"], sc["bbox"], (48, 40, 36)).cpu().numpy()
    iso = float(np.quantile(g, 0.7))
    _assert_same(mesh, g, sc["bbox"], iso)


def test_isosurface_more_than_one_scan_round(api):
    """The block totals are scanned 8 192 blocks of 256 at a time: the 129 x 128 x 128 lattice has 2 113 536 points, 8 256 blocks, so the vertex and the face totals
    need a second round.  All zero but for a few isolated inside points: in block 0, either side of point 2 097 152 (the first of block 8 192), beyond block 8 192
    and in the last block.  Point 2 097 152 lies in the lattice's top plane, so the second round holds vertex counts (and the faces below read those vertex ids);
    a cell's min corner never lies in the top plane, so the face totals of the second round are all zero -- they still pass through the carry."""
    L, mesh, scene = api
    nx, ny, nz = 129, 128, 128
    inside = [(1, 1, 0), (60, 61, 62), (127, 0, 127), (0, 1, 127), (64, 64, 127), (127, 127, 127)]
    lin = [(z * ny + y) * nx + x for x, y, z in inside]
    assert lin[0] < 256 and lin[2] == 8192 * 256 - 1 and lin[3] == 8192 * 256 + 1 and lin[4] // 256 > 8192 and lin[5] // 256 == nx * ny * nz // 256 - 1 == 8255
    f = np.zeros((nz, ny, nx), np.float32)
    for k, (x, y, z) in enumerate(inside):
        f[z, y, x] = 1.0 + 0.25 * k
    box = np.array([-1.0, -0.5, -0.25, 1.0, 0.75, 0.5], np.float32)
    v, fc = _assert_same(mesh, f, box, 0.5)
    # vertices come in the order of their edge's origin: the last ones start in the top plane, beyond block 8 192, and faces use them
    assert len(v) > 40 and len(fc) > 40 and fc.max() == len(v) - 1 and (v[-8:, 2] == box[5]).all()


def test_isosurface_deterministic_256(api):
    L, mesh, scene = api
    sc = _scene(scene, "cu")
    box = sc["bbox"]
    g = mesh.DensityGrid(sc["renderer"], box, 256)
    iso = float(torch.quantile(g.reshape(-1)[::97].float(), 0.7))
    a = mesh.Isosurface(g, box, iso)
    b = mesh.Isosurface(g, box, iso)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    v, fc = a[0].cpu().numpy(), a[1].cpu().numpy().astype(np.int64)
    assert len(fc) > 1000
    # closed and oriented away from the box faces: an edge whose two ends lie on the same face of the box is a boundary edge of the open surface
    d = np.concatenate([fc[:, [0, 1]], fc[:, [1, 2]], fc[:, [2, 0]]])
    on_face = np.zeros(len(d), bool)
    for a_ in range(3):
        for lim in (box[a_], box[3 + a_]):
            on_face |= (v[d[:, 0], a_] == lim) & (v[d[:, 1], a_] == lim)
    d = d[~on_face]
    n = len(v)
    _, uc = np.unique(np.minimum(d[:, 0], d[:, 1]) * n + np.maximum(d[:, 0], d[:, 1]), return_counts=True)
    _, dc = np.unique(d[:, 0] * n + d[:, 1], return_counts=True)
    assert (uc == 2).all() and (dc == 1).all()


def test_nonfinite_lattice(api):
    L, mesh, scene = api
    f = np.random.default_rng(5).uniform(-1, 1, (9, 10, 11)).astype(np.float32)
    f[3, 4, 5] = np.nan
    f[0, 0, 0] = np.inf
    d = torch.from_numpy(f).cuda()
    box = (C.c_float * 6)(-1, -1, -1, 1, 1, 1)
    lib = L.lib()
    ws = torch.empty((int(lib.nrf_isosurface_workspace_bytes(11, 10, 9)),), device="cuda", dtype=torch.uint8)
    nv, nt, nb = C.c_int64(), C.c_int64(), C.c_int64()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.nrf_isosurface_count(C.c_void_p(d.data_ptr()), 11, 10, 9, box, C.c_float(0), C.byref(nv), C.byref(nt), C.byref(nb), C.c_void_p(ws.data_ptr()),
                                    C.c_size_t(ws.numel()), stream) == 0
    assert nb.value == 2 and nv.value > 0
    verts = torch.empty((nv.value, 3), device="cuda"); faces = torch.empty((nt.value, 3), device="cuda", dtype=torch.int32)
    assert lib.nrf_isosurface_emit(C.c_void_p(d.data_ptr()), 11, 10, 9, box, C.c_float(0), C.c_void_p(verts.data_ptr()), C.c_void_p(faces.data_ptr()), None,
                                   nv, nt, C.c_void_p(ws.data_ptr()), C.c_size_t(ws.numel()), stream) == L.NRF_ERR_NONFINITE
    assert b"non-finite" in lib.nrf_last_error()
    with pytest.raises(L.NrfError):
        mesh.Isosurface(d, [-1, -1, -1, 1, 1, 1], 0.0)


def test_extract_mesh_colours_and_ply(api, tmp_path):
    L, mesh, scene = api
    from oracle import capi as O
    sc = _scene(scene, "ngp")
    cfg = sc["cfg"]
    g = mesh.DensityGrid(sc["renderer"], None, 48).cpu().numpy()
    iso = float(np.quantile(g, 0.7))
    m = mesh.ExtractMesh(sc["renderer"], iso, resolution=48)
    v, fc = m.Vertices.cpu().numpy(), m.Faces.cpu().numpy()
    rv, rf, _, _ = M.isosurface(g, sc["bbox"], iso)
    assert (v == rv).all() and (fc == rf).all()
    rgb = m.Colors.cpu().numpy()
    assert rgb.shape == v.shape and (rgb >= 0).all() and (rgb <= 1).all()
    idx = np.random.default_rng(2).choice(len(v), 64, replace=False)
    pts = v[idx]
    dirs = -m.Normals.cpu().numpy()[idx]
    feats, keep = O.hash_ngp(pts, sc["table"], sc["bbox"], cfg["n_levels"], cfg["n_feat"], cfg["log2_t"], cfg["base"], cfg["finest"])
    raw = O.mlp_small(sc["mlp_blob"], np.concatenate([feats, O.sh_libtorch(dirs, cfg["sh_degree"])], 1), 32, 16)
    ref = 1.0 / (1.0 + np.exp(-raw[:, :3].astype(np.float64)))
    assert np.abs(rgb[idx] - ref).max() <= 1e-6
    path = os.path.join(tmp_path, "scene.ply")
    mesh.SavePLY(path, m)
    pv, pf = M.read_ply(path)
    assert len(pv) == len(v) and (np.stack([pv["x"], pv["y"], pv["z"]], 1) == v).all() and (pf["idx"] == fc).all()
    assert (np.stack([pv["red"], pv["green"], pv["blue"]], 1) == np.clip(np.rint(rgb.astype(np.float64) * 255), 0, 255)).all()
