"""Mesh export without a GPU: the numpy restatement of the isosurface contract (tests/mesh_ref.py) pinned on analytic fields, the C entries' argument
validation, and the PLY writer."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mesh_ref as M

BOX = np.array([-1, -1, -1, 1, 1, 1], np.float32)


def sphere(n, r=0.6, centre=(0.05, -0.03, 0.02), box=BOX):
    p = M.lattice_points(box, n, n, n).astype(np.float64)
    return (r - np.linalg.norm(p - np.asarray(centre), axis=-1)).astype(np.float32)


def torus(n, R=0.55, r=0.22, box=BOX):
    p = M.lattice_points(box, n, n, n).astype(np.float64)
    q = np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - R
    return (r - np.sqrt(q ** 2 + p[..., 2] ** 2)).astype(np.float32)


def two_spheres(n, r=0.4, box=BOX):
    p = M.lattice_points(box, n, n, n).astype(np.float64)
    a = r - np.linalg.norm(p - np.array([-r, 0.0, 0.0]), axis=-1)
    b = r - np.linalg.norm(p - np.array([r, 0.0, 0.0]), axis=-1)
    return np.maximum(a, b).astype(np.float32)


def test_case_rules_cover_all_tetrahedra():
    """0/4 corners inside: nothing; 1/3: one triangle; 2: two -- every triangle's edges are crossed edges of the tetrahedron"""
    for odd in (0, 1):
        for m in range(16):
            tris = M.tet_triangles(m, odd)
            pc = bin(m).count("1")
            assert len(tris) == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[pc]
            for t in tris:
                for j, k in t:
                    assert j < k and (m >> j & 1) != (m >> k & 1)


@pytest.mark.parametrize("n", [32, 41])
def test_sphere_closed_oriented_genus0(n):
    f = sphere(n)
    v, fc, nrm, bad = M.isosurface(f, BOX, 0.0)
    assert bad == 0 and len(fc) > 0
    assert M.edge_check(fc) == (True, True)
    assert M.euler(v, fc) == 2
    vol = M.signed_volume(v, fc)
    exact = 4.0 / 3.0 * np.pi * 0.6 ** 3
    assert abs(vol - exact) / exact < 0.03, (vol, exact)
    d = np.einsum("ij,ij->i", nrm.astype(np.float64), v - np.array([0.05, -0.03, 0.02]))
    assert (d > 0).all()
    assert np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-6)


def test_torus_genus1():
    v, fc, _, _ = M.isosurface(torus(48), BOX, 0.0)
    assert M.edge_check(fc) == (True, True)
    assert M.euler(v, fc) == 0
    vol = M.signed_volume(v, fc)
    exact = 2 * np.pi ** 2 * 0.55 * 0.22 ** 2
    assert abs(vol - exact) / exact < 0.05, (vol, exact)


def test_two_touching_spheres_closed():
    v, fc, _, _ = M.isosurface(two_spheres(40), BOX, 0.0)
    assert M.edge_check(fc) == (True, True)
    assert M.euler(v, fc) in (2, 4)           # joined at the touching point or not, depending on the lattice
    vol = M.signed_volume(v, fc)
    exact = 2 * 4.0 / 3.0 * np.pi * 0.4 ** 3
    assert abs(vol - exact) / exact < 0.04, (vol, exact)


def test_inverted_field_flips_orientation():
    """inside/outside swapped (f -> -f, iso 0 -> a value just below): the same surface with every triangle wound the other way"""
    f = sphere(33)
    v, fc, _, _ = M.isosurface(f, BOX, 0.0)
    v2, fc2, _, _ = M.isosurface(-f, BOX, np.float32(-1e-30))
    assert M.signed_volume(v, fc) > 0 > M.signed_volume(v2, fc2)


def test_workspace_and_validation_need_no_gpu():
    from nerfpp_amd import _lib
    lib = _lib.lib()
    box = (C.c_float * 6)(*BOX)
    bad_box = (C.c_float * 6)(-1, -1, 1, 1, 1, -1)
    fake = C.c_void_p(1 << 20)             # never dereferenced: every check below fails before any launch
    nv, nt, nb = C.c_int64(), C.c_int64(), C.c_int64()
    small = lib.nrf_isosurface_workspace_bytes(8, 8, 8)
    assert small > 0 and lib.nrf_isosurface_workspace_bytes(16, 16, 16) > small and lib.nrf_isosurface_workspace_bytes(1, 8, 8) == 0

    def count(nx, ny, nz, bb, iso, wsb):
        return lib.nrf_isosurface_count(fake, nx, ny, nz, bb, C.c_float(iso), C.byref(nv), C.byref(nt), C.byref(nb), fake, C.c_size_t(wsb), None)

    def emit(nx, ny, nz, bb, iso, wsb):
        return lib.nrf_isosurface_emit(fake, nx, ny, nz, bb, C.c_float(iso), fake, fake, fake, C.c_int64(0), C.c_int64(0), fake, C.c_size_t(wsb), None)

    for call, name in ((count, b"nrf_isosurface_count"), (emit, b"nrf_isosurface_emit")):
        assert call(1, 8, 8, box, 0.0, small) == 1 and name in lib.nrf_last_error()            # dimension below 2
        assert call(8, 8, 8, bad_box, 0.0, small) == 1 and name in lib.nrf_last_error()        # inverted box
        assert call(8, 8, 8, box, float("nan"), small) == 1 and name in lib.nrf_last_error()   # NaN iso
        assert call(8, 8, 8, box, float("inf"), small) == 1
        assert call(8, 8, 8, box, 0.0, small - 1) == 4 and name in lib.nrf_last_error()        # NRF_ERR_WORKSPACE
    assert lib.nrf_isosurface_emit(fake, 8, 8, 8, box, C.c_float(0), fake, fake, None, C.c_int64(1 << 31), C.c_int64(0), fake, C.c_size_t(small), None) == 1
    # density grid: a renderer needs a device, so a NULL one is the argument error to see here
    assert lib.nrf_density_grid(None, box, 8, 8, 8, fake, C.c_int64(0), fake, C.c_size_t(1 << 30), None) == 1
    assert b"nrf_density_grid" in lib.nrf_last_error()
    assert lib.nrf_density_grid_workspace_bytes(None, 8, 8, 8, C.c_int64(0)) == 0


def test_save_ply_round_trip(tmp_path):
    from nerfpp_amd.mesh import Mesh, SavePLY
    v, fc, nrm, _ = M.isosurface(sphere(17), BOX, 0.0)
    rgb = np.random.default_rng(3).uniform(-0.1, 1.1, (len(v), 3)).astype(np.float32)
    rgb[:4] = [[0, 0, 0], [1, 1, 1], [0.5 / 255, 1.5 / 255, 254.5 / 255], [0.2, 0.4, 0.6]]
    mesh = Mesh(torch.from_numpy(v), torch.from_numpy(fc), torch.from_numpy(nrm), torch.from_numpy(rgb))
    path = os.path.join(tmp_path, "sphere.ply")
    SavePLY(path, mesh)
    rv, rf = M.read_ply(path)
    assert (np.stack([rv["x"], rv["y"], rv["z"]], 1) == v).all()
    assert (np.stack([rv["nx"], rv["ny"], rv["nz"]], 1) == nrm).all()
    assert (rf["n"] == 3).all() and (rf["idx"] == fc).all()
    c = np.stack([rv["red"], rv["green"], rv["blue"]], 1)
    assert (c == np.clip(np.rint(rgb.astype(np.float64) * 255), 0, 255).astype(np.uint8)).all()
    assert list(c[0]) == [0, 0, 0] and list(c[1]) == [255, 255, 255]
    SavePLY(path, Mesh(mesh.Vertices, mesh.Faces, mesh.Normals))           # no colours: no colour properties
    rv, rf = M.read_ply(path)
    assert "red" not in rv.dtype.names and len(rv) == len(v) and (rf["idx"] == fc).all()
