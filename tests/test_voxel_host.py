"""The mesh voxeliser without a GPU: the definition (tests/voxel_ref.py, the numpy restatement the GPU tests compare nrf_mesh_voxelize with bit for bit) pinned on
facts that do not depend on it -- cubes between and on lattice planes, inverted and nested shells, permutations, an axis-aligned plane; the header, the binding and
the refusals of the C entry (they come before any device call)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import voxel_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
INVALID_ARG = 1
BBOX, DIMS = VR.LATTICE_EXACT          # steps of exactly 0.25


def _winding(mesh, bbox=BBOX, dims=DIMS):
    delta, stats, _ = VR.delta_of(mesh[0], mesh[1], bbox, dims)
    assert stats[0] == 0
    return VR.winding_of(delta)


def _strictly_inside(lo, hi, bbox=BBOX, dims=DIMS):
    P = VR.lattice_points(bbox, dims).astype(np.float64)
    return ((P > np.asarray(lo, np.float64)) & (P < np.asarray(hi, np.float64))).all(-1)


def test_header_binding_and_constants_agree():
    from nerfpp_amd import _lib, voxel
    hdr = open(os.path.join(ROOT, "include", "nerfpp_hip.h")).read()
    for name, value in (("NRF_VOXEL_WIDE_COLUMNS", voxel.WIDE_COLUMNS), ("NRF_VOXEL_WIDE_POINTS", voxel.WIDE_POINTS), ("NRF_VOX_NONZERO", VR.NONZERO),
                        ("NRF_VOX_POSITIVE", VR.POSITIVE), ("NRF_VOX_ODD", VR.ODD), ("NRF_RASTER_SUBPIXEL", VR.SUBPIXEL), ("NRF_RASTER_GUARD", VR.GUARD)):
        m = re.findall(rf"#define\s+{name}\s+(\d+)", hdr)
        assert len(m) == 1 and int(m[0]) == value, name          # one definition: the rasteriser's constants are reused, not redefined
    assert voxel.RULES == {"nonzero": VR.NONZERO, "positive": VR.POSITIVE, "odd": VR.ODD}
    assert (_lib.NRF_VOX_NONZERO, _lib.NRF_VOX_POSITIVE, _lib.NRF_VOX_ODD) == VR.RULES
    assert re.search(r"NRF_API size_t nrf_mesh_voxelize_workspace_bytes\(", hdr) and re.search(r"NRF_API int nrf_mesh_voxelize\(", hdr)
    for words in ("WHY THE BOX IS COMPLETE", "WHY THE WINDING OF A CLOSED MESH IS EXACT", "VOIDS THE WINDING"):
        assert words in hdr, words
    assert _lib.SIGNATURES["nrf_mesh_voxelize_workspace_bytes"] == ("z", "lliii")
    assert _lib.SIGNATURES["nrf_mesh_voxelize"] == ("i", "plplpiiifipppppzp")
    at = _lib.SYMBOLS.index("nrf_mesh_ambient_occlusion")
    assert _lib.SYMBOLS[at + 1:at + 3] == ["nrf_mesh_voxelize_workspace_bytes", "nrf_mesh_voxelize"], "in the header's order"
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "nrf_mesh_voxelize") and hasattr(lib, "nrf_mesh_voxelize_workspace_bytes")
    import nerfpp_amd
    assert "voxel" in nerfpp_amd.__all__ and nerfpp_amd.voxel is voxel
    for name in ("WindingGrid", "MeshToSDF", "SDFVolume", "RemeshUnion", "VoxelVolume", "VolumeIoU"):
        assert hasattr(voxel, name), name
    import inspect
    from nerfpp_amd import mesh
    assert inspect.signature(mesh.ExtractMesh).parameters["union_resolution"].default is None


def test_closest_point_lives_in_the_shared_header():
    """cm_closest and CmHit moved to face_grid.h: one definition, and geometry.hip includes it"""
    src = {n: open(os.path.join(ROOT, "nerfpp_amd", "csrc", n)).read() for n in ("face_grid.h", "geometry.hip", "voxel.hip")}
    assert len(re.findall(r"void cm_closest\(", src["face_grid.h"])) == 1 and "struct CmHit" in src["face_grid.h"]
    for n in ("geometry.hip", "voxel.hip"):
        assert "void cm_closest(" not in src[n] and "struct CmHit" not in src[n] and '#include "face_grid.h"' in src[n] and "cm_closest(" in src[n], n


def test_workspace_size_and_refusals_need_no_gpu():
    """Every bad argument of the header is refused before anything touches the device, so the whole list is checked here; the GPU test repeats it over live buffers."""
    from nerfpp_amd import _lib
    lib = _lib.lib()
    size = lib.nrf_mesh_voxelize_workspace_bytes
    n = 9 * 5 * 17
    assert size(8, 12, 9, 5, 17) >= 8 * 16 + 2 * 12 * 4 + 8 + n * 4 + n * 8
    assert size(0, 0, 2, 2, 2) > 0
    for bad in ((-1, 1, 4, 4, 4), (1, -1, 4, 4, 4), (1, 2 ** 31 - 1, 4, 4, 4), (2 ** 31, 1, 4, 4, 4), (1, 1, 1, 4, 4), (1, 1, 4, 1, 4), (1, 1, 4, 4, 1), (1, 1, 4, 4, 0),
                (1, 1, 2048, 1024, 1024), (1, 1, 2 ** 30, 2, 2)):
        assert size(*bad) == 0, bad
    assert size(1, 1, 2047, 1024, 1024) > 12 * (2 ** 31 - 2 ** 20)
    box = BBOX.copy()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(256)          # never dereferenced: every call below is refused

    def call(verts=fake, nv=8, faces=fake, nf=12, bbox=p(box), nx=9, ny=5, nz=17, trunc=0.5, rule=0, winding=fake, sdf=fake, face=fake, ws=fake, ws_bytes=1 << 40):
        return lib.nrf_mesh_voxelize(verts, nv, faces, nf, bbox, nx, ny, nz, trunc, rule, winding, sdf, face, None, ws, ws_bytes, None)

    nan, inf = float("nan"), float("inf")
    boxes = [np.array(b, F32) for b in ([0, 0, 0, 0, 1, 1], [0, 0, 0, 1, -1, 1], [0, 0, 0, 1, 1, nan], [0, -inf, 0, 1, 1, 1], [0, 0, 0, inf, 1, 1], [1, 1, 1, 0, 0, 0])]
    full, winding_only = size(8, 12, 9, 5, 17), size(8, 12, 9, 5, 17) - 8 * n
    bad = [dict(bbox=None), dict(faces=None), dict(verts=None), dict(winding=None, sdf=None, face=None), dict(nx=1), dict(ny=1), dict(nz=1), dict(nz=0), dict(nx=-4),
           dict(nx=2048, ny=1024, nz=1024), dict(trunc=0.0), dict(trunc=-1.0), dict(trunc=nan), dict(trunc=inf), dict(trunc=nan, winding=None), dict(trunc=0.0, sdf=None),
           dict(rule=3), dict(rule=-1), dict(nf=-1), dict(nf=2 ** 31 - 1), dict(nv=-1), dict(nv=2 ** 31), dict(ws=None), dict(ws=C.c_void_p(264)), dict(ws=C.c_void_p(128)),
           dict(ws_bytes=full - 1), dict(ws_bytes=0), dict(ws_bytes=winding_only - 256, sdf=None, face=None), dict(ws_bytes=winding_only, face=None)]
    bad += [dict(bbox=p(b)) for b in boxes]
    for kw in bad:
        assert call(**kw) == INVALID_ARG, kw
        assert lib.nrf_last_error().startswith(b"nrf_mesh_voxelize"), (kw, lib.nrf_last_error())


def test_cube_between_lattice_planes_is_one_strictly_inside_and_zero_elsewhere():
    lo, hi = (-0.6, -0.3, -0.9), (0.55, 0.35, 0.6)
    w = _winding(VR.cube(lo, hi))
    inside = _strictly_inside(lo, hi)
    assert inside.sum() == 5 * 3 * 6 and np.array_equal(w, inside.astype(np.int32))


@pytest.mark.parametrize("name", ["exact", "inexact"])
def test_cube_with_vertices_on_columns_counts_every_edge_and_corner_column_once(name):
    """Vertices ON lattice columns: the top-left rule gives every edge and corner column to exactly one of the faces that meet there, so top and bottom cover the same
    columns once each -- no column sums to 2 or to -1 anywhere above or below the solid, and every column nets 0 below it"""
    bbox, dims = VR.LATTICES[name]
    P = VR.lattice_points(bbox, dims)
    lo = (P[0, 1, 1, 0], P[0, 1, 1, 1], F32(-0.6))
    hi = (P[0, -2, -2, 0], P[0, -2, -2, 1], F32(0.3))
    mesh = VR.cube(lo, hi)
    delta, stats, covered = VR.delta_of(mesh[0], mesh[1], bbox, dims)
    w = VR.winding_of(delta)
    assert set(np.unique(w)) == {0, 1}
    up, down = (covered > 0).sum(0), (covered < 0).sum(0)
    assert up.max() == 1 and down.max() == 1 and np.array_equal(up, down)          # the side faces have no projected area
    # the rule is top-left: the columns on the low-x and low-y edges belong to the solid, those on the high edges do not
    nx, ny, _ = dims
    want = np.zeros((ny, nx), bool)
    want[1:ny - 2, 1:nx - 2] = True
    assert np.array_equal(up.astype(bool), want)
    z = P[:, 0, 0, 2].astype(np.float64)
    levels = (z > -0.6) & (z < 0.3)
    assert np.array_equal(w, (levels[:, None, None] & want[None]).astype(np.int32))


def test_inverted_and_nested_shells_and_the_three_rules():
    m = VR.meshes()
    outer, inner = _strictly_inside((-0.8, -0.4, -0.9), (0.8, 0.4, 0.6)), _strictly_inside((-0.3, -0.2, -0.4), (0.3, 0.2, 0.3))
    assert inner.sum() > 0 and (outer & ~inner).sum() > 0
    assert np.array_equal(_winding(m["cube_inverted"]), -_strictly_inside((-0.6, -0.3, -0.9), (0.55, 0.35, 0.6)).astype(np.int32))
    like = _winding(m["cube_nested_like"])
    assert np.array_equal(like, outer.astype(np.int32) + inner.astype(np.int32)) and like.max() == 2
    cavity = _winding(m["cube_nested_cavity"])
    assert np.array_equal(cavity, outer.astype(np.int32) - inner.astype(np.int32)) and (cavity[inner] == 0).all()
    # nonzero merges the like-oriented shells, odd carves the inner one out; an inverted solid is inside under nonzero and odd, empty under positive
    assert np.array_equal(VR.inside_of(like, VR.NONZERO), outer) and np.array_equal(VR.inside_of(like, VR.POSITIVE), outer)
    assert np.array_equal(VR.inside_of(like, VR.ODD), outer & ~inner)
    for rule in VR.RULES:
        assert np.array_equal(VR.inside_of(cavity, rule), outer & ~inner)
    inv = _winding(m["cube_inverted"])
    assert VR.inside_of(inv, VR.NONZERO).sum() == VR.inside_of(inv, VR.ODD).sum() == 90 and not VR.inside_of(inv, VR.POSITIVE).any()


def test_permutations_and_corner_rotations_leave_the_winding_unchanged():
    rng = np.random.default_rng(7)
    for name in ("icosphere", "cube_on_columns", "twin_vertices", "beyond_box"):
        V, Fc = VR.meshes()[name]
        for bbox, dims in VR.LATTICES.values():
            want = VR.delta_of(V, Fc, bbox, dims)[0]
            perm = rng.permutation(len(Fc))
            rot = np.stack([np.roll(f, rng.integers(0, 3)) for f in Fc[perm]])
            assert np.array_equal(VR.delta_of(V, rot, bbox, dims)[0], want), name


def test_sdf_of_a_large_plane_is_the_height_above_it():
    """|sdf| of a large axis-aligned plane equals the lattice point's height above it, exactly, at power-of-two steps"""
    bbox, dims = BBOX, DIMS
    V = np.array([[-64, -64, -0.75], [64, -64, -0.75], [64, 64, -0.75], [-64, 64, -0.75]], F32)
    Fc = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    trunc = 1.0
    out = VR.voxelize(V, Fc, bbox, dims, trunc, VR.NONZERO)
    z = VR.lattice_points(bbox, dims)[..., 2]
    height = np.abs(z - F32(-0.75))
    assert np.array_equal(np.abs(out["sdf"]), np.minimum(height, F32(trunc)))
    assert np.array_equal(out["face"] >= 0, height <= F32(trunc)) and (out["face"] <= 1).all()
    assert np.array_equal(out["sdf"] < 0, (z < F32(-0.75)) & (height > 0))          # one +z-facing sheet above: below the plane counts as inside


def test_the_box_of_step_7_changes_nothing():
    """WHY THE BOX IS COMPLETE, on the test meshes: every face against every lattice point gives the keys the boxes give"""
    for name in ("icosphere", "beyond_box", "quad_stack", "bad_and_nan"):
        V, Fc = VR.meshes()[name]
        for bbox, dims in VR.LATTICES.values():
            for steps in (1.5, 3.0):
                trunc = F32(steps) * VR.lattice(bbox, dims)[1].max()
                assert np.array_equal(VR.keys_of(V, Fc, bbox, dims, trunc, True), VR.keys_of(V, Fc, bbox, dims, trunc, False)), (name, steps)
