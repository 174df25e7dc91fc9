"""The mesh voxeliser on the MI355X: nrf_mesh_voxelize against the numpy restatement (tests/voxel_ref.py) bit for bit -- winding, signed distance, face and
statistics -- on cubes, an icosphere, open, degenerate, contended, invalid and out-of-box meshes and on meshes that take the wide kernel; the permutation and
run-to-run guarantees, the agreement with ClosestOnMesh, the refusals, and the Python layer built on it: MeshToSDF, SDFVolume.Extract, RemeshUnion and VolumeIoU."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import voxel_ref as VR

pytestmark = pytest.mark.gpu

INVALID_ARG = 1
F32 = np.float32
MESHES = VR.meshes()
TRUNC_STEPS = (1.5, 3.0)


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from nerfpp_amd import _lib as L, geometry, mesh, voxel
    return L, voxel, mesh, geometry


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def trunc_of(bbox, dims, steps):
    return float(F32(steps) * VR.lattice(bbox, dims)[1].max())


def run(api, verts, faces, bbox, dims, trunc, rule, skip=(), stats=None, ws_bytes=None):
    """The C entry itself -> dict of numpy arrays (None for the outputs named in `skip`: they are passed as NULL); stats: a device tensor to add to"""
    lib = api[0].lib()
    nx, ny, nz = dims
    dv = torch.from_numpy(np.ascontiguousarray(verts, F32).reshape(-1, 3)).cuda()
    df = torch.from_numpy(np.ascontiguousarray(faces, np.int32).reshape(-1, 3)).cuda()
    out = {n: None if n in skip else torch.full((nz, ny, nx), -7, dtype=t, device="cuda") for n, t in (("winding", torch.int32), ("sdf", torch.float32), ("face", torch.int32))}
    if stats is None:
        stats = torch.zeros((4,), dtype=torch.int32, device="cuda")
    need = int(lib.nrf_mesh_voxelize_workspace_bytes(len(dv), len(df), nx, ny, nz)) if ws_bytes is None else ws_bytes
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    p = lambda t: None if t is None else t.data_ptr()
    box = np.ascontiguousarray(bbox, F32)
    status = lib.nrf_mesh_voxelize(p(dv), len(dv), p(df), len(df), box.ctypes.data_as(C.c_void_p), nx, ny, nz, trunc, rule, p(out["winding"]), p(out["sdf"]),
                                   p(out["face"]), p(stats), p(ws), ws.numel(), None)
    assert status == 0, lib.nrf_last_error()
    torch.cuda.synchronize()
    res = {n: None if t is None else t.cpu().numpy() for n, t in out.items()}
    res["stats"] = stats.cpu().numpy().view(np.uint32)
    return res


@functools.lru_cache(maxsize=None)
def reference(name, lattice, steps):
    """The restatement of one mesh on one lattice at one truncation, under the non-zero rule: computed once, shared, never written to"""
    V, Fc = MESHES[name]
    bbox, dims = VR.LATTICES[lattice]
    return VR.voxelize(V, Fc, bbox, dims, trunc_of(bbox, dims, steps), VR.NONZERO)


def same(got, want, rule):
    """Bit for bit: winding, sdf (the restatement's distance signed by `rule`), face and stats"""
    sdf = np.where(VR.inside_of(want["winding"], rule), -np.abs(want["sdf"]), np.abs(want["sdf"])).astype(F32)
    assert np.array_equal(got["winding"], want["winding"])
    assert np.array_equal(bits(got["sdf"]), bits(sdf))
    assert np.array_equal(got["face"], want["face"])
    assert np.array_equal(got["stats"], want["stats"])


@pytest.mark.parametrize("lattice", sorted(VR.LATTICES))
@pytest.mark.parametrize("name", sorted(MESHES))
def test_bit_for_bit_against_the_restatement(api, name, lattice):
    V, Fc = MESHES[name]
    bbox, dims = VR.LATTICES[lattice]
    for steps in TRUNC_STEPS:
        want = reference(name, lattice, steps)
        for rule in VR.RULES:
            same(run(api, V, Fc, bbox, dims, trunc_of(bbox, dims, steps), rule), want, rule)
    # what the cases are there to exercise is there
    w = reference(name, lattice, 3.0)
    expect = {"cube_inverted": lambda: w["winding"].min() == -1, "cube_nested_like": lambda: w["winding"].max() == 2, "quad_stack": lambda: w["winding"].max() == 2,
              "bad_and_nan": lambda: tuple(w["stats"]) == (0, 2, 1, 0), "z_parallel": lambda: not w["winding"].any() and (w["face"] >= 0).any(),
              "beyond_box": lambda: w["winding"].max() >= 1 and (w["winding"][-1] != 0).any()}
    assert expect.get(name, lambda: True)(), name


def test_wide_paths_equal_the_restatement_and_the_split_mesh(api):
    """Two triangles of 1089 columns each beside 40 small ones: the wide kernel's columns and lattice boxes against the restatement; the winding also against the same
    mesh with the wide faces split where coverage is exact"""
    bbox, dims, wide, split = VR.wide_case()
    trunc = trunc_of(bbox, dims, 3.0)
    want = VR.voxelize(wide[0], wide[1], bbox, dims, trunc, VR.NONZERO)
    delta, _, covered = VR.delta_of(wide[0], wide[1], bbox, dims)
    assert (np.abs(covered[:2]).sum((1, 2)) > api[1].WIDE_COLUMNS).all() and np.abs(covered[:2]).sum() == 33 * 33          # every column, each by one of the two
    got = run(api, wide[0], wide[1], bbox, dims, trunc, VR.NONZERO)
    same(got, want, VR.NONZERO)
    got_split = run(api, split[0], split[1], bbox, dims, trunc, VR.NONZERO)
    assert np.array_equal(got_split["winding"], got["winding"])
    same(got_split, VR.voxelize(split[0], split[1], bbox, dims, trunc, VR.NONZERO), VR.NONZERO)


@pytest.mark.parametrize("name", ["icosphere", "quad_stack", "beyond_box"])
def test_permutation_and_repeatability(api, name):
    V, Fc = MESHES[name]
    bbox, dims = VR.LATTICE_INEXACT
    trunc = trunc_of(bbox, dims, 3.0)
    a, b = (run(api, V, Fc, bbox, dims, trunc, VR.ODD) for _ in range(2))
    perm = np.random.default_rng(3).permutation(len(Fc))
    c = run(api, V, Fc[perm], bbox, dims, trunc, VR.ODD)
    for other in (b, c):
        assert np.array_equal(a["winding"], other["winding"]) and np.array_equal(bits(a["sdf"]), bits(other["sdf"])) and np.array_equal(a["stats"], other["stats"])
    assert np.array_equal(a["face"], b["face"])
    # the permuted list names faces by their new index; on an exact tie of d2 it may name another face of the same distance
    found = a["face"] >= 0
    assert np.array_equal(found, c["face"] >= 0)
    if name == "icosphere":          # no two faces of it are coincident: the nearest face is the same face
        assert np.array_equal(bits(a["sdf"]), bits(c["sdf"]))


def test_null_outputs(api):
    V, Fc = MESHES["icosphere"]
    bbox, dims = VR.LATTICE_EXACT
    want = reference("icosphere", "exact", 3.0)
    n = dims[0] * dims[1] * dims[2]
    full = int(api[0].lib().nrf_mesh_voxelize_workspace_bytes(len(V), len(Fc), *dims))
    # winding alone: trunc is not read, and the workspace may leave out the key lattice
    alone = run(api, V, Fc, bbox, dims, float("nan"), VR.NONZERO, skip=("sdf", "face"), ws_bytes=full - 8 * n)
    assert np.array_equal(alone["winding"], want["winding"]) and alone["sdf"] is None
    trunc = trunc_of(bbox, dims, 3.0)
    for skip in (("winding",), ("face",), ("sdf",), ("winding", "face"), ("winding", "sdf")):
        got = run(api, V, Fc, bbox, dims, trunc, VR.NONZERO, skip=skip)
        for k in ("winding", "sdf", "face"):
            assert got[k] is None if k in skip else np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (skip, k)


def test_empty_face_list_and_added_stats(api):
    bbox, dims = VR.LATTICE_INEXACT
    trunc = trunc_of(bbox, dims, 1.5)
    got = run(api, np.zeros((0, 3), F32), np.zeros((0, 3), np.int32), bbox, dims, trunc, VR.NONZERO)
    assert not got["winding"].any() and (got["face"] == -1).all() and np.array_equal(bits(got["sdf"]), bits(np.full(got["sdf"].shape, trunc, F32)))
    stats = torch.tensor([5, 6, 7, 8], dtype=torch.int32, device="cuda")
    V, Fc = MESHES["bad_and_nan"]
    got = run(api, V, Fc, bbox, dims, trunc, VR.NONZERO, stats=stats)
    assert tuple(got["stats"]) == (5, 8, 8, 8)          # ADDED to; [3] untouched
    # faces beyond the guard band are clipped from the winding pass only: counted, and still found by the distance pass
    far = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1e9, 0, 0]], F32)
    got = run(api, far, np.array([[0, 1, 2], [0, 1, 3]], np.int32), bbox, dims, trunc, VR.NONZERO)
    want = VR.voxelize(far, np.array([[0, 1, 2], [0, 1, 3]], np.int32), bbox, dims, trunc, VR.NONZERO)
    assert tuple(want["stats"]) == (1, 0, 0, 0)
    same(got, want, VR.NONZERO)


def test_keys_agree_with_closest_on_mesh(api):
    """The key lattice is nrf_closest_on_mesh(max_dist = trunc) at the lattice points: the same face, and the same d2 under the square root"""
    _, voxel, M, G = api
    for name in ("icosphere", "beyond_box"):
        V, Fc = MESHES[name]
        mesh = M.Mesh(torch.from_numpy(V).cuda(), torch.from_numpy(Fc).cuda(), torch.zeros((len(V), 3), device="cuda"))
        for lattice, (bbox, dims) in VR.LATTICES.items():
            trunc = trunc_of(bbox, dims, 3.0)
            got = run(api, V, Fc, bbox, dims, trunc, VR.NONZERO)
            pts = torch.from_numpy(VR.lattice_points(bbox, dims).reshape(-1, 3)).cuda()
            res = G.ClosestOnMesh(pts, mesh, max_dist=trunc, uv=False, points=False)
            face, d2 = res.Face.cpu().numpy().reshape(got["face"].shape), res.Dist2.cpu().numpy().reshape(got["face"].shape)
            assert np.array_equal(got["face"], face) and (face >= 0).any() and ((face < 0).any() or name != "icosphere"), (name, lattice)
            dist = np.minimum(np.where(face >= 0, np.sqrt(d2), F32(trunc)), F32(trunc)).astype(F32)
            assert np.array_equal(bits(np.abs(got["sdf"])), bits(dist)), (name, lattice)


def test_refusals_leave_the_outputs_untouched(api):
    lib = api[0].lib()
    V, Fc = MESHES["cube_between"]
    bbox, dims = VR.LATTICE_EXACT
    nx, ny, nz = dims
    dv, df = torch.from_numpy(V).cuda(), torch.from_numpy(Fc).cuda()
    outs = [torch.full((nz, ny, nx), -7, dtype=t, device="cuda") for t in (torch.int32, torch.float32, torch.int32)]
    stats = torch.full((4,), 9, dtype=torch.int32, device="cuda")
    full = int(lib.nrf_mesh_voxelize_workspace_bytes(len(V), len(Fc), nx, ny, nz))
    ws = torch.empty((full + 256,), dtype=torch.uint8, device="cuda")
    box = np.ascontiguousarray(bbox, F32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(verts=dv.data_ptr(), nv=len(V), faces=df.data_ptr(), nf=len(Fc), bb=p(box), nx=nx, ny=ny, nz=nz, trunc=0.5, rule=0, w=outs[0].data_ptr(), s=outs[1].data_ptr(),
             f=outs[2].data_ptr(), ws_ptr=ws.data_ptr(), ws_bytes=full):
        return lib.nrf_mesh_voxelize(verts, nv, faces, nf, bb, nx, ny, nz, trunc, rule, w, s, f, stats.data_ptr(), ws_ptr, ws_bytes, None)

    nan = float("nan")
    inverted = np.array([1, 1, 1, 0, 0, 0], F32)
    bad = [dict(bb=None), dict(faces=None), dict(verts=None), dict(w=None, s=None, f=None), dict(nx=1), dict(nz=0), dict(nx=2048, ny=1024, nz=1024), dict(bb=p(inverted)),
           dict(trunc=0.0), dict(trunc=nan), dict(trunc=float("inf")), dict(trunc=-1.0, w=None, s=None), dict(rule=3), dict(rule=-1), dict(nf=-1), dict(nv=2 ** 31),
           dict(ws_ptr=None), dict(ws_ptr=ws.data_ptr() + 8), dict(ws_bytes=full - 1), dict(ws_bytes=0)]
    for kw in bad:
        assert call(**kw) == INVALID_ARG, kw
        assert lib.nrf_last_error().startswith(b"nrf_mesh_voxelize"), (kw, lib.nrf_last_error())
    torch.cuda.synchronize()
    assert all((o == -7).all() for o in outs) and (stats == 9).all()
    assert call() == 0          # the same buffers are accepted once the arguments are good


@pytest.fixture(scope="module")
def sphere_volume(api):
    """MeshToSDF of an icosphere at 33^3 with the default box and truncation: shared by the round-trip tests, never written to"""
    _, voxel, M, _ = api
    V, Fc = VR.icosphere(0.8, (0.1, -0.05, 0.2), 2)
    colors = torch.from_numpy((0.5 + 0.5 * V / 1.2).astype(F32)).cuda()
    mesh = M.Mesh(torch.from_numpy(V).cuda(), torch.from_numpy(Fc).cuda(), torch.from_numpy((V - np.array([0.1, -0.05, 0.2], F32)) / F32(0.8)).cuda(), colors)
    return mesh, voxel.MeshToSDF(mesh, resolution=33)


def test_round_trip_is_closed_manifold_and_within_a_lattice_diagonal(api, sphere_volume):
    """The remesh is marching tetrahedra on a lattice of that step: each of its vertices lies on a lattice edge whose ends the source surface separates, so neither
    surface strays further from the other than the diagonal of one cell"""
    _, voxel, M, G = api
    mesh, vol = sphere_volume
    assert tuple(vol.sdf.shape) == (33, 33, 33) and int(vol.stats.sum()) == 0
    assert float(vol.sdf.abs().max()) <= vol.trunc and float(vol.sdf.min()) == -vol.trunc and float(vol.sdf.max()) == vol.trunc
    rim = torch.ones_like(vol.sdf, dtype=torch.bool)
    rim[1:-1, 1:-1, 1:-1] = False
    assert (vol.sdf[rim] == vol.trunc).all() and not vol.winding[rim].any()          # the surface never touches the lattice's rim
    out = vol.Extract()
    topo = M.MeshTopology(out)
    assert topo["closed"] and topo["manifold"] and topo["euler"] == 2 and out.Faces.shape[0] > 1000
    step = (vol.bbox[3:] - vol.bbox[:3]) / 32.0
    diagonal = float(np.linalg.norm(step))
    d = G.SurfaceDistance(out, mesh, n_points=20000, to="surface")
    print(f"round trip: Hausdorff {float(d.Hausdorff):.5f}, lattice diagonal {diagonal:.5f}, Chamfer {float(d.Chamfer):.5f}")
    assert float(d.Hausdorff) < diagonal
    # the volume of the solid, to the lattice's resolution (the icosphere is inscribed in the sphere of radius 0.8)
    sphere = 4.0 / 3.0 * np.pi * 0.8 ** 3
    volume = float(voxel.VoxelVolume(mesh, vol.bbox, 33))
    assert 0.85 * sphere < volume < 1.02 * sphere


def test_offsets_attributes_and_inside(api, sphere_volume):
    _, voxel, M, G = api
    mesh, vol = sphere_volume
    centre = torch.tensor([0.1, -0.05, 0.2], device="cuda")
    radius = {o: torch.linalg.vector_norm(vol.Extract(offset=o).Vertices - centre, dim=1) for o in (-0.1, 0.0, 0.1)}
    assert float(radius[-0.1].max()) < float(radius[0.0].min()) + 0.03 and float(radius[0.0].max()) < float(radius[0.1].min()) + 0.03
    assert abs(float(radius[0.1].mean()) - float(radius[0.0].mean()) - 0.1) < 0.02 and abs(float(radius[0.0].mean()) - float(radius[-0.1].mean()) - 0.1) < 0.02
    with pytest.raises(api[0].NrfError):
        vol.Extract(offset=vol.trunc)
    out = vol.Extract(attributes=True)
    want = 0.5 + 0.5 * out.Vertices / 1.2          # the source's colours are linear in position: interpolation reproduces them on its faces
    assert out.Colors.shape == out.Vertices.shape and float((out.Colors - want).abs().max()) < 0.05
    assert float((torch.linalg.vector_norm(out.Normals, dim=1) - 1).abs().max()) < 1e-5
    pts = torch.tensor([[0.1, -0.05, 0.2], [0.1, -0.05, 0.7], [0.1, 0.95, 0.2], [5.0, 0.0, 0.0], [float("nan"), 0.0, 0.0]], device="cuda")
    assert vol.Inside(pts).tolist() == [True, True, False, False, False]


def test_volumetric_iou(api):
    _, voxel, M, _ = api
    bbox, dims = VR.LATTICE_EXACT

    def mesh(vf):
        return M.Mesh(torch.from_numpy(vf[0]).cuda(), torch.from_numpy(vf[1]).cuda(), torch.zeros((len(vf[0]), 3), device="cuda"))
    a, b = VR.cube((-0.75, -0.25, -1.0), (0.25, 0.25, 1.0)), VR.cube((-0.25, -0.25, -1.0), (0.75, 0.25, 1.0))          # lattice-aligned, overlapping by half
    far = VR.cube((0.5, -0.25, -1.0), (0.75, 0.25, 1.0))
    resolution = dims
    iou, n_i, n_u = voxel.VolumeIoU(mesh(a), mesh(a), bbox, resolution)
    assert float(iou) == 1.0 and int(n_i) == int(n_u) > 0 and iou.dtype == torch.float64
    iou, n_i, n_u = voxel.VolumeIoU(mesh(a), mesh(far), bbox, resolution)
    assert float(iou) == 0.0 and int(n_i) == 0 and int(n_u) > 0
    ia, ib = (VR.inside_of(VR.winding_of(VR.delta_of(m[0], m[1], bbox, dims)[0]), VR.NONZERO) for m in (a, b))
    iou, n_i, n_u = voxel.VolumeIoU(mesh(a), mesh(b), bbox, resolution)
    assert (int(n_i), int(n_u)) == (int((ia & ib).sum()), int((ia | ib).sum())) and int(n_i) > 0
    assert float(iou) == int(n_i) / int(n_u) and 0.25 < float(iou) < 0.45
    assert float(voxel.VolumeIoU(mesh(a), mesh(b), None, 33)[0]) == pytest.approx(1.0 / 3.0, abs=0.07)          # default box: the padded bounds of both; 8 of 24 columns, each count within one


def test_union_drops_the_inner_shell(api):
    _, voxel, M, _ = api
    V, Fc = MESHES["cube_nested_like"]
    mesh = M.Mesh(torch.from_numpy(V).cuda(), torch.from_numpy(Fc).cuda(), torch.zeros((len(V), 3), device="cuda"))
    assert M.MeshComponents(mesh)[1] == 2
    union = voxel.RemeshUnion(mesh, resolution=41)
    assert M.MeshComponents(union)[1] == 1 and M.MeshTopology(union)["closed"]
    assert M.MeshComponents(voxel.RemeshUnion(mesh, resolution=41, rule="odd"))[1] == 2          # parity keeps the inner shell as a cavity
    w = voxel.WindingGrid(mesh, resolution=41)
    assert w.dtype == torch.int32 and tuple(w.shape) == (41, 41, 41) and int(w.max()) == 2 and int(w.min()) == 0
    with pytest.raises(api[0].NrfError, match="1 faces"):
        far = M.Mesh(torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1e9, 0, 0]], device="cuda"), torch.tensor([[0, 1, 2], [0, 1, 3]], dtype=torch.int32, device="cuda"),
                     torch.zeros((4, 3), device="cuda"))
        voxel.MeshToSDF(far, bbox=[-1, -1, -1, 2, 2, 2], resolution=9)


def test_extract_mesh_union_resolution(api):
    """ExtractMesh(union_resolution=) is RemeshUnion of the bare isosurface, placed before the colours; None leaves the mesh as it was"""
    from nerfpp_amd import scene
    _, voxel, M, _ = api
    r = scene.make_hash_scene(mode="ngp", log2_t=14, seed=5000)["renderer"]
    iso = float(torch.quantile(M.DensityGrid(r, None, 24).reshape(-1), 0.7))
    plain = M.ExtractMesh(r, iso, resolution=24)
    again = M.ExtractMesh(r, iso, resolution=24, union_resolution=None)
    assert torch.equal(plain.Vertices, again.Vertices) and torch.equal(plain.Faces, again.Faces) and torch.equal(plain.Colors, again.Colors)
    union = M.ExtractMesh(r, iso, resolution=24, union_resolution=40)
    want = voxel.RemeshUnion(M.Mesh(plain.Vertices, plain.Faces, plain.Normals), resolution=40)
    assert want.Faces.shape[0] > 0 and torch.equal(union.Vertices, want.Vertices) and torch.equal(union.Faces, want.Faces) and torch.equal(union.Normals, want.Normals)
    assert union.Colors.shape == union.Vertices.shape and bool(torch.isfinite(union.Colors).all())
