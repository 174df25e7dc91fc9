"""Connected components on the MI355X: nrf_mesh_components and nrf_lattice_components against the numpy restatement (tests/components_ref.py), integer for integer
and twice over (the labels are canonical: two runs give the same array), bad input, and the Python layers built on them: FilterComponents, ExtractMesh's filter,
LatticeComponents and LocateObject."""
import ctypes as C

import numpy as np
import pytest
import torch

import components_ref as R
import lerf_query_ref as Q
import mesh_ref as M

pytestmark = pytest.mark.gpu

INVALID_ARG = 1


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from nerfpp_amd import _lib as L, mesh, query, scene
    return L, mesh, query, scene


@pytest.fixture(scope="module")
def mesh_cases():
    return R.mesh_cases()


def _twice(fn, *args):
    a, ka = fn(*args)
    b, kb = fn(*args)
    assert ka == kb and torch.equal(a, b), "two runs give the same labels"
    return a.cpu().numpy(), ka


# ------------------------------------------------------------------------------------ 1. meshes
@pytest.mark.parametrize("name", ["strip", "tetrahedra", "joined_last", "two_strips", "degenerate"])
def test_mesh_components_equal_the_restatement(api, mesh_cases, name):
    mesh = api[1]
    faces, v, k = mesh_cases[name]
    want, kw = R.mesh_components(faces, v)
    assert kw == k
    got, kg = _twice(mesh.MeshComponents, torch.from_numpy(faces).cuda(), v)
    assert got.dtype == np.int32 and got.shape == (v,)
    assert kg == k and np.array_equal(got, want)
    if name == "tetrahedra":
        assert (got == -1).sum() == 37


def test_mesh_components_more_than_one_scan_round(api):
    """The per-block root counts are scanned 8 192 blocks of 256 at a time: 2 097 153 vertices need a second round and end one past a block boundary.  A few dozen
    faces; components whose smallest vertex lies in block 0, in block 8 191 and -- the (a, a, a) face on the last vertex -- at index 2 097 152, whose rank is K - 1
    and comes through the carry of the first round."""
    mesh = api[1]
    v = 8192 * 256 + 1
    rng = np.random.default_rng(12)
    faces = np.concatenate([rng.integers(0, v, (40, 3)),
                            [[3, 1000000, v - 2], [200, 7, 90], [8191 * 256 + 4, 8191 * 256 + 100, v - 3], [v - 4, 8191 * 256, 8191 * 256 + 200],
                             [v - 1, v - 1, v - 1], [90, 200, 1000001]]]).astype(np.int32)
    faces = faces[rng.permutation(len(faces))]
    want, kw = R.mesh_components(faces, v)
    assert kw > 40 and want[v - 1] == kw - 1 and want[3] == 0 and want[8191 * 256] == want[v - 4] == kw - 3 and want[v - 3] == kw - 2 and (want == -1).sum() > v - 140
    got, kg = _twice(mesh.MeshComponents, torch.from_numpy(faces).cuda(), v)
    assert kg == kw and np.array_equal(got, want)


def test_mesh_components_empty_inputs(api):
    mesh = api[1]
    none = torch.empty((0, 3), dtype=torch.int32, device="cuda")
    labels, k = mesh.MeshComponents(none, 0)
    assert k == 0 and labels.shape == (0,)
    labels, k = mesh.MeshComponents(none, 5)
    assert k == 0 and labels.cpu().tolist() == [-1] * 5


def test_mesh_components_refuse_an_index_out_of_range(api):
    """Only the value V, with V no multiple of 64: even an implementation that followed it would stay inside the padded buffers handed in here."""
    L, mesh = api[0], api[1]
    lib = L.lib()
    v = 1000
    faces = R.scramble(R.strip(v), v, 9)
    faces[len(faces) // 2, 1] = v
    d_faces = torch.from_numpy(faces).cuda()
    labels = torch.full((1024,), -7, dtype=torch.int32, device="cuda")
    ws = torch.zeros((int(lib.nrf_mesh_components_workspace_bytes(v, len(faces))) + 4096,), dtype=torch.uint8, device="cuda")
    k = C.c_int64(-1)
    rc = lib.nrf_mesh_components(d_faces.data_ptr(), v, len(faces), labels.data_ptr(), C.byref(k), ws.data_ptr(), ws.numel(), None)
    assert rc == INVALID_ARG and b"outside [0, 1000)" in lib.nrf_last_error()
    assert (labels[v:] == -7).all(), "nothing written past the V labels"
    with pytest.raises(L.NrfError, match="outside"):
        mesh.MeshComponents(d_faces, v)
    # the same list without the bad face is fine afterwards
    good = np.delete(faces, len(faces) // 2, axis=0)
    got, kg = mesh.MeshComponents(torch.from_numpy(good).cuda(), v)
    want, kw = R.mesh_components(good, v)
    assert kg == kw and np.array_equal(got.cpu().numpy(), want)


def test_known_mesh_answer(api):
    """Two balls and a torus: K = 3 on the extracted surface and on the lattice under the isosurface's own connectivity; the largest component is the closed torus."""
    _, mesh, query, _ = api
    f, box = R.known_field()
    d = torch.from_numpy(f).cuda()
    verts, faces, normals = mesh.Isosurface(d, box, 0.0)
    assert (verts.shape[0], faces.shape[0]) == (3238, 6468)
    labels, k = _twice(mesh.MeshComponents, faces, verts.shape[0])
    fc = faces.cpu().numpy()
    want, kw = R.mesh_components(fc, verts.shape[0])
    assert k == kw == 3 and np.array_equal(labels, want)
    assert np.bincount(labels[fc[:, 0]]).tolist() == [1536, 600, 4332]
    lat, kl = _twice(query.LatticeComponents, d > 0, 14)
    assert kl == 3 and np.array_equal(lat, R.lattice_components(f > 0, 14)[0])
    full = mesh.Mesh(verts, faces, normals)
    torus = mesh.FilterComponents(full, keep_largest=1)
    assert torus.Faces.shape[0] == 4332 and M.edge_check(torus.Faces.cpu().numpy()) == (True, True)
    assert M.euler(torus.Vertices.cpu().numpy(), torus.Faces.cpu().numpy()) == 0
    old = torch.nonzero(torch.from_numpy(labels == 2).cuda()).reshape(-1)
    assert torch.equal(torus.Vertices, verts[old]) and torch.equal(torus.Normals, normals[old])
    assert torch.equal(old[torus.Faces.to(torch.int64)], faces[torch.from_numpy(labels[fc[:, 0]] == 2).cuda()].to(torch.int64))
    # the device path and the labels= path are one function
    host = mesh.FilterComponents(mesh.Mesh(verts.cpu(), faces.cpu(), normals.cpu()), keep_largest=2, min_faces=1000, labels=want)
    dev = mesh.FilterComponents(full, keep_largest=2, min_faces=1000)
    assert host.Faces.shape[0] == 4332 + 1536 and torch.equal(dev.Faces.cpu(), host.Faces) and torch.equal(dev.Vertices.cpu(), host.Vertices)


# ------------------------------------------------------------------------------------ 2. lattices
@pytest.mark.parametrize("connectivity", [6, 14, 26])
def test_lattice_components_equal_the_restatement(api, connectivity):
    query = api[2]
    for name, m in R.lattice_masks().items():            # each percolation mask also under the other two connectivities
        want, kw = R.lattice_components(m, connectivity)
        got, kg = _twice(query.LatticeComponents, torch.from_numpy(m).cuda(), connectivity)
        assert got.dtype == np.int32 and got.shape == m.shape
        assert kg == kw and np.array_equal(got, want), name
        if name == "serpentine":
            assert kg == 1
        if name == "wrap":
            assert kg == m.sum(), "neighbours in memory are no neighbours on the lattice"
        if name == "ones":
            assert kg == 1 and (got == 0).all()
        if name == "zeros":
            assert kg == 0 and (got == -1).all()


def test_lattice_components_accept_any_mask_dtype_and_refuse_other_connectivities(api):
    L, _, query, _ = api
    m = R.percolation_mask(14)[:7, :9, :11]
    want, kw = R.lattice_components(m, 14)
    for t in (torch.from_numpy(m), torch.from_numpy(m.astype(np.float32) * 0.25).cuda(), torch.from_numpy(m.astype(np.uint8) * 255).cuda()):
        got, k = query.LatticeComponents(t, 14)
        assert k == kw and np.array_equal(got.cpu().numpy(), want)
    lib = L.lib()
    d = torch.from_numpy(m.astype(np.uint8)).cuda()
    labels = torch.empty(m.shape, dtype=torch.int32, device="cuda")
    ws = torch.empty((int(lib.nrf_lattice_components_workspace_bytes(11, 9, 7)),), dtype=torch.uint8, device="cuda")
    k = C.c_int64(-1)
    for bad in (8, 0, 18, -6):
        assert lib.nrf_lattice_components(d.data_ptr(), 11, 9, 7, bad, labels.data_ptr(), C.byref(k), ws.data_ptr(), ws.numel(), None) == INVALID_ARG
    assert b"connectivity" in lib.nrf_last_error()
    assert lib.nrf_lattice_components(d.data_ptr(), 11, 9, 7, 14, labels.data_ptr(), C.byref(k), ws.data_ptr(), ws.numel() - 256, None) == 4          # workspace too small
    with pytest.raises(L.NrfError):
        query.LatticeComponents(d, 8)


# ------------------------------------------------------------------------------------ 3. ExtractMesh
def _same_mesh(a, b):
    for name in ("Vertices", "Faces", "Normals", "Colors"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None) and (x is None or (x.shape == y.shape and torch.equal(x, y))), name


def test_extract_mesh_filters_before_colouring(api):
    _, mesh, _, scene = api
    sc = scene.make_hash_scene()
    r = sc["renderer"]
    sigma = mesh.DensityGrid(r, None, 33)
    thr = float(sigma.reshape(-1).quantile(0.7).item())
    plain = mesh.ExtractMesh(r, thr, resolution=33)
    verts, faces, normals = mesh.Isosurface(sigma, sc["bbox"], thr)
    assert torch.equal(plain.Vertices, verts) and torch.equal(plain.Faces, faces) and torch.equal(plain.Normals, normals), "the defaults change nothing"
    labels, k = mesh.MeshComponents(plain)
    assert k >= 2, "the scene's isosurface has floaters"
    _same_mesh(mesh.ExtractMesh(r, thr, resolution=33, keep_largest=1), mesh.FilterComponents(plain, keep_largest=1))
    _same_mesh(mesh.ExtractMesh(r, thr, resolution=33, min_component_faces=50, colors=False),
               mesh.FilterComponents(mesh.Mesh(verts, faces, normals), min_faces=50))
    sizes = np.bincount(labels.cpu().numpy()[faces.cpu().numpy()[:, 0]], minlength=k)
    assert mesh.FilterComponents(plain, keep_largest=1).Faces.shape[0] == sizes.max()
    assert mesh.FilterComponents(plain, min_faces=50, labels=labels).Faces.shape[0] == sizes[sizes >= 50].sum()


# ------------------------------------------------------------------------------------ 4. LocateObject
def test_locate_object_is_relevancy_grid_plus_components(api):
    _, _, query, scene = api
    sc = scene.make_lerf_scene(log2_t=14)
    r = sc["renderer"]
    r.SetLeRFPrompts(Q.unit_prompts(1, 21), Q.unit_prompts(4, 22))
    res = 24
    rel, sig = query.RelevancyGrid(r, resolution=res)
    rel_h, sig_h = rel.cpu().numpy(), sig.cpu().numpy()
    st, rt = float(np.float32(np.quantile(sig_h, 0.5))), float(np.float32(np.quantile(rel_h[..., 0], 0.4)))            # fp32 values: one meaning on either side
    mask = (sig_h >= np.float32(st)) & (rel_h[..., 0] >= np.float32(rt))
    assert 0.05 < mask.mean() < 0.95, "neither empty nor full"
    cand = np.nonzero(mask.reshape(-1))[0]
    seed = int(cand[np.argmax(rel_h.reshape(-1, 2)[cand, 0])])            # argmax: the first of equal maxima, i.e. the lowest flat index
    pts = M.lattice_points(sc["bbox"], res, res, res)
    for c in (14, 6):
        labels, _ = R.lattice_components(mask, c)
        comp = labels == labels.reshape(-1)[seed]
        z, y, x = np.nonzero(comp)
        got = query.LocateObject(r, resolution=res, sigma_threshold=st, relevancy_threshold=rt, connectivity=c)
        assert got["mask"].dtype == torch.bool and np.array_equal(got["mask"].cpu().numpy(), comp)
        assert got["count"] == comp.sum() and got["seed_index"] == seed
        assert np.array_equal(got["seed_position"].cpu().numpy(), pts.reshape(-1, 3)[seed])
        assert np.array_equal(got["relevancy"].cpu().numpy(), rel_h.reshape(-1, 2)[seed])
        assert np.array_equal(got["bbox"].cpu().numpy(), np.concatenate([pts[z.min(), y.min(), x.min()], pts[z.max(), y.max(), x.max()]]))
    none = query.LocateObject(r, resolution=res, sigma_threshold=float("inf"))
    assert none["count"] == 0 and none["bbox"] is None and none["mask"].shape == (res, res, res) and not bool(none["mask"].any())
