"""Mesh adjacency, smoothing and vertex normals on the MI355X: nrf_mesh_adjacency_count / _emit, nrf_mesh_smooth and nrf_mesh_vertex_normals against the numpy
restatement (tests/smooth_ref.py), every output bit for bit -- closed spheres, the open hemisphere with its unused vertices, fans on both sides of the row-length
threshold and a hub of 4 096 faces, a dirty mesh (bad indices, repeated corners, a duplicated face, a non-manifold edge, a NaN vertex), poisoned workspaces and
outputs, permuted faces, empty meshes, the refusal of totals that are not the count call's -- and the Python layer: BuildAdjacency, MeshTopology, VertexNormals,
SmoothMesh, SmoothAttributes and ExtractMesh(smooth_iterations=)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import smooth_ref as S

pytestmark = pytest.mark.gpu

F32 = np.float32
INVALID_ARG = 1
MODES = (S.SMOOTH_FREE, S.SMOOTH_FIXED, S.SMOOTH_CURVE)
ADJ_KEYS = ("face_start", "face_list", "nbr_start", "nbr", "nbr_faces", "flags", "stats")


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from nerfpp_amd import _lib as L, mesh
    return L, mesh


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def p(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def poisoned(shape, dtype):
    """A device tensor whose every byte is 0xFF"""
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(0xFF)
    return t


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same_floats(got, want, what, nan_input=False):
    """Bit for bit; where the input held a NaN, a NaN for a NaN (its payload is unspecified) and the bits everywhere else"""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    assert got.shape == want.shape, what
    if nan_input:
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaNs at {np.nonzero(np.isnan(got) != np.isnan(want))[0][:8]}"
        ok = ~np.isnan(want)
        assert np.array_equal(bits(got)[ok], bits(want)[ok]), what
    else:
        diff = bits(got) != bits(want)
        assert not diff.any(), f"{what}: differs at {np.argwhere(diff)[:8].tolist()}"


def adjacency(api, faces, n_verts, pattern=0xFF, totals=None):
    """The two C entries -> (the dict smooth_ref.adjacency returns, the same arrays as device tensors); the workspace and every output start as `pattern` bytes"""
    lib = api[0].lib()
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    nf, nv = len(faces), int(n_verts)
    df = dev(faces, np.int32)
    ws = torch.full((max(1, int(lib.nrf_mesh_adjacency_workspace_bytes(nv, nf))),), pattern, dtype=torch.uint8, device="cuda")
    ni, nn = C.c_int64(-7), C.c_int64(-7)
    assert lib.nrf_mesh_adjacency_count(p(df), nv, nf, C.addressof(ni), C.addressof(nn), ws.data_ptr(), ws.numel(), None) == 0, lib.nrf_last_error()
    ni, nn = int(ni.value), int(nn.value)
    if totals is not None:
        return ni, nn, ws, df
    d = dict(face_start=poisoned((nv + 1,), torch.int64), face_list=poisoned((ni,), torch.int32), nbr_start=poisoned((nv + 1,), torch.int64),
             nbr=poisoned((nn,), torch.int32), nbr_faces=poisoned((nn,), torch.int32), flags=poisoned((nv,), torch.uint8), stats=poisoned((8,), torch.int64))
    assert lib.nrf_mesh_adjacency_emit(p(df), nv, nf, ni, nn, d["face_start"].data_ptr(), p(d["face_list"]), d["nbr_start"].data_ptr(), p(d["nbr"]), p(d["nbr_faces"]),
                                       p(d["flags"]), d["stats"].data_ptr(), ws.data_ptr(), ws.numel(), None) == 0, lib.nrf_last_error()
    torch.cuda.synchronize()
    host = {k: t.cpu().numpy() for k, t in d.items()}
    host["n_verts"] = nv
    d["n_verts"], d["faces"], d["n_faces"] = nv, df, nf
    return host, d


def assert_adjacency(got, want, what, keys=ADJ_KEYS):
    for k in keys:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), f"{what}: {k} differs at {np.nonzero(got[k] != want[k])[0][:8] if got[k].shape == want[k].shape else (got[k].shape, want[k].shape)}"


def smooth(api, x, d, iterations, lam, mu, mode):
    lib = api[0].lib()
    x = np.asarray(x, F32)
    c = 1 if x.ndim == 1 else x.shape[1]
    dx, out, tmp = dev(x, F32), poisoned(x.shape, torch.float32), poisoned(x.shape, torch.float32)
    assert lib.nrf_mesh_smooth(p(dx), p(out), p(tmp), d["n_verts"], c, iterations, lam, mu, mode, d["nbr_start"].data_ptr(), p(d["nbr"]), p(d["nbr_faces"]),
                               p(d["flags"]), d["nbr"].numel(), None) == 0, lib.nrf_last_error()
    torch.cuda.synchronize()
    assert torch.equal(dx.cpu(), torch.from_numpy(x)) or np.isnan(x).any(), "the input is not written"
    return out.cpu().numpy()


def normals(api, verts, d, weighting):
    lib = api[0].lib()
    dv, out = dev(verts, F32), poisoned((d["n_verts"], 3), torch.float32)
    assert lib.nrf_mesh_vertex_normals(p(dv), d["n_verts"], p(d["faces"]), d["n_faces"], d["face_start"].data_ptr(), p(d["face_list"]), d["face_list"].numel(), weighting,
                                       p(out), None) == 0, lib.nrf_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def channels(verts, c, seed=5):
    """[V, c] values to smooth: the positions themselves for c == 3"""
    return verts if c == 3 else np.random.default_rng(seed + c).standard_normal((len(verts), c)).astype(F32)


@functools.lru_cache(maxsize=None)
def reference(kind, level):
    verts, faces = (S.sphere if kind == "sphere" else S.hemisphere)(level)
    return verts, faces, S.adjacency(faces, len(verts))


@pytest.mark.parametrize("level", [2, 3])
def test_closed_spheres_equal_the_restatement(api, level):
    verts, faces, want = reference("sphere", level)
    got, d = adjacency(api, faces, len(verts))
    assert_adjacency(got, want, f"sphere {level}")
    assert got["stats"].tolist()[2:] == [len(verts), 3 * len(faces) // 2, 0, 0, 6, 6]
    for c in (1, 2, 3, 4):
        x = channels(verts, c)
        x = x[:, 0] if c == 1 and level == 2 else x          # a flat [V] array is C == 1 as well
        for iterations in (0, 1, 5):
            for mu in (0.0, -0.53):
                for mode in MODES:
                    same_floats(smooth(api, x, d, iterations, 0.5, mu, mode), S.smooth(x, want, iterations, 0.5, mu, mode), f"sphere {level}, C {c}, {iterations} x mu {mu}, mode {mode}")
    for weighting in (S.NORMALS_AREA, S.NORMALS_UNIT):
        same_floats(normals(api, verts, d, weighting), S.vertex_normals(verts, faces, want, weighting), f"sphere {level} normals {weighting}")


def test_the_hemisphere_keeps_its_unused_vertices(api):
    verts, faces, want = reference("hemisphere", 3)
    got, d = adjacency(api, faces, len(verts))
    assert_adjacency(got, want, "hemisphere")
    unused = np.diff(want["face_start"]) == 0
    rim = (want["flags"] & S.ADJ_BOUNDARY) != 0
    assert unused.sum() == len(verts) - 145 and rim.sum() == 32 and (got["flags"][unused] == 0).all()
    for mode in MODES:
        for c in (3, 4):
            x = channels(verts, c)
            y = smooth(api, x, d, 4, 0.5, -0.53, mode)
            same_floats(y, S.smooth(x, want, 4, 0.5, -0.53, mode), f"hemisphere, mode {mode}, C {c}")
            assert np.array_equal(bits(y[unused]), bits(x[unused]))
            if mode == S.SMOOTH_FIXED:
                assert np.array_equal(bits(y[rim]), bits(x[rim]))
            if mode == S.SMOOTH_CURVE and c == 3:
                assert np.array_equal(bits(y[rim, 2]), bits(x[rim, 2])) and (y[rim, :2] != x[rim, :2]).any()
    for weighting in (S.NORMALS_AREA, S.NORMALS_UNIT):
        n = normals(api, verts, d, weighting)
        same_floats(n, S.vertex_normals(verts, faces, want, weighting), f"hemisphere normals {weighting}")
        assert (n[unused] == 0).all()


@pytest.mark.parametrize("n", [S.ADJ_SHORT_ROW - 1, S.ADJ_SHORT_ROW, S.ADJ_SHORT_ROW + 1, 300, 4096])
def test_fans_on_both_sides_of_the_row_threshold_and_a_hub(api, n):
    """Vertex 0 has n faces and n + 1 neighbours: the one-lane path up to ADJ_SHORT_ROW faces, the workgroup path beyond (more than one round of its 256 lanes from
    257 half-edge ends on); shuffled faces, so the cursor order is not the sorted one"""
    verts, faces = S.fan(n)
    faces = S.permuted(faces, n)
    want = S.adjacency(faces, len(verts))
    assert want["stats"].tolist() == [0, 0, n + 2, 2 * n + 1, n + 2, 0, n, n + 1]
    got, d = adjacency(api, faces, len(verts))
    assert_adjacency(got, want, f"fan {n}")
    for mode in MODES:
        same_floats(smooth(api, verts, d, 1, 0.5, 0.0, mode), S.smooth(verts, want, 1, 0.5, 0.0, mode), f"fan {n}, mode {mode}")
    for weighting in (S.NORMALS_AREA, S.NORMALS_UNIT):
        same_floats(normals(api, verts, d, weighting), S.vertex_normals(verts, faces, want, weighting), f"fan {n} normals {weighting}")


def test_more_than_one_scan_round_of_vertices(api):
    """The block totals of the degrees are scanned 8 192 blocks of 256 at a time: 2 097 153 vertices need a second round and end one past a block boundary.  A handful
    of faces on the first vertex, the last one (index 2 097 152, alone in its block) and the last of block 8 191 beside it; both row-start arrays and all rows"""
    nv = 8192 * 256 + 1
    faces = np.array([[0, 1, 2], [2, 1, 255], [0, nv - 2, nv - 1], [nv - 1, nv - 2, nv - 3], [256, nv - 1, 8191 * 256], [1000000, 1000001, nv - 2], [nv - 1, 0, 1000000],
                      [5, 5, 6], [nv, 0, 1]], np.int32)
    want = S.adjacency(faces, nv)
    assert want["stats"].tolist()[:3] == [1, 1, 11] and want["face_start"][nv - 1] == 3 * 7 - 4 and want["face_start"][nv] == 3 * 7 and want["nbr_start"][nv] == len(want["nbr"])
    assert np.diff(want["nbr_start"])[[0, nv - 2, nv - 1]].tolist() == [5, 5, 6]
    got, _ = adjacency(api, faces, nv)
    assert_adjacency(got, want, "two scan rounds")


def test_the_dirty_mesh(api):
    verts, faces = S.dirty()
    want = S.adjacency(faces, len(verts))
    got, d = adjacency(api, faces, len(verts))
    assert_adjacency(got, want, "dirty")
    assert got["stats"].tolist() == [3, 3, 9, 15, 8, 2, 5, 6] and got["flags"].tolist() == [3, 3, 1, 1, 1, 3, 3, 0, 1, 0]
    for mode in MODES:
        for iterations, mu in ((1, 0.0), (2, -0.53)):
            y = smooth(api, verts, d, iterations, 0.5, mu, mode)
            same_floats(y, S.smooth(verts, want, iterations, 0.5, mu, mode), f"dirty, mode {mode}, {iterations} iterations", nan_input=True)
    y = smooth(api, verts, d, 1, 0.5, 0.0, S.SMOOTH_FREE)
    assert np.isnan(y).any(axis=1).tolist() == [False, True, True, False, False, True, True, True, True, False], "the NaN reaches the neighbours of vertex 5 only"
    for weighting in (S.NORMALS_AREA, S.NORMALS_UNIT):
        same_floats(normals(api, verts, d, weighting), S.vertex_normals(verts, faces, want, weighting), f"dirty normals {weighting}", nan_input=True)
    clean = np.nan_to_num(verts, nan=0.5)
    for weighting in (S.NORMALS_AREA, S.NORMALS_UNIT):
        same_floats(normals(api, clean, d, weighting), S.vertex_normals(clean, faces, want, weighting), f"dirty normals {weighting}, finite")


def test_poisoned_workspaces_and_permuted_faces(api):
    verts, faces, want = reference("sphere", 3)
    runs = [adjacency(api, faces, len(verts), pattern) for pattern in (0xFF, 0xFF, 0x00, 0x5A)]
    for got, _ in runs:
        assert_adjacency(got, want, "repeated run")
    x = channels(verts, 3)
    first = smooth(api, x, runs[0][1], 3, 0.5, -0.53, S.SMOOTH_CURVE)
    for _, d in runs[1:]:
        assert np.array_equal(bits(smooth(api, x, d, 3, 0.5, -0.53, S.SMOOTH_CURVE)), bits(first))
    for kind in ("sphere", "hemisphere"):
        verts, faces, want = reference(kind, 3)
        for seed in (1, 2):
            other = S.permuted(faces, seed)
            got, d = adjacency(api, other, len(verts))
            assert_adjacency(got, want, f"permuted {kind}", keys=("face_start", "nbr_start", "nbr", "nbr_faces", "flags", "stats"))
            assert np.array_equal(got["face_list"], S.adjacency(other, len(verts))["face_list"])
            for mode in MODES:
                same_floats(smooth(api, verts, d, 3, 0.5, -0.53, mode), S.smooth(verts, want, 3, 0.5, -0.53, mode), f"permuted {kind}, mode {mode}")


def test_empty_meshes(api):
    none = np.zeros((0, 3), np.int32)
    for what, faces, nv in (("no vertex, no face", none, 0), ("no face", none, 5), ("no vertex", [[0, 1, 2]], 0), ("only invalid faces", [[0, 0, 1], [0, 1, 7], [-1, 2, 3]], 5)):
        want = S.adjacency(faces, nv)
        got, d = adjacency(api, faces, nv)
        assert_adjacency(got, want, what)
        assert got["face_list"].size == 0 == got["nbr"].size and (got["flags"] == 0).all() and got["stats"].tolist()[2:] == [0] * 6
        x = np.arange(nv * 3, dtype=F32).reshape(nv, 3)
        if nv:
            assert np.array_equal(bits(smooth(api, x, d, 2, 0.5, -0.53, S.SMOOTH_CURVE)), bits(x))
            assert (normals(api, x, d, S.NORMALS_AREA) == 0).all()
        else:
            lib = api[0].lib()
            assert lib.nrf_mesh_smooth(None, None, None, 0, 3, 2, 0.5, -0.53, S.SMOOTH_CURVE, d["nbr_start"].data_ptr(), None, None, None, 0, None) == 0
            assert lib.nrf_mesh_vertex_normals(None, 0, p(d["faces"]), d["n_faces"], d["face_start"].data_ptr(), None, 0, S.NORMALS_AREA, None, None) == 0


def test_emit_refuses_totals_that_are_not_the_count_calls(api):
    lib = api[0].lib()
    verts, faces, want = reference("sphere", 2)
    nv, nf = len(verts), len(faces)
    ni, nn, ws, df = adjacency(api, faces, nv, totals=True)
    assert (ni, nn) == (3 * nf, 3 * nf)
    out = dict(fs=poisoned((nv + 1,), torch.int64), fl=poisoned((ni + 8,), torch.int32), ns=poisoned((nv + 1,), torch.int64), nb=poisoned((nn + 8,), torch.int32),
               nbf=poisoned((nn + 8,), torch.int32), flags=poisoned((nv,), torch.uint8), stats=poisoned((8,), torch.int64))

    def emit(ni_, nn_):
        return lib.nrf_mesh_adjacency_emit(df.data_ptr(), nv, nf, ni_, nn_, out["fs"].data_ptr(), out["fl"].data_ptr(), out["ns"].data_ptr(), out["nb"].data_ptr(),
                                           out["nbf"].data_ptr(), out["flags"].data_ptr(), out["stats"].data_ptr(), ws.data_ptr(), ws.numel(), None)
    for bad in ((ni - 3, nn), (ni, nn - 2), (ni + 3, nn), (ni, nn + 2), (0, 0)):          # (ni + 3, nn) cannot come from these faces; the others are not this mesh's
        assert emit(*bad) == INVALID_ARG and lib.nrf_last_error().startswith(b"nrf_mesh_adjacency_emit"), bad
    torch.cuda.synchronize()
    for k, t in out.items():
        assert (t.view(torch.uint8) == 0xFF).all(), f"a refused call wrote {k}"
    assert emit(ni, nn) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out["nb"][:nn].cpu().numpy(), want["nbr"]) and (out["nb"][nn:].view(torch.uint8) == 0xFF).all()


# ---- the Python layer ----

def sphere_mesh(mesh, level=3, colours=True):
    verts, faces, _ = reference("sphere", level)
    v = dev(verts, F32)
    rng = np.random.default_rng(9)
    return mesh.Mesh(v, dev(faces, np.int32), torch.zeros_like(v), dev(rng.uniform(0, 1, verts.shape), F32) if colours else None,
                     dev(rng.standard_normal((len(verts), 2)), F32) if colours else None)


def test_smooth_mesh_smooth_attributes_and_topology(api):
    L, mesh = api
    verts, faces, want = reference("sphere", 3)
    m = sphere_mesh(mesh)
    adj = mesh.BuildAdjacency(m)
    assert isinstance(adj, mesh.MeshAdjacency) and (adj.NumVerts, adj.NumFaces) == (len(verts), len(faces))
    for k, t in (("face_start", adj.FaceStart), ("face_list", adj.FaceList), ("nbr_start", adj.NbrStart), ("nbr", adj.Nbr), ("nbr_faces", adj.NbrFaces),
                 ("flags", adj.Flags), ("stats", adj.Stats)):
        assert np.array_equal(t.cpu().numpy(), want[k]) and t.cpu().numpy().dtype == want[k].dtype, k
    assert mesh.MeshTopology(m) == mesh.MeshTopology(adj) == S.topology(want) and adj.stats == dict(zip(S.STATS, want["stats"].tolist()))
    hv, hf, hwant = reference("hemisphere", 3)
    assert mesh.MeshTopology(dev(hf, np.int32)) == S.topology(S.adjacency(hf, int(hf.max()) + 1)), "faces alone: the largest index + 1 vertices"
    assert mesh.MeshTopology(mesh.BuildAdjacency(hf, n_verts=len(hv))) == S.topology(hwant)

    out = mesh.SmoothMesh(m)
    assert out.Faces is m.Faces or torch.equal(out.Faces, m.Faces)
    same_floats(out.Vertices.cpu().numpy(), S.smooth(verts, want, 10, 0.5, -0.53, S.SMOOTH_CURVE), "SmoothMesh defaults")
    assert torch.equal(out.Normals, mesh.VertexNormals(out)) and torch.equal(out.Normals, mesh.VertexNormals(out, adjacency=adj))
    same_floats(out.Normals.cpu().numpy(), S.vertex_normals(out.Vertices.cpu().numpy(), faces, want), "recomputed normals")
    assert torch.equal(out.Colors, m.Colors) and torch.equal(out.Relevancy, m.Relevancy), "attributes that were not named are carried"
    both = mesh.SmoothMesh(m, iterations=3, lam=0.4, mu=0.0, boundary="free", attributes=("Colors", "Relevancy"), recompute_normals=False, adjacency=adj)
    same_floats(both.Vertices.cpu().numpy(), S.smooth(verts, want, 3, 0.4, 0.0, S.SMOOTH_FREE), "SmoothMesh, Laplacian")
    same_floats(both.Colors.cpu().numpy(), S.smooth(m.Colors.cpu().numpy(), want, 3, 0.4, 0.0, S.SMOOTH_FREE), "Colors")
    same_floats(both.Relevancy.cpu().numpy(), S.smooth(m.Relevancy.cpu().numpy(), want, 3, 0.4, 0.0, S.SMOOTH_FREE), "Relevancy")
    assert torch.equal(both.Normals, m.Normals)
    same_floats(mesh.VertexNormals(m, "unit").cpu().numpy(), S.vertex_normals(verts, faces, want, S.NORMALS_UNIT), "VertexNormals unit")

    att = mesh.SmoothAttributes(m, ["Relevancy"], 4)
    assert torch.equal(att.Vertices, m.Vertices) and torch.equal(att.Normals, m.Normals) and torch.equal(att.Colors, m.Colors) and torch.equal(att.Faces, m.Faces)
    same_floats(att.Relevancy.cpu().numpy(), S.smooth(m.Relevancy.cpu().numpy(), want, 4, 0.5, 0.0, S.SMOOTH_FREE), "SmoothAttributes")
    flat = mesh.Mesh(m.Vertices, m.Faces, m.Normals, None, m.Relevancy[:, 0].contiguous())
    same_floats(mesh.SmoothAttributes(flat, "Relevancy", 2).Relevancy.cpu().numpy(), S.smooth(m.Relevancy[:, 0].cpu().numpy(), want, 2, 0.5, 0.0, S.SMOOTH_FREE), "[V] relevancy")

    bare = sphere_mesh(mesh, colours=False)
    for call in (lambda: mesh.SmoothMesh(m, boundary="pinned"), lambda: mesh.SmoothMesh(m, iterations=-1), lambda: mesh.SmoothMesh(m, lam=float("nan")),
                 lambda: mesh.SmoothMesh(m, mu=float("inf")), lambda: mesh.SmoothMesh(bare, attributes=("Colors",)), lambda: mesh.SmoothMesh(m, attributes=("Normals",)),
                 lambda: mesh.SmoothAttributes(bare, ["Relevancy"], 1), lambda: mesh.VertexNormals(m, "angle"),
                 lambda: mesh.SmoothMesh(m, adjacency=mesh.BuildAdjacency(dev(hf, np.int32), n_verts=len(hv)))):
        with pytest.raises(L.NrfError):
            call()


def test_extract_mesh_smooths_before_the_colours(api):
    _, mesh = api
    from nerfpp_amd import scene
    sc = scene.make_hash_scene(mode="ngp")
    g = mesh.DensityGrid(sc["renderer"], None, 33)
    iso = float(torch.quantile(g.reshape(-1), 0.7))
    plain = mesh.ExtractMesh(sc["renderer"], iso, resolution=33)
    zero = mesh.ExtractMesh(sc["renderer"], iso, resolution=33, smooth_iterations=0)
    assert plain.Faces.shape[0] > 1000
    for name in ("Vertices", "Faces", "Normals", "Colors"):
        assert torch.equal(getattr(plain, name), getattr(zero, name)), name
    bare = mesh.ExtractMesh(sc["renderer"], iso, resolution=33, colors=False)
    want = mesh.SmoothMesh(bare, iterations=2)
    for normals_from in ("lattice", "field"):
        got = mesh.ExtractMesh(sc["renderer"], iso, resolution=33, colors=False, smooth_iterations=2, normals=normals_from)
        assert torch.equal(got.Vertices, want.Vertices) and torch.equal(got.Faces, bare.Faces) and not torch.equal(got.Vertices, bare.Vertices)
        assert torch.equal(got.Normals, want.Normals) and torch.equal(got.Normals, mesh.VertexNormals(got)) and got.Colors is None
    coloured = mesh.ExtractMesh(sc["renderer"], iso, resolution=33, smooth_iterations=2)
    assert torch.equal(coloured.Vertices, want.Vertices) and coloured.Colors.shape == want.Vertices.shape and torch.isfinite(coloured.Colors).all()
