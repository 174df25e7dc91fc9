"""Mesh simplification on the MI355X: nrf_mesh_simplify_count / _emit against the numpy restatement (tests/simplify_ref.py), every output bit for bit -- both
totals, the stats, vertices, faces, rep, face_src and cluster -- on random soups and subdivided spheres at every size and grid at which a kernel takes another path,
vertices on cell faces and outside the box, coincident faces that meet in one slot, bad indices, non-finite and unused vertices, NULL outputs, dirty workspaces and
repeated runs; the refusals over live buffers; and the Python layer: SimplifyMesh, SimplifyToFaces, ExtractMesh(simplify_cell=...) and the distance to the input."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import raster_ref as R
import simplify_ref as S
import tsdf_ref as T

pytestmark = pytest.mark.gpu

F32 = np.float32
INVALID_ARG, WORKSPACE = 1, 4
UNIT_BOX = (-1, -1, -1, 1, 1, 1)
PATTERNS = (0x00, 0x5A, 0xA5, 0xFF)
OUTPUTS = ("rep", "face_src", "cluster", "stats")


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from nerfpp_amd import _lib as L, geometry, mesh
    return L, geometry, mesh


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def p(t):
    return None if t is None else t.data_ptr()


def workspace(nbytes, pattern):
    ws = torch.empty((max(1, int(nbytes)),), dtype=torch.uint8, device="cuda")
    if pattern is not None:
        ws.fill_(pattern)
    return ws


@functools.lru_cache(maxsize=None)
def sphere(level):
    return R.octa_sphere(T.SPHERE["centre"], T.SPHERE["radius"], level)


def run(api, verts, faces, bbox, dims, position=S.POS_MEAN, skip=(), pattern=None):
    """The two C entries -> the dict tests/simplify_ref.py's simplify returns; outputs named in `skip` are passed as NULL"""
    lib = api[0].lib()
    verts, faces = np.asarray(verts, F32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)
    nv, nf = len(verts), len(faces)
    dv, df = (dev(verts, F32) if nv else None), (dev(faces, np.int32) if nf else None)
    box = np.asarray(bbox, F32)
    stats = None if "stats" in skip else torch.zeros((4,), dtype=torch.int32, device="cuda")
    ws = workspace(lib.nrf_mesh_simplify_workspace_bytes(nv, nf, *dims), pattern)
    ov, of = C.c_int64(-7), C.c_int64(-7)
    status = lib.nrf_mesh_simplify_count(p(dv), nv, p(df), nf, box.ctypes.data_as(C.c_void_p), *dims, C.addressof(ov), C.addressof(of), p(stats), p(ws), ws.numel(), None)
    assert status == 0, lib.nrf_last_error()
    ov, of = int(ov.value), int(of.value)
    out_v = torch.full((ov, 3), -7.0, device="cuda")
    out_f = torch.full((of, 3), -7, dtype=torch.int32, device="cuda")
    rep = None if "rep" in skip else torch.full((ov,), -7, dtype=torch.int32, device="cuda")
    src = None if "face_src" in skip else torch.full((of,), -7, dtype=torch.int32, device="cuda")
    cluster = None if "cluster" in skip else torch.full((nv,), -7, dtype=torch.int32, device="cuda")
    status = lib.nrf_mesh_simplify_emit(p(dv), nv, p(df), nf, box.ctypes.data_as(C.c_void_p), *dims, position, ov, of, p(out_v) if ov else None, p(out_f) if of else None,
                                        p(rep) if ov else None, p(src) if of else None, p(cluster) if nv else None, p(ws), ws.numel(), None)
    assert status == 0, lib.nrf_last_error()
    torch.cuda.synchronize()
    h = lambda t: None if t is None else t.cpu().numpy()
    return dict(n_verts=ov, n_faces=of, stats=None if stats is None else h(stats).view(np.uint32), verts=h(out_v), faces=h(out_f), rep=h(rep), face_src=h(src),
                cluster=h(cluster))


def assert_equal(got, want, what=""):
    assert (got["n_verts"], got["n_faces"]) == (want["n_verts"], want["n_faces"]), f"{what}: totals {got['n_verts']} / {got['n_faces']}, not {want['n_verts']} / {want['n_faces']}"
    gv, wv = got["verts"].view(np.uint32), want["verts"].view(np.uint32)
    assert np.array_equal(gv, wv), f"{what}: vertices differ at {np.nonzero((gv != wv).any(-1))[0][:8]}"
    assert np.array_equal(got["faces"], want["faces"]), f"{what}: faces"
    for k in OUTPUTS:
        if got[k] is not None:
            assert np.array_equal(got[k], want[k]), f"{what}: {k} differs at {np.nonzero(got[k] != want[k])[0][:8]}"


def check(api, verts, faces, bbox, dims, what, positions=(S.POS_MEAN, S.POS_MEMBER), patterns=(None, 0xA5)):
    """Both entries against the restatement: every position mode, twice, over differently filled workspaces"""
    want = None
    for position in positions:
        want = S.simplify(verts, faces, bbox, dims, position)
        for pattern in patterns:
            assert_equal(run(api, verts, faces, bbox, dims, position, pattern=pattern), want, f"{what}, position {position}, pattern {pattern}")
    return want


def soup(n_verts, n_faces, seed, spread=1.1):
    """Random vertices (some outside the unit box at the default spread) and random faces over them"""
    rng = np.random.default_rng(seed)
    verts = rng.uniform(-spread, spread, (n_verts, 3)).astype(F32)
    faces = rng.integers(0, max(n_verts, 1), (n_faces, 3)).astype(np.int32)
    return verts, faces


SIZES = [(0, 0), (1, 1), (63, 63), (64, 64), (65, 65), (1000, 1000), (4097, 4097), (0, 65), (65, 0), (4097, 63), (63, 4097), (1, 1000)]


@pytest.mark.parametrize("dims", [(1, 1, 1), (2, 3, 5), (32, 32, 32), (1024, 1, 1), (1, 1024, 1), (1, 1, 1024)])
def test_random_soups_equal_the_restatement(api, dims):
    kept = 0
    for k, (nv, nf) in enumerate(SIZES):
        verts, faces = soup(nv, nf, 100 + k)
        want = check(api, verts, faces, UNIT_BOX, dims, f"soup {nv} / {nf} on {dims}")
        kept += want["n_faces"]
        assert want["stats"][0] == (nf if nv == 0 else 0)
    assert (kept == 0) == (dims == (1, 1, 1)), "the soups exercise the emit kernels on every grid but the single cell"


@pytest.mark.parametrize("level", [3, 4, 5])
def test_spheres_equal_the_restatement(api, level):
    verts, faces = sphere(level)
    box = S.mesh_box(verts)
    for n in (1, 2, 6, 8, 12, 32):
        want = check(api, verts, faces, box, (n, n, n), f"sphere level {level}, n {n}")
        assert (want["n_faces"] == 0) == (n == 1)
    if level == 4:
        assert (want["n_verts"], want["n_faces"]) == (1026, 2048)


def test_more_than_one_scan_round_of_faces_and_cells(api):
    """The block totals are scanned 8 192 blocks of 256 at a time: 2 097 153 faces and 103 x 131 x 157 = 2 118 401 cells each need a second round and end one past a
    block boundary.  A vertex at the centre of every cell; every 97th face and the last one join three random cells, the others collapse"""
    dims, nf = (103, 131, 157), 8192 * 256 + 1
    cells = dims[0] * dims[1] * dims[2]
    assert cells > 8192 * 256 and cells % 256 == 1
    axes = [((np.arange(n, dtype=np.float64) + 0.5) * (2.0 / n) - 1.0) for n in dims]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    verts = np.stack([x, y, z], -1).reshape(-1, 3).astype(F32)
    assert np.array_equal(S.vertex_cells(verts, UNIT_BOX, dims)[0], np.arange(cells))
    rng = np.random.default_rng(7)
    k = rng.integers(0, cells, nf).astype(np.int32)
    faces = np.stack([k, k, (k + 1) % cells], 1).astype(np.int32)
    live = np.concatenate([np.arange(0, nf, 97), [nf - 1]])
    faces[live] = rng.integers(0, cells, (len(live), 3))
    faces[0], faces[nf - 1] = [0, 5, cells - 1], [cells - 2, 1, 7]
    want = check(api, verts, faces, UNIT_BOX, dims, "two scan rounds", positions=(S.POS_MEAN,), patterns=(0x5A,))
    assert want["n_faces"] > len(live) - 8 and want["face_src"][-1] == nf - 1 and want["cells"][0] == 0 and want["cells"][-1] == cells - 1
    assert (want["face_src"] > 8192 * 256 - 97 * 40).sum() > 30 and want["n_verts"] > 3 * len(live) - 2000


def test_vertices_on_cell_faces_and_outside_the_box(api):
    """Grid 4 x 4 x 4 over [0, 1]^3: every coordinate a multiple of 1/4 or the float next to it on either side, -0.25 .. 1.25; and values far outside"""
    base = np.arange(-1, 6, dtype=F32) * F32(0.25)
    coords = np.unique(np.concatenate([base, np.nextafter(base, F32(-10)), np.nextafter(base, F32(10))]))
    rng = np.random.default_rng(3)
    verts = rng.choice(coords, (1500, 3)).astype(F32)
    verts[:6] = [[3e38, 0.5, 0.5], [-3e38, 0.5, 0.5], [0.5, 3e38, -3e38], [1e30, -1e30, 0.1], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0]]
    faces = rng.integers(0, len(verts), (3000, 3)).astype(np.int32)
    faces[:4] = [[0, 1, 2], [3, 4, 5], [0, 4, 5], [5, 4, 3]]
    want = check(api, verts, faces, (0, 0, 0, 1, 1, 1), (4, 4, 4), "cell faces")
    assert want["n_faces"] > 1000 and np.isfinite(want["verts"]).all() and (want["cluster"] >= -1).all()
    check(api, verts, faces, (-1e30, 0, 0, 1, 1, 1), (2, 4, 4), "a box far wider than the mesh", positions=(S.POS_MEAN,))


def test_degenerate_bad_and_nonfinite_inputs(api):
    verts, faces = soup(500, 2000, 21)
    verts[[3, 50, 77]] = [[np.nan, 0, 0], [0, np.inf, 0], [0.5, 0.5, -np.inf]]
    faces[0:3] = [[5, 5, 9], [8, 8, 8], [9, 5, 9]]                                         # degenerate as given
    faces[10:16] = [[-1, 2, 4], [2, 500, 4], [2, 4, 2 ** 31 - 1], [-2 ** 31, 0, 1], [3, 4, 6], [4, 50, 77]]          # bad indices next to valid faces, non-finite corners
    faces[16] = [3, 600, 4]                                                                # bad comes first
    for dims in ((2, 3, 5), (8, 8, 8)):
        want = check(api, verts, faces, UNIT_BOX, dims, f"adversarial on {dims}")
        assert want["stats"][0] == 5 and want["stats"][1] >= 2 and want["stats"][2] >= 3 and want["cluster"][[3, 50, 77]].tolist() == [-1, -1, -1]


def one_per_cell(n=32):
    """A vertex at the centre of every cell of the n^3 grid over the unit box, in cell order"""
    c = (np.arange(n, dtype=np.float64) + 0.5) * (2.0 / n) - 1.0
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    return np.stack([x, y, z], -1).reshape(-1, 3).astype(F32)


def test_coincident_faces_meet_in_one_slot(api):
    """4 097 copies of one face: every insert meets the same slot.  Split even and odd: net positive, negative and (4 096 copies, half and half) zero"""
    verts, _ = soup(300, 0, 31, spread=1.0)
    cells = S.vertex_cells(verts, UNIT_BOX, (4, 4, 4))[0]
    a, b, c = (int(np.nonzero(cells == k)[0][0]) for k in np.unique(cells)[:3])
    a2, b2, c2 = (int(np.nonzero(cells == k)[0][1]) for k in np.unique(cells)[:3])
    even, odd = [a, b, c], [c, b, a]
    rng = np.random.default_rng(5)

    def copies(n_even, n_odd):
        rows = np.array([even] * n_even + [odd] * n_odd, np.int32)
        for r in rows:                                                 # any rotation, any of the two vertices of a cell: the same three cells
            r[:] = np.roll(r, rng.integers(3))
        swap = rng.random(len(rows)) < 0.5
        rows[swap] = np.select([rows[swap] == a, rows[swap] == b, rows[swap] == c], [a2, b2, c2])
        return rows[rng.permutation(len(rows))]
    for n_even, n_odd, kept in ((4097, 0, 1), (2049, 2048, 1), (2048, 2049, 1), (2048, 2048, 0), (0, 4097, 1)):
        faces = copies(n_even, n_odd)
        want = check(api, verts, faces, UNIT_BOX, (4, 4, 4), f"{n_even} even, {n_odd} odd")
        assert want["n_faces"] == kept and want["stats"][3] == len(faces) - kept and want["n_verts"] == 3 * kept
        if kept:
            cells_of = cells[faces[want["face_src"][0]]]
            assert (np.argsort(cells_of).tolist() in ([0, 1, 2], [1, 2, 0], [2, 0, 1])) == (n_even > n_odd)


@pytest.mark.parametrize("n_faces,distinct", [(4097, 4097), (4096, 4095), (4096, 4096)])
def test_distinct_triples_probe_past_occupied_slots(api, n_faces, distinct):
    """The table has the power of two >= 2F slots: 4 096 faces of 4 095 distinct triples fill 8 192 slots to just under one half, 4 097 fill 16 384 to a quarter"""
    verts = one_per_cell(32)
    k = np.arange(distinct, dtype=np.int32)
    faces = np.stack([k, k + 9000, k + 20000], 1)
    faces[1::2] = faces[1::2, ::-1]
    faces = np.concatenate([faces, faces[:n_faces - distinct]]).astype(np.int32)
    want = check(api, verts, faces, UNIT_BOX, (32, 32, 32), f"{distinct} distinct triples", patterns=(0xFF,))
    assert want["n_faces"] == distinct and want["n_verts"] == 3 * distinct and want["stats"].tolist() == [0, 0, 0, n_faces - distinct]
    assert np.array_equal(want["verts"].view(np.uint32), verts[want["rep"]].view(np.uint32)), "the mean of one vertex is the vertex (cell centres are exact)"


def test_unused_vertices_do_not_move_a_mean(api):
    verts, faces = sphere(4)
    box = S.mesh_box(verts)
    rng = np.random.default_rng(9)
    extra = (verts[rng.integers(0, len(verts), 700)] + rng.uniform(-0.05, 0.05, (700, 3))).astype(F32)
    more = np.concatenate([verts, extra])
    want = check(api, more, faces, box, (8, 8, 8), "unused vertices")
    alone = S.simplify(verts, faces, box, (8, 8, 8))
    assert np.array_equal(want["mean"].view(np.uint32), alone["mean"].view(np.uint32)) and np.array_equal(want["faces"], alone["faces"])
    assert (want["rep"] < len(verts)).all() and (want["cluster"][len(verts):] >= 0).any()


@pytest.mark.parametrize("skip", ["rep", "face_src", "cluster", "stats", OUTPUTS])
def test_optional_outputs_may_be_null(api, skip):
    verts, faces = sphere(4)
    box = S.mesh_box(verts)
    skip = (skip,) if isinstance(skip, str) else skip
    for position in (S.POS_MEAN, S.POS_MEMBER):
        got = run(api, verts, faces, box, (6, 6, 6), position, skip=skip)
        assert all(got[k] is None for k in skip)
        assert_equal(got, S.simplify(verts, faces, box, (6, 6, 6), position), f"without {skip}")


def test_twice_and_over_dirty_workspaces(api):
    verts, faces = soup(3000, 4097, 13)
    faces[:64] = faces[64:128, ::-1]          # some cancel
    for dims in ((2, 3, 5), (12, 12, 12)):
        for position in (S.POS_MEAN, S.POS_MEMBER):
            want = S.simplify(verts, faces, UNIT_BOX, dims, position)
            for pattern in PATTERNS:
                for again in range(2):
                    assert_equal(run(api, verts, faces, UNIT_BOX, dims, position, pattern=pattern), want, f"{dims}, position {position}, pattern {pattern:#x}, run {again}")


def test_stats_are_added_to(api):
    lib = api[0].lib()
    verts, faces = sphere(4)
    box = S.mesh_box(verts)
    want = S.simplify(verts, faces, box, (6, 6, 6))
    dv, df = dev(verts, F32), dev(faces, np.int32)
    stats = torch.tensor([5, 6, 7, 8], dtype=torch.int32, device="cuda")
    ws = workspace(lib.nrf_mesh_simplify_workspace_bytes(len(verts), len(faces), 6, 6, 6), 0xA5)
    ov, of = C.c_int64(), C.c_int64()
    for k in (1, 2):
        assert lib.nrf_mesh_simplify_count(p(dv), len(verts), p(df), len(faces), box.ctypes.data_as(C.c_void_p), 6, 6, 6, C.addressof(ov), C.addressof(of), p(stats), p(ws),
                                           ws.numel(), None) == 0
        assert stats.cpu().numpy().tolist() == (np.array([5, 6, 7, 8]) + k * want["stats"].astype(np.int64)).tolist()


def test_refusals_over_live_buffers_write_nothing(api):
    lib = api[0].lib()
    verts, faces = sphere(3)
    box = S.mesh_box(verts)
    nv, nf, dims = len(verts), len(faces), (6, 6, 6)
    dv, df = dev(verts, F32), dev(faces, np.int32)
    need = lib.nrf_mesh_simplify_workspace_bytes(nv, nf, *dims)
    ws = workspace(need, 0xA5)
    pb = lambda a: a.ctypes.data_as(C.c_void_p)
    ov, of = C.c_int64(-7), C.c_int64(-7)
    stats = torch.zeros((4,), dtype=torch.int32, device="cuda")

    def count(ws_bytes=need, b=box, d=dims, n_v=C.addressof(ov)):
        return lib.nrf_mesh_simplify_count(p(dv), nv, p(df), nf, pb(b), *d, n_v, C.addressof(of), p(stats), p(ws), ws_bytes, None)
    for status, kw in ((WORKSPACE, dict(ws_bytes=need - 1)), (INVALID_ARG, dict(b=np.array([0, 0, 0, 1, 0, 1], F32))), (INVALID_ARG, dict(d=(6, 6, 0))), (INVALID_ARG, dict(n_v=None))):
        assert count(**kw) == status and lib.nrf_last_error().startswith(b"nrf_mesh_simplify_count"), kw
    torch.cuda.synchronize()
    assert (ws == 0xA5).all() and (ov.value, of.value) == (-7, -7) and stats.cpu().numpy().tolist() == [0, 0, 0, 0]
    assert count() == 0
    want = S.simplify(verts, faces, box, dims)
    assert (ov.value, of.value) == (want["n_verts"], want["n_faces"]) == (116, 228)
    out_v = torch.full((ov.value + 8, 3), -7.0, device="cuda")
    out_f = torch.full((of.value + 8, 3), -7, dtype=torch.int32, device="cuda")
    rep = torch.full((ov.value + 8,), -7, dtype=torch.int32, device="cuda")
    src = torch.full((of.value + 8,), -7, dtype=torch.int32, device="cuda")
    cluster = torch.full((nv,), -7, dtype=torch.int32, device="cuda")
    before = ws.clone()

    def emit(n_v=ov.value, n_f=of.value, pos=0, ws_bytes=need, d=dims, v_out=p(out_v)):
        return lib.nrf_mesh_simplify_emit(p(dv), nv, p(df), nf, pb(box), *d, pos, n_v, n_f, v_out, p(out_f), p(rep), p(src), p(cluster), p(ws), ws_bytes, None)
    # a wrong total: larger, smaller, both, out of range
    for kw in (dict(n_v=ov.value + 1), dict(n_v=ov.value - 1), dict(n_f=of.value + 1), dict(n_f=of.value - 1), dict(n_v=0, n_f=0), dict(n_v=-1), dict(n_f=nf + 1), dict(pos=2),
               dict(v_out=None), dict(d=(6, 6, 0))):
        assert emit(**kw) == INVALID_ARG and lib.nrf_last_error().startswith(b"nrf_mesh_simplify_emit"), kw
    assert emit(ws_bytes=need - 1) == WORKSPACE
    torch.cuda.synchronize()
    assert (out_v == -7).all() and (out_f == -7).all() and (rep == -7).all() and (src == -7).all() and (cluster == -7).all() and torch.equal(ws, before)
    assert emit() == 0
    torch.cuda.synchronize()
    assert (out_v[ov.value:] == -7).all() and (out_f[of.value:] == -7).all() and (rep[ov.value:] == -7).all() and (src[of.value:] == -7).all(), "nothing beyond the totals"
    got = dict(n_verts=ov.value, n_faces=of.value, verts=out_v[:ov.value].cpu().numpy(), faces=out_f[:of.value].cpu().numpy(), rep=rep[:ov.value].cpu().numpy(),
               face_src=src[:of.value].cpu().numpy(), cluster=cluster.cpu().numpy(), stats=stats.cpu().numpy().view(np.uint32))
    assert_equal(got, want, "after the refusals")


# ------------------------------------------------------------------------------------ the Python layer
def coloured_sphere(mesh, level):
    verts, faces = sphere(level)
    v = torch.from_numpy(verts).cuda()
    centre = torch.tensor(T.SPHERE["centre"], device="cuda", dtype=torch.float32)
    normals = (v - centre) / T.SPHERE["radius"]
    idx = torch.arange(len(verts), device="cuda", dtype=torch.float32)
    return mesh.Mesh(v, torch.from_numpy(faces).cuda(), normals, 0.5 + 0.5 * normals, torch.stack([idx, -idx], 1))


def test_simplify_mesh_carries_the_attributes_of_the_representative(api):
    _, _, mesh = api
    m = coloured_sphere(mesh, 4)
    verts, faces = sphere(4)
    for kw, dims in ((dict(resolution=6), (6, 6, 6)), (dict(resolution=(4, 6, 8)), (4, 6, 8))):
        for position in ("mean", "member"):
            out, (cluster, face_src, rep, stats) = mesh.SimplifyMesh(m, position=position, return_maps=True, **kw)
            want = S.simplify(verts, faces, S.mesh_box(verts), dims, mesh._POSITIONS[position])
            got = dict(n_verts=out.Vertices.shape[0], n_faces=out.Faces.shape[0], verts=out.Vertices.cpu().numpy(), faces=out.Faces.cpu().numpy(), rep=rep.cpu().numpy(),
                       face_src=face_src.cpu().numpy(), cluster=cluster.cpu().numpy(), stats=stats.cpu().numpy().view(np.uint32))
            assert_equal(got, want, f"SimplifyMesh {kw} {position}")
            at = rep.to(torch.int64)
            assert torch.equal(out.Normals, m.Normals[at]) and torch.equal(out.Colors, m.Colors[at]) and torch.equal(out.Relevancy, m.Relevancy[at])
            assert torch.equal(out.Relevancy[:, 0], rep.to(torch.float32))
    # cube cells: n = ceil(extent / cell_size) per axis over [bmin, bmin + n * cell_size]
    box = S.mesh_box(verts)
    cell = 0.3
    n = [int(np.ceil((float(box[3 + a]) - float(box[a])) / cell)) for a in range(3)]
    cube = np.concatenate([box[:3], (box[:3].astype(np.float64) + np.array(n) * cell).astype(F32)])
    out = mesh.SimplifyMesh(m, cell_size=cell)
    want = S.simplify(verts, faces, cube, n)
    assert n == [5, 5, 5] and np.array_equal(out.Vertices.cpu().numpy().view(np.uint32), want["verts"].view(np.uint32)) and np.array_equal(out.Faces.cpu().numpy(), want["faces"])
    empty = mesh.SimplifyMesh(m, resolution=1)
    assert empty.Vertices.shape == (0, 3) and empty.Faces.shape == (0, 3) and empty.Normals.shape == (0, 3) and empty.Colors.shape == (0, 3) and empty.Relevancy.shape == (0, 2)
    none = mesh.SimplifyMesh(mesh.Mesh(m.Vertices[:0], m.Faces[:0], m.Normals[:0]), cell_size=0.1)
    assert none.Vertices.shape == (0, 3) and none.Faces.shape == (0, 3) and none.Colors is None
    lv, lf = R.lattice_mesh(0.1)          # a plane: zero extent on z, widened by one cell
    lv_t = torch.from_numpy(lv).cuda()
    flat = mesh.SimplifyMesh(mesh.Mesh(lv_t, torch.from_numpy(lf).cuda(), torch.zeros_like(lv_t)), resolution=(4, 4, 2))
    lbox = S.mesh_box(lv)
    lbox[5] = F32(float(lbox[2]) + max(float(lbox[3]) - float(lbox[0]), float(lbox[4]) - float(lbox[1])) / 4)
    want = S.simplify(lv, lf, lbox, (4, 4, 2))
    assert want["n_faces"] > 0 and np.array_equal(flat.Vertices.cpu().numpy().view(np.uint32), want["verts"].view(np.uint32)) and np.array_equal(flat.Faces.cpu().numpy(), want["faces"])
    for bad in (dict(), dict(cell_size=0.1, resolution=4), dict(cell_size=0.0), dict(resolution=4, position="median")):
        with pytest.raises(api[0].NrfError):
            mesh.SimplifyMesh(m, **bad)


def test_simplify_to_faces(api):
    _, _, mesh = api
    m = coloured_sphere(mesh, 5)
    lib = api[0].lib()
    calls = []
    real = lib.nrf_mesh_simplify_count

    class Counting:          # the library handle with one entry wrapped
        def __getattr__(self, name):
            if name == "nrf_mesh_simplify_count":
                return lambda *a: (calls.append(a[5:8]), real(*a))[1]
            return getattr(lib, name)
    orig = api[0].lib
    api[0].lib = lambda: Counting()
    try:
        out, n = mesh.SimplifyToFaces(m, 1000)
    finally:
        api[0].lib = orig
    assert 0 < out.Faces.shape[0] <= 1000 and len(calls) <= 11 and calls[-1] == (n, n, n)
    same = mesh.SimplifyMesh(m, resolution=n)
    assert torch.equal(out.Vertices, same.Vertices) and torch.equal(out.Faces, same.Faces) and torch.equal(out.Colors, same.Colors)
    verts, faces = sphere(5)
    tried = {c[0]: S.simplify(verts, faces, S.mesh_box(verts), c)["n_faces"] for c in set(calls)}
    assert tried[n] == out.Faces.shape[0] and all(k <= n or f > 1000 for k, f in tried.items()), "the largest n tried that qualifies"
    zero, n1 = mesh.SimplifyToFaces(m, 0)
    assert zero.Faces.shape[0] == 0 and n1 >= 1


def test_extract_mesh_simplifies_before_the_network(api):
    _, _, mesh = api
    from nerfpp_amd import scene
    sc = scene.make_hash_scene(mode="ngp")
    g = mesh.DensityGrid(sc["renderer"], None, 48)
    iso = float(torch.quantile(g.reshape(-1), 0.7))
    b = np.asarray(sc["bbox"], np.float64).reshape(6)
    cell = 3.0 * float((b[3:] - b[:3]).max()) / 47
    full = mesh.ExtractMesh(sc["renderer"], iso, resolution=48, colors=False, keep_largest=1)
    want = mesh.SimplifyMesh(full, cell_size=cell)
    for normals in ("lattice", "field"):
        got = mesh.ExtractMesh(sc["renderer"], iso, resolution=48, keep_largest=1, simplify_cell=cell, normals=normals)
        assert 0 < got.Faces.shape[0] < full.Faces.shape[0] // 4
        assert torch.equal(got.Vertices, want.Vertices) and torch.equal(got.Faces, want.Faces)
        assert got.Colors.shape == got.Vertices.shape and torch.isfinite(got.Colors).all() and got.Normals.shape == got.Vertices.shape
    assert torch.equal(mesh.ExtractMesh(sc["renderer"], iso, resolution=48, colors=False, keep_largest=1, simplify_cell=cell).Normals, want.Normals)


def test_the_simplified_sphere_stays_within_a_cell_of_the_input(api):
    """Every used vertex moves by at most one cell diagonal, and a point of a face is a convex combination of its corners: the Chamfer distance between sampled
    points of the two surfaces is at most sqrt(3) * cell; per vertex, the distance to its cluster's position is too"""
    _, geometry, mesh = api
    m = coloured_sphere(mesh, 5)
    for n in (8, 16):
        out, (cluster, _, _, _) = mesh.SimplifyMesh(m, resolution=n, return_maps=True)
        verts = sphere(5)[0]
        box = S.mesh_box(verts).astype(np.float64)
        cell = float((box[3:] - box[:3]).max()) / n
        d = geometry.SurfaceDistance(out, m, n_points=20000, seed=1)
        print(f"n {n}: {out.Faces.shape[0]} faces, Chamfer {float(d.Chamfer):.5f}, Hausdorff {float(d.Hausdorff):.5f}, sqrt(3) cell {np.sqrt(3) * cell:.5f}")
        assert float(d.Chamfer) <= np.sqrt(3.0) * cell
        has = cluster >= 0
        moved = torch.linalg.vector_norm(m.Vertices[has] - out.Vertices[cluster[has].to(torch.int64)], dim=1)
        assert has.any() and float(moved.max()) <= np.sqrt(3.0) * cell * (1 + 1e-6)
