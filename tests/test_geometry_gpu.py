"""Geometry in space on the MI355X: nrf_mesh_sample_count / _emit, nrf_nearest_points and nrf_distance_stats against the numpy restatement (tests/geometry_ref.py)
with uint32 / integer equality -- the sphere and an adversarial mesh, every size and grid at which the search takes another path, points on cell faces, exact ties
across rings, the brute-force fallback, max_dist at a float's edge -- the run-to-run guarantees, the refusals over live buffers, and the Python layer built on them:
SampleSurface, InterpolateAttributes, NearestPoints, TransferAttributes and SurfaceDistance.  No input here is outside the contract: bad indices and non-finite
values have a defined answer and are rejected before any dereference."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import geometry_ref as G
import raster_ref as R
import tsdf_ref as T

pytestmark = pytest.mark.gpu

F32 = np.float32
INVALID_ARG, WORKSPACE = 1, 4
INF = float("inf")
UNIT_BOX = (-1, -1, -1, 1, 1, 1)


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from nerfpp_amd import _lib as L, geometry, mesh
    return L, geometry, mesh


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, F32).view(np.uint32)


def bits64(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


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
def sphere(radius=0.7):
    return R.octa_sphere(T.SPHERE["centre"], radius)


# ------------------------------------------------------------------------------------ 1. sampling
def run_sample(api, verts, faces, density, seed, skip=(), pattern=None):
    """The two C entries -> dict(n_points, total_area, points, face, uv, stats); outputs named in `skip` are passed as NULL"""
    lib = api[0].lib()
    verts, faces = np.asarray(verts, F32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)
    dv, df = (dev(verts, F32) if len(verts) else None), (dev(faces, np.int32) if len(faces) else None)
    stats = None if "stats" in skip else torch.zeros((3,), dtype=torch.int32, device="cuda")
    ws = workspace(lib.nrf_mesh_sample_workspace_bytes(len(verts), len(faces)), pattern)
    n, area = C.c_int64(-7), C.c_double(-7.0)
    status = lib.nrf_mesh_sample_count(p(dv), len(verts), p(df), len(faces), density, seed, C.addressof(n), C.addressof(area), p(stats), p(ws), ws.numel(), None)
    assert status == 0, lib.nrf_last_error()
    n = int(n.value)
    pts = torch.full((n, 3), -7.0, device="cuda")
    face = None if "face" in skip else torch.full((n,), -7, dtype=torch.int32, device="cuda")
    uv = None if "uv" in skip else torch.full((n, 2), -7.0, device="cuda")
    status = lib.nrf_mesh_sample_emit(p(dv), len(verts), p(df), len(faces), seed, n, p(pts) if n else None, p(face) if n else None, p(uv) if n else None, p(ws), ws.numel(), None)
    assert status == 0, lib.nrf_last_error()
    torch.cuda.synchronize()
    h = lambda t: None if t is None else t.cpu().numpy()
    return dict(n_points=n, total_area=float(area.value), points=h(pts), face=h(face), uv=h(uv), stats=None if stats is None else h(stats).view(np.uint32))


@functools.lru_cache(maxsize=None)
def sample_reference(name, density, seed):
    verts, faces = sphere() if name == "sphere" else G.adversarial_mesh()[:2]
    c, pts, face, uv = G.sample(verts, faces, density, seed)
    return dict(n_points=c["n_points"], total_area=c["total_area"], points=pts, face=face, uv=uv, stats=c["stats"])


def assert_sample_equal(got, want, what=""):
    assert got["n_points"] == want["n_points"], f"{what}: {got['n_points']} points, not {want['n_points']}"
    assert np.float64(got["total_area"]).view(np.uint64) == np.float64(want["total_area"]).view(np.uint64), f"{what}: area {got['total_area']!r} != {want['total_area']!r}"
    assert np.array_equal(bits(got["points"]), bits(want["points"])), f"{what}: points"
    if got["face"] is not None:
        assert np.array_equal(got["face"], want["face"]), f"{what}: face"
    if got["uv"] is not None:
        assert np.array_equal(bits(got["uv"]), bits(want["uv"])), f"{what}: uv"
    if got["stats"] is not None:
        assert np.array_equal(got["stats"], want["stats"]), f"{what}: stats {got['stats']} != {want['stats']}"


@pytest.mark.parametrize("density,about", [(0.0, 0), (170.0, 1000), (3400.0, 20000)])
def test_sphere_samples_equal_the_restatement(api, density, about):
    verts, faces = sphere()
    want = sample_reference("sphere", density, 4)
    assert abs(want["n_points"] - about) <= 0.05 * about and (about == 0 or len(np.unique(want["face"])) > 400)
    assert_sample_equal(run_sample(api, verts, faces, density, 4), want, f"density {density}")


def test_adversarial_mesh_every_class_counted(api):
    verts, faces, kinds = G.adversarial_mesh()
    for density in (1.0, 50.0):
        want = sample_reference("adversarial", density, 3)
        assert (want["stats"] > 0).all() and want["n_points"] > G.SAMPLE_MAX_PER_FACE
        got = run_sample(api, verts, faces, density, 3, pattern=0xA5)
        assert_sample_equal(got, want, f"adversarial, density {density}")
        assert np.isfinite(got["points"]).all()


def test_sampling_more_than_one_scan_round_of_faces(api):
    """The block totals of the point counts are scanned 8 192 blocks of 256 at a time: 2 097 153 faces need a second round and end one past a block boundary.  Small
    faces over eleven vertices at a density that gives most of them no point and nearly all the others one; the first and the last face are large.  A point's face is
    found by a search in the offsets, so `face` equal to the restatement's is the offsets equal to its; the total is n_points"""
    nf = 8192 * 256 + 1
    rng = np.random.default_rng(21)
    verts = np.concatenate([rng.uniform(-0.05, 0.05, (8, 3)), [[-1, -1, 0], [1, -1, 0], [0, 1, 0.5]]]).astype(F32)
    faces = rng.integers(0, 8, (nf, 3)).astype(np.int32)
    faces[0] = faces[nf - 1] = [8, 9, 10]
    density = 2.0
    want = dict(zip(("c", "points", "face", "uv"), G.sample(verts, faces, density, 6)))
    c = want.pop("c")
    want.update(n_points=c["n_points"], total_area=c["total_area"], stats=c["stats"])
    assert 1000 < c["n_points"] < 40000 and (c["count"][1:-1] <= 1).all() and c["count"][0] >= 4 and c["count"][-1] >= 4 and c["offset"][-1] == c["n_points"] - c["count"][-1]
    assert want["face"][-1] == nf - 1 and ((want["face"] >= 8191 * 256) & (want["face"] < nf - 1)).any()
    assert_sample_equal(run_sample(api, verts, faces, density, 6, pattern=0x5A), want, "two scan rounds")


def test_empty_meshes(api):
    _, faces = sphere()
    got = run_sample(api, np.zeros((0, 3), F32), faces, 10.0, 0)          # no vertices: every face has a bad index
    assert got["n_points"] == 0 and got["total_area"] == 0.0 and got["stats"].tolist() == [len(faces), 0, 0]
    got = run_sample(api, sphere()[0], np.zeros((0, 3), np.int32), 10.0, 0, pattern=0xFF)
    assert got["n_points"] == 0 and got["total_area"] == 0.0 and got["stats"].tolist() == [0, 0, 0]
    got = run_sample(api, np.zeros((0, 3), F32), np.zeros((0, 3), np.int32), 10.0, 0)
    assert got["n_points"] == 0 and got["total_area"] == 0.0


@pytest.mark.parametrize("skip", ["face", "uv", "stats", ("face", "uv", "stats")])
def test_optional_sample_outputs_may_be_null(api, skip):
    verts, faces = sphere()
    skip = (skip,) if isinstance(skip, str) else skip
    got = run_sample(api, verts, faces, 170.0, 4, skip=skip)
    assert all(got[k] is None for k in skip)
    assert_sample_equal(got, sample_reference("sphere", 170.0, 4), f"without {skip}")


def test_sampling_twice_and_over_a_dirty_workspace(api):
    verts, faces = sphere()
    a = run_sample(api, verts, faces, 3400.0, 9)
    for pattern in (None, 0x00, 0xFF, 0x5A):
        b = run_sample(api, verts, faces, 3400.0, 9, pattern=pattern)
        assert_sample_equal(b, a, f"pattern {pattern}")
    other = run_sample(api, verts, faces, 3400.0, 10)
    assert not np.array_equal(bits(other["points"][:1000]), bits(a["points"][:1000])), "another seed gives other points"


# ------------------------------------------------------------------------------------ 2. nearest points
def run_nearest(api, query, target, bbox=UNIT_BOX, cells=(4, 4, 4), max_dist=INF, stats=True, pattern=None):
    """The C entry -> (d2 [nq] f32, index [nq] i32, stats [3] u32 or None)"""
    lib = api[0].lib()
    q, t = np.asarray(query, F32).reshape(-1, 3), np.asarray(target, F32).reshape(-1, 3)
    dq, dt = (dev(q, F32) if len(q) else None), (dev(t, F32) if len(t) else None)
    d2 = torch.full((len(q),), -7.0, device="cuda")
    idx = torch.full((len(q),), -7, dtype=torch.int32, device="cuda")
    st = torch.zeros((3,), dtype=torch.int32, device="cuda") if stats else None
    ws = workspace(lib.nrf_nearest_points_workspace_bytes(len(q), len(t), *cells), pattern)
    box = np.asarray(bbox, F32)
    status = lib.nrf_nearest_points(p(dq), len(q), p(dt), len(t), box.ctypes.data_as(C.c_void_p), *cells, max_dist, p(d2) if len(q) else None, p(idx) if len(q) else None,
                                    p(st), p(ws), ws.numel(), None)
    assert status == 0, lib.nrf_last_error()
    torch.cuda.synchronize()
    return d2.cpu().numpy(), idx.cpu().numpy(), None if st is None else st.cpu().numpy().view(np.uint32)


def assert_nearest_equal(got, want, what=""):
    assert np.array_equal(bits(got[0]), bits(want[0])), f"{what}: d2 differs at {np.nonzero(bits(got[0]) != bits(want[0]))[0][:8]}"
    assert np.array_equal(got[1], want[1]), f"{what}: index differs at {np.nonzero(got[1] != want[1])[0][:8]}"
    if got[2] is not None and len(got[0]):
        assert np.array_equal(got[2][:2], want[2][:2]), f"{what}: stats {got[2]} != {want[2]}"


@functools.lru_cache(maxsize=None)
def cloud(n, seed, spread=1.0):
    """n points, most of them uniform in the unit box, every 7th up to 1.5 x outside it, every 50th a duplicate of the first"""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-1, 1, (n, 3)).astype(F32) * F32(spread)
    pts[::7] *= F32(1.5)
    pts[::50] = pts[:1]
    return pts


SIZES = (0, 1, 63, 64, 65, 1000, 4097)


@functools.lru_cache(maxsize=None)
def cloud_reference(nq, nt):
    return G.nearest(cloud(nq, 100 + nq), cloud(nt, 200 + nt))


@pytest.mark.parametrize("nt", SIZES)
def test_every_size_equals_the_restatement(api, nt):
    for nq in SIZES:
        got = run_nearest(api, cloud(nq, 100 + nq), cloud(nt, 200 + nt), cells=(5, 4, 6))
        assert_nearest_equal(got, cloud_reference(nq, nt), f"nq {nq} nt {nt}")
        if nq and nt >= 1000:
            assert got[2][2] == 0, "a dense cloud needs no fallback"


@pytest.mark.parametrize("cells", [(1, 1, 1), (2, 3, 5), (32, 32, 32), (1024, 1, 1), (1, 1024, 1), (1, 1, 1024)])
def test_every_grid_gives_the_same_bits(api, cells):
    want = cloud_reference(1000, 4097)
    assert len(np.unique(want[1])) > 500
    assert_nearest_equal(run_nearest(api, cloud(1000, 1100), cloud(4097, 4297), cells=cells, pattern=0xA5), want, f"grid {cells}")
    assert_nearest_equal(run_nearest(api, cloud(4097, 4197), cloud(1000, 1200), cells=cells, stats=False), cloud_reference(4097, 1000), f"grid {cells}, swapped")


def test_more_than_one_scan_round_of_cells(api):
    """The block totals of the cell counts are scanned 8 192 blocks of 256 at a time: a grid of 129 x 128 x 128 = 2 113 536 cells (the call allows 2^26, each side up to
    1 024) needs a second round.  A sparse cloud, with targets in the first cell, either side of cell 2 097 152, beyond it and in the last cell; every query lies
    within a fifth of a cell of a target, so the rings serve it from the start array -- a wrong start would send it to the fallback, which no query here needs"""
    cells = (129, 128, 128)
    h = np.array([2.0 / n for n in cells])
    corner = np.array([[0, 0, 0], [127, 0, 127], [128, 0, 127], [0, 1, 127], [64, 64, 127], [128, 127, 127]], np.float64)
    own = (corner[:, 2] * cells[1] + corner[:, 1]) * cells[0] + corner[:, 0]
    assert own.tolist() == [0, 8192 * 256 - 1, 8192 * 256, 8192 * 256 + 1, own[4], cells[0] * cells[1] * cells[2] - 1] and own[4] > 8192 * 256 + 256
    rng = np.random.default_rng(31)
    target = np.concatenate([(-1.0 + (corner + 0.5) * h)[np.arange(60) % 6] + rng.uniform(-0.3, 0.3, (60, 3)) * h, cloud(4097, 4297)]).astype(F32)
    near = np.concatenate([np.arange(60), rng.choice(np.arange(60, len(target)), 900, replace=False)])
    query = (target[near] + rng.uniform(-0.2, 0.2, (len(near), 3)) * h.min()).astype(F32)
    want = G.nearest(query, target)
    assert len(np.unique(want[1])) > 900 and (want[0] < (0.4 * h.min()) ** 2).all()
    got = run_nearest(api, query, target, cells=cells, pattern=0xA5)
    assert_nearest_equal(got, want, "two scan rounds")
    assert got[2][2] == 0, "no query needs the fallback"


def face_points(n_cells=8):
    """Coordinates on the cell faces of an n^3 grid over [0, 1]^3 (h = 1/8 is a float) and one float either side, on all three axes"""
    c = []
    for k in range(n_cells + 1):
        x = F32(k) / F32(n_cells)
        c += [G.next_float(x, False), x, G.next_float(x)]
    return np.array(c, F32)


def test_points_on_cell_faces_and_one_float_either_side(api):
    c = face_points()
    rng = np.random.default_rng(8)
    target = np.stack([rng.choice(c, 600), rng.choice(c, 600), rng.choice(c, 600)], -1)
    query = np.stack([rng.choice(c, 500), rng.choice(c, 500), rng.choice(c, 500)], -1)
    query[::3] += rng.uniform(-0.06, 0.06, query[::3].shape).astype(F32)
    want = G.nearest(query, target)
    for cells in ((8, 8, 8), (16, 8, 4), (7, 9, 11)):
        assert_nearest_equal(run_nearest(api, query, target, bbox=(0, 0, 0, 1, 1, 1), cells=cells), want, f"faces, grid {cells}")
    # a sparse set: every query has to look several rings away, where the stop rule's slack decides
    sparse = target[:12]
    assert_nearest_equal(run_nearest(api, query, sparse, bbox=(0, 0, 0, 1, 1, 1), cells=(8, 8, 8)), G.nearest(query, sparse), "faces, sparse")
    assert_nearest_equal(run_nearest(api, query, sparse, bbox=(0, 0, 0, 1, 1, 1), cells=(64, 64, 64)), G.nearest(query, sparse), "faces, sparse, fine grid")


def test_points_far_outside_the_box(api):
    rng = np.random.default_rng(12)
    target = np.concatenate([cloud(500, 1), rng.uniform(-80, 80, (40, 3)).astype(F32)])
    query = np.concatenate([rng.uniform(-50, 50, (300, 3)).astype(F32), cloud(200, 2), np.array([[1e30, 0, 0], [0, -3e38, 3e38]], F32)])
    want = G.nearest(query, target)
    assert (np.abs(target[want[1]]).max(-1) > 1).sum() > 50, "border cells hold the nearest point of many queries"
    for cells in ((6, 6, 6), (32, 32, 32)):
        assert_nearest_equal(run_nearest(api, query, target, cells=cells), want, f"outside, grid {cells}")


def test_duplicates_and_ties_across_rings(api):
    # duplicates: the lowest index wins
    target = np.tile(cloud(100, 3), (4, 1))[np.random.default_rng(4).permutation(400)]
    got = run_nearest(api, cloud(300, 5), target, cells=(6, 6, 6))
    assert_nearest_equal(got, G.nearest(cloud(300, 5), target), "duplicates")
    first = {tuple(r): i for i, r in reversed(list(enumerate(map(tuple, target))))}
    assert all(first[tuple(target[j])] == j for j in got[1])
    # an exact tie between rings: grid 8^3 over [0, 8]^3, the query in cell 3; a higher index at the same distance in the nearer ring must lose
    query = np.array([[3.5, 3.5, 3.5]], F32)
    for near, far, d2 in (((3.0, 3.5, 3.5), (4.0, 3.5, 3.5), 0.25),          # ring 0 against ring 1
                          ((3.5, 2.0, 3.5), (3.5, 3.5, 5.0), 2.25),          # ring 1 against ring 2
                          ((0.5, 3.5, 3.5), (3.5, 6.5, 3.5), 9.0)):          # ring 3 against ring 3
        target = np.array([(7.9, 7.9, 7.9), far, (0.1, 0.1, 0.1), near], F32)
        got = run_nearest(api, query, target, bbox=(0, 0, 0, 8, 8, 8), cells=(8, 8, 8))
        assert got[0][0] == F32(d2) and got[1][0] == 1, (near, far, got)
        assert_nearest_equal(got, G.nearest(query, target), "tie")


def test_the_fallback_serves_what_the_rings_do_not_reach(api):
    # one target in the far corner of a 64^3 grid: every query is listed (16 waves of them) and brute-forced
    target = np.array([[0.99, 0.99, 0.99]], F32)
    query = cloud(1000, 6) * F32(0.3) - F32(0.5)
    got = run_nearest(api, query, target, cells=(64, 64, 64))
    assert_nearest_equal(got, G.nearest(query, target), "far corner")
    assert got[2].tolist() == [0, 0, 1000] and (got[1] == 0).all()
    # grid 32^3 over [0, 32]^3 (h = 1), R = NRF_NN_MAX_RINGS: a target R - 0.8 away in ring R is settled by ring R (B = 0.999 R is larger); one cell farther, in ring
    # R + 1, it is not
    rings = G.NN_MAX_RINGS
    assert 1 <= rings <= 20
    query = np.array([[10.9, 10.5, 10.5]], F32)
    for x, listed in ((10.1 + rings, 0), (11.1 + rings, 1)):
        target = np.array([[x, 10.5, 10.5]], F32)
        got = run_nearest(api, query, target, bbox=(0, 0, 0, 32, 32, 32), cells=(32, 32, 32))
        assert_nearest_equal(got, G.nearest(query, target), f"target at {x}")
        assert got[1][0] == 0 and got[2][2] == listed, (x, got)
    # a mixture: a dense cloud in one corner, queries everywhere
    target = cloud(2000, 7) * F32(0.3) + F32(0.5)
    query = cloud(1500, 8)
    got = run_nearest(api, query, target, cells=(40, 40, 40))
    assert_nearest_equal(got, G.nearest(query, target), "mixture")
    assert 100 < got[2][2] < 1500


def test_non_finite_points_max_dist_and_overflow(api):
    target, query = cloud(500, 9).copy(), cloud(300, 10).copy()
    target[[3, 77, 400], [0, 1, 2]] = [np.nan, np.inf, -np.inf]
    query[[0, 150, 299], [2, 0, 1]] = [np.nan, -np.inf, np.inf]
    want = G.nearest(query, target)
    got = run_nearest(api, query, target, cells=(7, 7, 7))
    assert_nearest_equal(got, want, "non-finite")
    assert got[2][:2].tolist() == [3, 3] and (got[1][[0, 150, 299]] == -1).all() and np.isinf(got[0][[0, 150, 299]]).all() and not np.isin(got[1], [3, 77, 400]).any()
    # max_dist: a target at exactly max_dist is included, one float beyond it is excluded
    q = np.zeros((1, 3), F32)
    at, beyond = np.array([[0, 0.5, 0]], F32), np.array([[G.next_float(0.5), 0, 0]], F32)
    for t, md, index in ((at, 0.5, 0), (at, float(G.next_float(0.5, False)), -1), (beyond, 0.5, -1), (beyond, float(G.next_float(0.5)), 0), (at, 0.0, -1), (q, 0.0, 0),
                         (np.concatenate([beyond, at]), 0.5, 1), (np.concatenate([beyond, at]), INF, 1)):
        got = run_nearest(api, q, t, cells=(4, 4, 4), max_dist=md)
        assert got[1][0] == index, (t, md, got)
        assert_nearest_equal(got, G.nearest(q, t, md), f"max_dist {md}")
    for md in (0.05, 0.2):
        got = run_nearest(api, cloud(1000, 1100), cloud(4097, 4297), cells=(32, 32, 32), max_dist=md)
        assert_nearest_equal(got, G.nearest(cloud(1000, 1100), cloud(4097, 4297), md), f"cloud, max_dist {md}")
        assert 0 < (got[1] < 0).sum() < 1000 and got[2][2] == 0, "beyond max_dist a query is finished, not listed"
    # 3e19: d2 overflows to +inf and the index is still valid
    q = np.array([[3e19, 0, 0], [0, 0, 0]], F32)
    t = np.array([[-3e19, 0, 0], [1e19, 1, 0]], F32)
    got = run_nearest(api, q, t, cells=(4, 4, 4))
    assert np.isinf(got[0][0]) and got[1].tolist() == [0, 1] and np.isfinite(got[0][1])
    assert_nearest_equal(got, G.nearest(q, t), "3e19")


def test_permutation_runs_and_dirty_workspace(api):
    query, target = cloud(1000, 1100), cloud(4097, 4297)
    base = run_nearest(api, query, target, cells=(16, 16, 16))
    for pattern in (None, 0x00, 0xFF, 0x5A):
        assert_nearest_equal(run_nearest(api, query, target, cells=(16, 16, 16), pattern=pattern), base, f"pattern {pattern}")
    perm = np.random.default_rng(13).permutation(len(target))
    got = run_nearest(api, query, target[perm], cells=(16, 16, 16))
    assert np.array_equal(bits(got[0]), bits(base[0]))
    unique = ~np.isin(base[1], np.arange(0, len(target), 50))          # cloud() repeats its first point at every 50th index: ties
    assert unique.sum() > 900 and np.array_equal(perm[got[1][unique]], base[1][unique])


def test_refusals_over_live_buffers_then_a_valid_call(api):
    lib = api[0].lib()
    query, target = dev(cloud(100, 1), F32), dev(cloud(200, 2), F32)
    d2 = torch.full((100,), -7.0, device="cuda")
    idx = torch.full((100,), -7, dtype=torch.int32, device="cuda")
    ws = workspace(lib.nrf_nearest_points_workspace_bytes(100, 200, 4, 4, 4), 0xA5)
    box = np.asarray(UNIT_BOX, F32)

    def call(nq=100, nt=200, b=box, cells=(4, 4, 4), md=INF, ws_bytes=None):
        return lib.nrf_nearest_points(p(query), nq, p(target), nt, b.ctypes.data_as(C.c_void_p), *cells, md, p(d2), p(idx), None, p(ws), ws.numel() if ws_bytes is None else ws_bytes,
                                      None)

    for kw, status in ((dict(nq=-1), INVALID_ARG), (dict(cells=(0, 4, 4)), INVALID_ARG), (dict(cells=(1025, 1, 1)), INVALID_ARG), (dict(md=-1.0), INVALID_ARG),
                       (dict(md=float("nan")), INVALID_ARG), (dict(b=np.array([0, 0, 0, 1, 0, 1], F32)), INVALID_ARG), (dict(ws_bytes=ws.numel() - 1), WORKSPACE)):
        assert call(**kw) == status, kw
    torch.cuda.synchronize()
    assert (d2 == -7).all() and (idx == -7).all() and (ws == 0xA5).all(), "a refusal writes nothing"
    assert call() == 0
    torch.cuda.synchronize()
    want = G.nearest(cloud(100, 1), cloud(200, 2))
    assert np.array_equal(bits(d2), bits(want[0])) and np.array_equal(idx.cpu().numpy(), want[1])
    # the sampling and statistics entries likewise
    verts, faces = sphere()
    dv, df = dev(verts, F32), dev(faces, np.int32)
    sws = workspace(lib.nrf_mesh_sample_workspace_bytes(len(verts), len(faces)), 0xA5)
    n, area = C.c_int64(-7), C.c_double(-7.0)
    count = lambda density, nbytes: lib.nrf_mesh_sample_count(p(dv), len(verts), p(df), len(faces), density, 0, C.addressof(n), C.addressof(area), None, p(sws), nbytes, None)
    assert count(-1.0, sws.numel()) == INVALID_ARG and count(1.0, sws.numel() - 1) == WORKSPACE and n.value == -7 and (sws == 0xA5).all()
    assert count(170.0, sws.numel()) == 0 and n.value == G.sample_count(verts, faces, 170.0, 0)["n_points"]
    out = torch.full((6,), -7.0, dtype=torch.float64, device="cuda")
    tws = workspace(lib.nrf_distance_stats_workspace_bytes(100), 0xA5)
    taus = np.array([0.1, 0.2], F32)
    stats = lambda n_tau, nbytes: lib.nrf_distance_stats(p(d2), 100, taus.ctypes.data_as(C.c_void_p), n_tau, p(out), p(tws), nbytes, None)
    assert stats(5, tws.numel()) == INVALID_ARG and stats(2, tws.numel() - 1) == WORKSPACE
    torch.cuda.synchronize()
    assert (out == -7).all() and (tws == 0xA5).all()
    assert stats(2, tws.numel()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits64(out), bits64(G.distance_stats(want[0], taus)))


# ------------------------------------------------------------------------------------ 3. statistics
@pytest.mark.parametrize("n", [0, 1, 4095, 4096, 4097, 20000])
def test_statistics_equal_the_restatement(api, n):
    lib = api[0].lib()
    rng = np.random.default_rng(n)
    d2 = (rng.uniform(0, 1, n).astype(F32)) ** 2
    if n > 1:
        d2[rng.integers(0, n, n // 10)] = np.inf
        d2[n // 2] = F32(0.25) * F32(0.25)          # sqrtf gives exactly 0.25: an entry at a tau
    taus = np.array([0.1, 0.25, 0.5, 2.0], F32)
    dd = dev(d2, F32) if n else None
    for n_tau in (0, 1, 4):
        for pattern in (None, 0xA5):
            out = torch.full((4 + n_tau,), -7.0, dtype=torch.float64, device="cuda")
            ws = workspace(lib.nrf_distance_stats_workspace_bytes(n), pattern)
            assert lib.nrf_distance_stats(p(dd), n, taus.ctypes.data_as(C.c_void_p), n_tau, p(out), p(ws), ws.numel(), None) == 0, lib.nrf_last_error()
            torch.cuda.synchronize()
            want = G.distance_stats(d2, taus[:n_tau])
            assert np.array_equal(bits64(out), bits64(want)), (n, n_tau, out.cpu().numpy(), want)
    if n > 1:
        assert want[0] == np.isfinite(d2).sum() < n and want[5] == (np.sqrt(d2) <= F32(0.25)).sum() and want[7] == want[0]


# ------------------------------------------------------------------------------------ 4. the Python layer
def make_mesh(api, verts, faces, **kw):
    v = dev(verts, F32)
    return api[2].Mesh(v, dev(faces, np.int32), torch.zeros_like(v), **kw)


def test_a_surface_is_at_distance_zero_from_itself(api):
    m = make_mesh(api, *sphere())
    r = api[1].SurfaceDistance(m, m, taus=(0.0, 0.01), n_points=3000, seed=5)
    for name in ("Accuracy", "Completeness", "Chamfer", "ChamferSq", "Hausdorff"):
        assert getattr(r, name).dtype == torch.float64 and getattr(r, name).is_cuda and float(getattr(r, name)) == 0.0, name
    assert r.Precision.tolist() == [1, 1] and r.Recall.tolist() == [1, 1] and r.FScore.tolist() == [1, 1]


def test_two_spheres_equal_the_restatement_composed_by_hand(api):
    n_points, seed = 2500, 2
    meshes, clouds = [], []
    for radius in (0.70, 0.75):
        verts, faces = sphere(radius)
        area = G.sample_count(verts, faces, 0.0, seed)["total_area"]
        clouds.append(G.sample(verts, faces, F32(n_points / area), seed)[1])
        meshes.append(make_mesh(api, verts, faces))
    # both meshes are sampled with one seed, so the pairs sit on one ray from the centre and every distance is close to 0.05: the middle tau, and the max_dist, is
    # the median distance of the restatement, which half of the points are within
    mid = float(np.median(np.sqrt(G.nearest(clouds[0], clouds[1])[0])))
    taus = (0.03, mid, 0.2)
    assert 0.049 < mid < 0.05
    for max_dist in (None, mid):
        want = G.surface_distance(clouds[0], clouds[1], taus, INF if max_dist is None else max_dist)
        got = api[1].SurfaceDistance(meshes[0], meshes[1], taus=taus, n_points=n_points, seed=seed, max_dist=max_dist, bbox=T.SPHERE["bbox"])
        for name, value in want.items():
            assert np.array_equal(bits64(getattr(got, name)), bits64(value)), (max_dist, name, getattr(got, name), value)
        assert 0.0385 < float(got.Accuracy) <= float(got.Hausdorff) < 0.12 and got.Precision.tolist()[0] == 0 and 0.3 < got.Recall.tolist()[1] < 0.7
        assert got.FScore.tolist()[2] == (1 if max_dist is None else got.FScore.tolist()[1])
    # point sets are taken as they are, and the grid's box may be left to the call
    pts = api[1].SurfaceDistance(dev(clouds[0], F32), dev(clouds[1], F32), taus=taus, max_dist=mid)
    for name, value in want.items():
        assert np.array_equal(bits64(getattr(pts, name)), bits64(value)), name


def test_sample_surface_and_interpolation(api):
    verts, faces = sphere()
    m = make_mesh(api, verts, faces, Colors=dev(verts, F32))
    for n_points in (1000, 20000):
        s = api[1].SampleSurface(m, n_points=n_points, seed=1)
        n = s.Points.shape[0]
        print(f"asked {n_points}, got {n}")
        assert abs(n - n_points) <= 4 * np.sqrt(n_points) and s.Faces.shape == (n,) and s.UV.shape == (n, 2) and s.Stats.tolist() == [0, 0, 0]
        area = G.sample_count(verts, faces, 0.0, 1)["total_area"]
        assert s.Area == area
        want = G.sample(verts, faces, F32(n_points / area), 1)
        assert np.array_equal(bits(s.Points), bits(want[1])) and np.array_equal(s.Faces.cpu().numpy(), want[2])
        # positions as an attribute interpolate to the points themselves
        c = api[1].InterpolateAttributes(m, s, "Colors")
        assert c.shape == (n, 3) and float((c - s.Points).abs().max()) < 1e-6
    by_density = api[1].SampleSurface(m, density=170.0, seed=4)
    assert np.array_equal(bits(by_density.Points), bits(sample_reference("sphere", 170.0, 4)["points"]))
    with pytest.raises(api[0].NrfError):
        api[1].SampleSurface(m)


def test_transfer_attributes_through_a_permutation(api):
    verts, faces = sphere()
    rng = np.random.default_rng(21)
    colors, relevancy = rng.uniform(0, 1, (len(verts), 3)).astype(F32), rng.uniform(0, 1, (len(verts), 2)).astype(F32)
    perm = rng.permutation(len(verts))
    inverse = np.argsort(perm)
    src = make_mesh(api, verts[perm], inverse[faces], Colors=dev(colors[perm], F32), Relevancy=dev(relevancy[perm], F32))
    dst = make_mesh(api, verts, faces)
    out = api[1].TransferAttributes(src, dst)
    assert out.Vertices is dst.Vertices and dst.Colors is None
    assert np.array_equal(bits(out.Colors), bits(colors)) and np.array_equal(bits(out.Relevancy), bits(relevancy))
    d2, idx = api[1].NearestPoints(dst.Vertices, src.Vertices)
    assert (d2 == 0).all() and np.array_equal(idx.cpu().numpy(), inverse)
    far = api[1].TransferAttributes(src, make_mesh(api, verts + F32(5), faces), names=("Colors",), max_dist=0.5)
    assert (far.Colors == 0).all() and far.Relevancy is None
