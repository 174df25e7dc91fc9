"""The point-cloud tools on the MI355X, every comparison an integer / bit equality unless stated: the buffer nrf_point_bvh_build writes against the restated tree
(tests/points_ref.py over tests/bvh_ref.py) and, past its first word, against nrf_mesh_bvh_build on the faces (i, i, i); nrf_bvh_knn against the brute-force sorted
keys at every k, size, option and order, and at k = 1 against nrf_nearest_points itself; normals, eigenvalues, scores, statistics and the plane sums from given
normals against their restatements; the Python layer; and the refusals over live buffers."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import align_ref as A
import bvh_ref as B
import geometry_ref as G
import points_ref as P

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
INVALID_ARG, WORKSPACE = 1, 4
INF = float("inf")
CLOUDS = ["rand0", "rand1", "rand2", "rand3", "rand255", "rand256", "rand257", "ico642", "copies300", "flat", "lattice", "mixed", "nonfinite_only"]
KS = [1, 2, 7, 8, 9, 31, 32]


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from nerfpp_amd import _lib as L, geometry, points, align
    return L, geometry, points, align


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, F32).view(np.uint32)


def dev(a, dtype):
    return torch.from_numpy(np.array(a, dtype, order="C")).cuda()          # a copy: the shared clouds are read-only


def p(t):
    return None if t is None else t.data_ptr()


def buffer(nbytes, pattern):
    ws = torch.empty((max(1, int(nbytes)),), dtype=torch.uint8, device="cuda")
    ws.fill_(pattern)
    return ws


# ------------------------------------------------------------------------------------ 1. the build
def build_pbvh(api, pts, pattern=0xA5, stats=None):
    """nrf_point_bvh_build over a poisoned buffer and workspace; the workspace is overwritten afterwards -> dict(dp, n, bvh): what a query takes"""
    lib = api[0].lib()
    pts = np.asarray(pts, F32).reshape(-1, 3)
    g = dict(dp=dev(pts, F32) if len(pts) else None, n=len(pts), bvh=buffer(lib.nrf_point_bvh_bytes(len(pts)), pattern))
    assert g["bvh"].numel() == lib.nrf_point_bvh_bytes(len(pts)) == B.layout(len(pts))[2]
    ws = buffer(lib.nrf_point_bvh_workspace_bytes(len(pts)), pattern)
    status = lib.nrf_point_bvh_build(p(g["dp"]), g["n"], p(g["bvh"]), g["bvh"].numel(), p(stats), p(ws), ws.numel(), None)
    assert status == 0, lib.nrf_last_error()
    ws.fill_(pattern ^ 0xFF)          # the workspace may go after the build
    return g


@functools.lru_cache(maxsize=None)
def built(name):
    """One build per cloud for the query tests (the api fixture has checked the device)"""
    from nerfpp_amd import _lib as L, geometry, points, align
    return build_pbvh((L, geometry, points, align), P.clouds()[name])


@pytest.mark.parametrize("name", CLOUDS)
def test_the_built_buffer_is_the_restated_tree_and_the_mesh_build_of_the_faces_iii(api, name):
    lib = api[0].lib()
    pts = P.clouds()[name]
    n = len(pts)
    want = P.build(pts)
    stats = torch.zeros((4,), dtype=torch.int32, device="cuda")
    g = build_pbvh(api, pts, 0xA5, stats)
    torch.cuda.synchronize()
    raw = g["bvh"].cpu().numpy()
    got = B.parse(raw, n)
    assert got["head"][0] == P.MAGIC
    got["head"][0] = B.MAGIC          # the rest is the mesh tree's, word for word
    assert B.same_tree(got, want) == [], name
    assert B.check_invariants(got, pts, P.faces_iii(n)) == want["height"]
    assert np.array_equal(stats.cpu().numpy().view(np.uint32), want["stats"]) and want["stats"][1] == 0
    again = build_pbvh(api, pts, 0x3C)
    torch.cuda.synchronize()
    assert np.array_equal(again["bvh"].cpu().numpy(), raw), "two builds over differently poisoned buffers: the same bytes"
    df = dev(P.faces_iii(n), np.int32) if n else None
    mesh = buffer(lib.nrf_mesh_bvh_bytes(n), 0x5A)
    ws = buffer(lib.nrf_mesh_bvh_workspace_bytes(n), 0x5A)
    assert lib.nrf_mesh_bvh_build(p(g["dp"]), n, p(df), n, p(mesh), mesh.numel(), None, p(ws), ws.numel(), None) == 0, lib.nrf_last_error()
    torch.cuda.synchronize()
    m = mesh.cpu().numpy()
    assert m[:8].view(np.int64)[0] == B.MAGIC and np.array_equal(m[8:], raw[8:]), "beyond the first word: nrf_mesh_bvh_build on the same arrays"


# ------------------------------------------------------------------------------------ 2. k nearest
def knn_gpu(api, g, query, k, max_dist=INF, exclude_self=False, order=None, stats=None, count=True):
    lib = api[0].lib()
    q = np.asarray(query, F32).reshape(-1, 3)
    nq = len(q)
    dq = dev(q, F32) if nq else None
    d2 = torch.full((nq, k), -7.0, device="cuda")          # pattern-filled: an unwritten slot shows
    idx = torch.full((nq, k), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((nq,), -7, dtype=torch.int32, device="cuda") if count else None
    do = None if order is None else dev(order, np.int32)
    status = lib.nrf_bvh_knn(p(dq), nq, p(g["dp"]), g["n"], p(g["bvh"]), g["bvh"].numel(), p(do), k, max_dist, int(exclude_self), p(d2) if nq else None,
                             p(idx) if nq else None, p(cnt) if nq else None, p(stats), None, 0, None)
    assert status == 0, lib.nrf_last_error()
    torch.cuda.synchronize()
    return dict(d2=d2.cpu().numpy(), index=idx.cpu().numpy(), count=None if cnt is None else cnt.cpu().numpy())


def same_knn(got, want, what):
    assert np.array_equal(bits(got["d2"]), bits(want["d2"])), f"{what}: d2 differs in rows {np.unique(np.nonzero(bits(got['d2']) != bits(want['d2']))[0])[:5]}"
    assert np.array_equal(got["index"], want["index"]), f"{what}: index differs in rows {np.unique(np.nonzero(got['index'] != want['index'])[0])[:5]}"
    if got["count"] is not None:
        assert np.array_equal(got["count"], want["count"]), f"{what}: count"


def morton_order(api, g, q):
    lib = api[0].lib()
    dq = dev(q, F32)
    codes = torch.full((len(q),), -7, dtype=torch.int32, device="cuda")
    assert lib.nrf_point_bvh_codes(p(dq), len(q), 3, p(g["bvh"]), g["bvh"].numel(), g["n"], p(codes), None) == 0, lib.nrf_last_error()
    torch.cuda.synchronize()
    return codes.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", CLOUDS)
def test_knn_is_the_brute_force_sorted_keys(api, name):
    pts = P.clouds()[name]
    g = built(name)
    q = P.queries(pts, seed=len(pts) + 1, n=257)
    codes = morton_order(api, g, q)
    tree = P.build(pts)
    with np.errstate(all="ignore"):
        assert np.array_equal(codes, B.morton(q, tree["lo"], tree["hi"])), "nrf_point_bvh_codes: the mesh query's codes against the cloud's box"
    orders = {"identity": None, "reversed": np.arange(len(q))[::-1], "morton": np.argsort(codes, kind="stable")}
    diag = 1.0 if not tree["n_valid"] else float(np.linalg.norm(tree["hi"].astype(F64) - tree["lo"].astype(F64)))
    for k in KS:
        for max_dist, exclude in ((INF, False), (0.3 * diag + 0.05, False), (0.0, False), (INF, True), (0.2 * diag + 0.05, True)):
            want = P.knn(q, pts, k, max_dist, exclude)
            for oname, order in orders.items():
                if oname != "identity" and k not in (1, 8, 32):
                    continue
                stats = torch.zeros((4,), dtype=torch.int32, device="cuda")
                got = knn_gpu(api, g, q, k, max_dist, exclude, order, stats)
                same_knn(got, want, f"{name} k={k} max_dist={max_dist} exclude={exclude} {oname}")
                assert stats.cpu().numpy().tolist() == [want["stats0"], 0, 0, 0]
    # the cloud against itself, the case of the normals: exact ties among the copies and on the lattice
    if len(pts):
        for k in (8, 9):
            same_knn(knn_gpu(api, g, pts, k, INF, True), P.knn(pts, pts, k, exclude_self=True), f"{name} self k={k}")


@pytest.mark.parametrize("nq", [0, 1, 63, 64, 65, 257])
def test_knn_at_every_query_count(api, nq):
    pts = P.clouds()["ico642"]
    q = P.queries(pts, seed=nq, n=max(nq, 16))[-nq:] if nq else np.zeros((0, 3), F32)          # the far and non-finite rows first to go in
    for k in (1, 8, 16, 17):
        same_knn(knn_gpu(api, built("ico642"), q, k), P.knn(q, pts, k), f"nq={nq} k={k}")
        same_knn(knn_gpu(api, built("ico642"), q, k, count=False), dict(P.knn(q, pts, k), count=None), f"nq={nq} k={k} without d_count")


@pytest.mark.parametrize("k", KS)
def test_knn_on_targets_around_k_points(api, k):
    rng = np.random.default_rng(k)
    q = rng.uniform(-1, 1, (65, 3)).astype(F32)
    for n in sorted({0, 1, max(k - 1, 0), k, k + 1}):
        pts = rng.uniform(-1, 1, (n, 3)).astype(F32)
        g = build_pbvh(api, pts)
        for exclude in (False, True):
            same_knn(knn_gpu(api, g, q, k, INF, exclude), P.knn(q, pts, k, INF, exclude), f"n={n} k={k} exclude={exclude}")


def nearest_grid(api, q, pts, max_dist):
    """nrf_nearest_points itself, over the box of the finite targets"""
    lib = api[0].lib()
    fin = pts[np.isfinite(pts).all(-1)]
    box = np.concatenate([fin.min(0) - 0.01, fin.max(0) + 0.01]).astype(F32) if len(fin) else np.array([0, 0, 0, 1, 1, 1], F32)
    dq, dt = dev(q, F32), (dev(pts, F32) if len(pts) else None)
    d2 = torch.full((len(q),), -7.0, device="cuda")
    idx = torch.full((len(q),), -7, dtype=torch.int32, device="cuda")
    ws = buffer(lib.nrf_nearest_points_workspace_bytes(len(q), len(pts), 4, 4, 4), 0xA5)
    status = lib.nrf_nearest_points(p(dq), len(q), p(dt), len(pts), box.ctypes.data_as(C.c_void_p), 4, 4, 4, max_dist, p(d2), p(idx), None, p(ws), ws.numel(), None)
    assert status == 0, lib.nrf_last_error()
    torch.cuda.synchronize()
    return d2.cpu().numpy(), idx.cpu().numpy()


@pytest.mark.parametrize("name", ["rand1", "rand257", "ico642", "copies300", "flat", "lattice", "mixed", "nonfinite_only"])
def test_k_1_is_nrf_nearest_points_bit_for_bit(api, name):
    pts = P.clouds()[name]
    q = np.concatenate([P.queries(pts, seed=5, n=257), np.array([[3e19, 0, 0], [3.0e38, -3.0e38, 3.0e38]], F32)])          # d2 overflows to +inf
    for max_dist in (INF, 0.25, 0.0):
        d2, idx = nearest_grid(api, q, pts, max_dist)
        got = knn_gpu(api, built(name), q, 1, max_dist)
        assert np.array_equal(bits(got["d2"][:, 0]), bits(d2)) and np.array_equal(got["index"][:, 0], idx), (name, max_dist)
        ref = G.nearest(q, pts, max_dist)
        assert np.array_equal(bits(d2), bits(ref[0])) and np.array_equal(idx, ref[1])


# ------------------------------------------------------------------------------------ 3. normals, scores, statistics, sums
def normals_gpu(api, pts, index, toward=None, stride=0, eigen=True, stats=None):
    lib = api[0].lib()
    n, k = index.shape
    dp, di = dev(pts, F32), dev(index, np.int32)
    dt = None if toward is None else dev(toward, F32)
    out_n = torch.full((n, 3), -7.0, device="cuda")
    out_e = torch.full((n, 3), -7.0, device="cuda") if eigen else None
    status = lib.nrf_points_normals(p(dp), n, p(di), k, p(dt), stride, p(out_n), p(out_e), p(stats), None)
    assert status == 0, lib.nrf_last_error()
    torch.cuda.synchronize()
    return out_n.cpu().numpy(), None if out_e is None else out_e.cpu().numpy()


@pytest.mark.parametrize("name", ["rand3", "rand255", "rand257", "ico642", "copies300", "flat", "lattice", "mixed"])
def test_normals_and_eigenvalues_equal_the_restatement(api, name):
    pts = P.clouds()[name]
    rng = np.random.default_rng(3)
    for k in (2, 8, 16):
        index = knn_gpu(api, built(name), pts, k, INF, True)["index"]
        per_point = rng.uniform(-2, 2, (len(pts), 3)).astype(F32)
        for toward, stride in ((None, 0), (np.array([0.3, 2.0, -1.0], F32), 0), (per_point, 3)):
            want = P.normals(pts, index, toward, stride)
            stats = torch.zeros((1,), dtype=torch.int32, device="cuda")
            n, e = normals_gpu(api, pts, index, toward, stride, stats=stats)
            assert np.array_equal(bits(n), bits(want["normals"])), f"{name} k={k} stride={stride}: normals differ at {np.unique(np.nonzero(bits(n) != bits(want['normals']))[0])[:5]}"
            assert np.array_equal(bits(e), bits(want["eigen"])), f"{name} k={k}: eigenvalues"
            assert int(stats.cpu()[0]) == want["stats0"]
        assert np.array_equal(bits(normals_gpu(api, pts, index, eigen=False)[0]), bits(P.normals(pts, index)["normals"])), "without d_eigen"


def test_normals_exact_and_degenerate_cases(api):
    layer = P.lattice(6)[P.lattice(6)[:, 2] == 0]
    g = build_pbvh(api, layer)
    index = knn_gpu(api, g, layer, 8, INF, True)["index"]
    n, e = normals_gpu(api, layer, index)
    assert (n == np.array([0, 0, 1], F32)).all() and (e[:, 0] == 0).all(), "the lattice's face layer: exactly (0, 0, 1) by the sign rule"
    n, _ = normals_gpu(api, layer, index, np.array([2.5, 2.5, -4], F32), 0)
    assert (n == np.array([0, 0, -1], F32)).all(), "and (0, 0, -1) toward a viewpoint below"
    line = np.stack([np.arange(10, dtype=F32), np.zeros(10, F32), np.zeros(10, F32)], -1)
    same = P.clouds()["copies300"][:20]
    two = P.clouds()["rand2"]
    for pts, k in ((line, 4), (same, 8), (two, 8)):
        index = knn_gpu(api, build_pbvh(api, pts), pts, k, INF, True)["index"]
        stats = torch.zeros((1,), dtype=torch.int32, device="cuda")
        n, e = normals_gpu(api, pts, index, stats=stats)
        assert not n.any() and not e.any() and int(stats.cpu()[0]) == len(pts), "collinear, coincident and m < 3 sets are flagged"


@pytest.mark.parametrize("k", [8, 16])
def test_the_icosphere_normals_are_as_accurate_as_on_the_cpu(api, k):
    """The largest angle to the analytic normal is the CPU restatement's (3.3381 degrees at k = 8, 1.6881 at k = 16: DESIGN 8u): the device equals it bit for bit"""
    pts = P.clouds()["ico642"]
    centre = np.array([0.1, -0.15, 0.2], F32)
    index = P.knn(pts, pts, k, exclude_self=True)["index"]
    want = P.normals(pts, index, centre)["normals"]
    got, _ = normals_gpu(api, pts, index, centre, 0)

    def worst(n):
        inward = centre.astype(F64) - pts.astype(F64)
        inward /= np.linalg.norm(inward, axis=1, keepdims=True)
        return float(np.degrees(np.arccos(np.clip((n.astype(F64) * inward).sum(1), -1, 1))).max())
    print(f"icosphere normals k={k}: device {worst(got):.4f} degrees, CPU {worst(want):.4f} degrees")
    assert np.array_equal(bits(got), bits(want)) and worst(got) <= worst(want)


@pytest.mark.parametrize("n", [0, 1, 255, 4096, 4097, 10001])
def test_scores_and_value_stats_equal_the_restatement(api, n):
    lib = api[0].lib()
    rng = np.random.default_rng(n)
    for k in (1, 5, 32):
        d2 = rng.uniform(0, 4, (n, k)).astype(F32)
        d2 = np.sort(d2, axis=1)
        cut = rng.integers(0, k + 1, n)
        d2[np.arange(k)[None] >= cut[:, None]] = np.inf          # rows with 0 .. k filled slots
        dd = dev(d2, F32) if n else None
        score = torch.full((n,), -7.0, device="cuda")
        assert lib.nrf_knn_mean_distance(p(dd), n, k, p(score) if n else None, None) == 0, lib.nrf_last_error()
        torch.cuda.synchronize()
        want = P.mean_distance(d2) if n else np.zeros(0, F32)
        assert np.array_equal(bits(score), bits(want)), (n, k)
        out = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
        ws = buffer(lib.nrf_value_stats_workspace_bytes(n), 0xA5)
        assert lib.nrf_value_stats(p(score) if n else None, n, p(out), p(ws), ws.numel(), None) == 0, lib.nrf_last_error()
        torch.cuda.synchronize()
        assert np.array_equal(A.bits64(out.cpu().numpy()), A.bits64(P.value_stats(want))), (n, k)


@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 3000])
def test_plane_sums_from_given_normals_equal_the_restatement_and_ignore_the_sign(api, n):
    lib = api[0].lib()
    rng = np.random.default_rng(n + 1)
    y, pp = rng.uniform(-1, 1, (n, 3)).astype(F32), rng.uniform(-1, 1, (n, 3)).astype(F32)
    nrm = rng.normal(size=(n, 3)).astype(F32)
    index = rng.integers(-1, 50, n).astype(np.int32)
    if n >= 1000:
        nrm[7], nrm[8, 1], y[9, 0], nrm[10, 2], pp[11, 1] = 0, np.nan, np.inf, np.inf, np.nan
    flipped = np.where(rng.integers(0, 2, (n, 1)) == 1, -nrm, nrm).astype(F32)
    want, wstats = P.sums_normals(y, pp, nrm, index)
    outs = []
    for normal in (nrm, flipped):
        ws = buffer(lib.nrf_align_workspace_bytes(n, A.PLANE), 0xA5)
        stats = torch.zeros((4,), dtype=torch.int32, device="cuda")
        dy = dp_ = dn = di = None
        if n:
            dy, dp_, dn, di = dev(y, F32), dev(pp, F32), dev(normal, F32), dev(index, np.int32)
        assert lib.nrf_align_sums_normals(p(dy), p(dp_), p(dn), p(di), n, p(stats), p(ws), ws.numel(), None) == 0, lib.nrf_last_error()
        torch.cuda.synchronize()
        part = ws[:want.size * 8].cpu().numpy().view(F64).reshape(want.shape)
        assert np.array_equal(A.bits64(part), A.bits64(want)), n
        assert np.array_equal(stats.cpu().numpy().view(np.uint32), wstats)
        outs.append(part)
    assert np.array_equal(A.bits64(outs[0]), A.bits64(outs[1])), "the sign of a normal changes no column"


# ------------------------------------------------------------------------------------ 4. the Python layer
def test_nearest_points_through_a_point_bvh_equals_the_grid(api):
    _, geometry, points, _ = api
    pts = P.clouds()["mixed"]
    q = P.queries(pts, seed=9, n=300)
    t, dq = dev(pts, F32), dev(q, F32)
    bvh = points.PointBVH(t)
    assert np.array_equal(bits(bvh.Box), bits(np.concatenate([P.build(pts)["lo"], P.build(pts)["hi"]])))
    for max_dist in (None, 0.3):
        stats = torch.zeros((3,), dtype=torch.int32, device="cuda")
        d2, idx = geometry.NearestPoints(dq, bvh, max_dist=max_dist, stats=stats)
        gd2, gidx = geometry.NearestPoints(dq, t, max_dist=max_dist)
        assert d2.shape == gd2.shape and np.array_equal(bits(d2), bits(gd2)) and np.array_equal(idx.cpu().numpy(), gidx.cpu().numpy())
        assert stats.cpu().numpy().tolist() == [int((~np.isfinite(q).all(-1)).sum()), 0, 0], "entry 2 untouched: there is no fallback"
    r = points.KNearest(dq, bvh, 9, max_dist=0.5, coherent=True)
    want = P.knn(q, pts, 9, 0.5)
    same_knn(dict(d2=r.Dist2.cpu().numpy(), index=r.Index.cpu().numpy(), count=r.Count.cpu().numpy()), want, "KNearest, coherent")
    keep = points.RadiusOutliers(t, 0.4, 3, bvh=bvh)
    assert np.array_equal(keep.cpu().numpy(), P.knn(pts, pts, 3, 0.4, True)["count"] >= 3)
    with pytest.raises(api[0].NrfError):
        points.KNearest(dq, bvh, 33)


def test_estimate_normals_and_surface_variation(api):
    points = api[2]
    pts = P.clouds()["ico642"]
    centre = np.array([0.1, -0.15, 0.2], F32)
    r = points.EstimateNormals(dev(pts, F32), k=16, toward=dev(centre, F32))
    want = P.normals(pts, P.knn(pts, pts, 16, exclude_self=True)["index"], centre)
    assert np.array_equal(bits(r.Normals), bits(want["normals"])) and np.array_equal(bits(r.Eigenvalues), bits(want["eigen"])) and r.Valid.all()
    sv = points.SurfaceVariation(r).cpu().numpy()
    e = want["eigen"]
    assert np.allclose(sv, e[:, 0] / (e[:, 0] + e[:, 1] + e[:, 2]), rtol=1e-6, atol=0) and sv.max() < 1.0 / 3.0          # a torch one-liner over the eigenvalues


def test_statistical_outliers_remove_exactly_the_planted_points(api):
    """642 sphere points and 20 points planted 4 to 6 units away: on the restatement (tests/test_points_host.py) the sphere's scores stay below half the threshold
    mean + 2 std and the planted ones above twice it, so the mask is exactly the planting"""
    import test_points_host as H
    points = api[2]
    pts, planted = H.outlier_case()
    keep, scores = points.StatisticalOutliers(dev(pts, F32), k=16, ratio=2.0)
    want = P.mean_distance(P.knn(pts, pts, 16, exclude_self=True)["d2"])
    assert np.array_equal(bits(scores), bits(want))
    assert np.array_equal(keep.cpu().numpy(), want.astype(F64) <= P.outlier_threshold(want, 2.0))
    assert keep[:642].all() and not keep[642:].any() and int((~keep).sum()) == planted


@functools.lru_cache(maxsize=None)
def icp_case():
    c = A.ellipsoid_case()
    c["src"] = A.surface_samples(*c["source"])
    c["cloud"] = A.surface_samples(*c["target"], seed=1)
    return c


def test_register_icp_plane_mode_against_a_cloud(api):
    L, geometry, points, align = api
    c = icp_case()
    src, cloud = dev(c["src"], F32), dev(c["cloud"], F32)
    iterations = 8
    with pytest.raises(L.NrfError, match="needs the faces"):
        align.RegisterICP(src, cloud, iterations=2, method="plane")
    with pytest.raises(L.NrfError):
        align.RegisterICP(src, cloud, iterations=2, method="point", target_normals="estimate")
    runs = [align.RegisterICP(src, cloud, iterations=iterations, method="plane", scale=True, target_normals="estimate") for _ in range(2)]
    torch.cuda.synchronize()
    state, history = runs[0].Transform.State.cpu().numpy(), runs[0].History.cpu().numpy()
    assert np.array_equal(A.bits64(state), A.bits64(runs[1].Transform.State.cpu().numpy())) and np.array_equal(A.bits64(history), A.bits64(runs[1].History.cpu().numpy()))
    # the same calls composed by hand
    lib = L.lib()
    bvh = points.PointBVH(cloud)
    normals = points.EstimateNormals(cloud, bvh=bvh).Normals
    given = align.RegisterICP(src, cloud, iterations=iterations, method="plane", scale=True, target_normals=normals)
    t = align.Transform(device="cuda")
    hist = torch.zeros((iterations, 8), dtype=torch.float64, device="cuda")
    ws = buffer(lib.nrf_align_workspace_bytes(len(c["src"]), A.PLANE), 0xA5)
    n = len(c["src"])
    for it in range(iterations):
        y = t.Apply(src)
        idx = points.KNearest(y, bvh, 1).Index.reshape(-1).contiguous()
        at = idx.clamp(min=0).to(torch.int64)
        pp, nn = cloud[at].contiguous(), normals[at].contiguous()
        assert lib.nrf_align_sums_normals(p(y), p(pp), p(nn), p(idx), n, None, p(ws), ws.numel(), None) == 0, lib.nrf_last_error()
        assert lib.nrf_align_solve(n, A.PLANE, 1, it, iterations, p(t.State), p(hist), p(ws), ws.numel(), None) == 0, lib.nrf_last_error()
    torch.cuda.synchronize()
    for r in (runs[0], given):
        assert np.array_equal(A.bits64(r.Transform.State.cpu().numpy()), A.bits64(t.State.cpu().numpy())), "the state equals the hand composition"
        assert np.array_equal(A.bits64(r.History.cpu().numpy()), A.bits64(hist.cpu().numpy()))
    assert (history[:, align.H_FLAG] == 0).all() and (history[:, align.H_PAIRS] > 0.99 * n).all()
    point = align.RegisterICP(src, cloud, iterations=iterations, method="point", scale=True)
    e_plane = A.pose_error(list(state), c)
    e_point = A.pose_error(list(point.Transform.State.cpu().numpy()), c)
    print("ICP against a cloud after %d iterations: plane (estimated normals) %.3e deg, scale %.3e, shift %.3e; point %.3e deg, scale %.3e, shift %.3e" % ((iterations,) + e_plane + e_point))
    assert e_plane[0] < e_point[0], "plane mode is nearer the true rotation than point mode at the same iteration count"


# ------------------------------------------------------------------------------------ 5. refusals
def test_refusals_come_before_any_write(api):
    lib = api[0].lib()
    pts = P.clouds()["rand257"]
    n, k, nq = len(pts), 8, 65
    g = build_pbvh(api, pts)
    q = dev(P.queries(pts, seed=1, n=nq), F32)
    d2 = torch.full((nq + 1, k), -7.0, device="cuda")
    idx = torch.full((nq + 1, k), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((nq + 1,), -7, dtype=torch.int32, device="cuda")
    stats = torch.zeros((4,), dtype=torch.int32, device="cuda")
    df = dev(P.faces_iii(n), np.int32)
    mesh = buffer(lib.nrf_mesh_bvh_bytes(n), 0)
    mws = buffer(lib.nrf_mesh_bvh_workspace_bytes(n), 0)
    assert lib.nrf_mesh_bvh_build(p(g["dp"]), n, p(df), n, p(mesh), mesh.numel(), None, p(mws), mws.numel(), None) == 0

    def knn(**kw):
        a = dict(q=p(q), nq=nq, pts=p(g["dp"]), n=n, bvh=p(g["bvh"]), bytes=g["bvh"].numel(), order=None, k=k, max_dist=INF, excl=0, d2=p(d2), idx=p(idx), cnt=p(cnt))
        a.update(kw)
        return lib.nrf_bvh_knn(a["q"], a["nq"], a["pts"], a["n"], a["bvh"], a["bytes"], a["order"], a["k"], a["max_dist"], a["excl"], a["d2"], a["idx"], a["cnt"],
                               p(stats), None, 0, None)

    def untouched():
        torch.cuda.synchronize()
        return bool((d2 == -7).all()) and bool((idx == -7).all()) and bool((cnt == -7).all()) and not stats.any()

    refused = [dict(k=0), dict(k=33), dict(k=-1), dict(nq=-1), dict(n=-1), dict(bytes=g["bvh"].numel() - 64), dict(n=n - 1), dict(bvh=None), dict(bvh=p(g["bvh"]) + 4),
               dict(q=None), dict(d2=None), dict(idx=None), dict(pts=None), dict(q=p(q) + 2), dict(d2=p(d2) + 2), dict(idx=p(idx) + 1), dict(cnt=p(cnt) + 2),
               dict(max_dist=-1.0), dict(max_dist=float("nan")), dict(excl=2)]
    for kw in refused:
        assert knn(**kw) == INVALID_ARG, kw
        assert untouched(), kw
        assert knn() == 0, lib.nrf_last_error()          # a valid call follows each refusal
        torch.cuda.synchronize()
        assert bool((d2[:nq] != -7).all()) and bool((d2[nq] == -7).all())
        d2.fill_(-7.0), idx.fill_(-7), cnt.fill_(-7), stats.zero_()
    # a mesh BVH handed to the point query: the size passes, the magic does not -- nothing is written; and the reverse
    assert knn(bvh=p(mesh), bytes=mesh.numel()) == 0 and untouched(), "a mesh buffer is read no further than its head"
    cd2 = torch.full((nq,), -7.0, device="cuda")
    cface = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
    assert lib.nrf_bvh_closest_on_mesh(p(q), nq, p(g["dp"]), n, p(df), n, p(g["bvh"]), g["bvh"].numel(), None, INF, p(cd2), p(cface), None, None, None, None, 0, None) == 0
    torch.cuda.synchronize()
    assert bool((cd2 == -7).all()) and bool((cface == -7).all()), "a point buffer handed to the mesh query"
    assert lib.nrf_bvh_closest_on_mesh(p(q), nq, p(g["dp"]), n, p(df), n, p(mesh), mesh.numel(), None, INF, p(cd2), p(cface), None, None, None, None, 0, None) == 0
    torch.cuda.synchronize()
    assert bool((cd2 != -7).all())
    # the build
    bvh = buffer(lib.nrf_point_bvh_bytes(n), 0xA5)
    ws = buffer(lib.nrf_point_bvh_workspace_bytes(n), 0xA5)

    def build(**kw):
        a = dict(pts=p(g["dp"]), n=n, bvh=p(bvh), bytes=bvh.numel(), ws=p(ws), wsb=ws.numel())
        a.update(kw)
        return lib.nrf_point_bvh_build(a["pts"], a["n"], a["bvh"], a["bytes"], None, a["ws"], a["wsb"], None)
    for kw, code in ((dict(n=-1), INVALID_ARG), (dict(n=1 << 31), INVALID_ARG), (dict(pts=None), INVALID_ARG), (dict(pts=p(g["dp"]) + 2), INVALID_ARG),
                     (dict(bvh=None), INVALID_ARG), (dict(bvh=p(bvh) + 32), INVALID_ARG), (dict(bytes=bvh.numel() + 64), INVALID_ARG), (dict(ws=None), INVALID_ARG),
                     (dict(ws=p(ws) + 4), INVALID_ARG), (dict(wsb=ws.numel() - 1), WORKSPACE)):
        assert build(**kw) == code, kw
        torch.cuda.synchronize()
        assert bool((bvh == 0xA5).all()) and bool((ws == 0xA5).all()), kw
    assert build() == 0
    torch.cuda.synchronize()
    assert np.array_equal(bvh.cpu().numpy(), g["bvh"].cpu().numpy())
    # normals, scores, statistics, sums
    index = torch.full((n, k), -1, dtype=torch.int32, device="cuda")
    nrm = torch.full((n, 3), -7.0, device="cuda")
    for args in ((p(g["dp"]), n, p(index), 0, None, 0, p(nrm), None, None, None), (p(g["dp"]), n, p(index), 33, None, 0, p(nrm), None, None, None),
                 (p(g["dp"]), n, p(index), k, None, 1, p(nrm), None, None, None), (p(g["dp"]), n, None, k, None, 0, p(nrm), None, None, None),
                 (p(g["dp"]), n, p(index), k, None, 0, None, None, None, None), (p(g["dp"]), n, p(index), k, None, 0, p(nrm) + 2, None, None, None),
                 (p(g["dp"]), -1, p(index), k, None, 0, p(nrm), None, None, None)):
        assert lib.nrf_points_normals(*args) == INVALID_ARG, args
    score = torch.full((n,), -7.0, device="cuda")
    assert lib.nrf_knn_mean_distance(p(d2), nq, 0, p(score), None) == INVALID_ARG and lib.nrf_knn_mean_distance(None, nq, k, p(score), None) == INVALID_ARG
    out = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
    sws = buffer(lib.nrf_value_stats_workspace_bytes(n), 0xA5)
    assert lib.nrf_value_stats(p(score), n, None, p(sws), sws.numel(), None) == INVALID_ARG
    assert lib.nrf_value_stats(p(score), n, p(out), None, sws.numel(), None) == INVALID_ARG
    assert lib.nrf_value_stats(p(score), n, p(out), p(sws), sws.numel() - 8, None) == WORKSPACE
    aws = buffer(lib.nrf_align_workspace_bytes(n, A.PLANE), 0xA5)
    assert lib.nrf_align_sums_normals(p(g["dp"]), p(g["dp"]), None, p(index), n, None, p(aws), aws.numel(), None) == INVALID_ARG
    assert lib.nrf_align_sums_normals(p(g["dp"]), p(g["dp"]), p(nrm), p(index), n, None, p(aws), aws.numel() - 8, None) == WORKSPACE
    torch.cuda.synchronize()
    assert bool((nrm == -7).all()) and bool((score == -7).all()) and bool((out == -7).all()) and bool((aws == 0xA5).all()) and bool((sws == 0xA5).all())
    assert lib.nrf_points_normals(p(g["dp"]), n, p(index), k, None, 0, p(nrm), None, None, None) == 0 and lib.nrf_value_stats(p(score), n, p(out), p(sws), sws.numel(), None) == 0
    torch.cuda.synchronize()
    assert not nrm.any(), "no neighbours: every set is degenerate"
