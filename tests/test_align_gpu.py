"""Registration on the MI355X: nrf_align_state_init, nrf_align_apply, nrf_align_sums and nrf_align_solve against the numpy restatement (tests/align_ref.py) with
uint32 / uint64 equality -- every size at which a kernel takes another path, every class of dropped pair, the permutations the order of a sum allows and those it
does not, every degenerate flag --, the composed iterations, the run-to-run guarantee, the refusals over live buffers, and the Python layer built on them:
Transform, TransformMesh, AlignPoints, RegisterICP and SurfaceDistance(align=).  No input here is outside the contract: bad indices and non-finite values have a
defined answer and are rejected before any dereference."""
import ctypes as C

import numpy as np
import pytest
import torch

import align_ref as A
import geometry_ref as G

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
INVALID_ARG, WORKSPACE = 1, 4
POSE = [0.3, -0.5, 0.7, 0.2, 1.7, 0.5, -2.0, 3.0]


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from nerfpp_amd import _lib as L, geometry, mesh, align
    return L, geometry, mesh, align


@pytest.fixture(scope="module")
def case():
    c = A.ellipsoid_case()
    c["src"] = A.surface_samples(*c["source"])
    return c


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, F32).view(np.uint32)


def bits64(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, F64).view(np.uint64)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def p(t):
    return t if t is None or isinstance(t, int) else t.data_ptr()


def buffer(nbytes, pattern=0x5A):
    return torch.full((max(1, int(nbytes)),), pattern, dtype=torch.uint8, device="cuda")


def make_mesh(api, verts, faces, **kw):
    v = dev(verts, F32)
    return api[2].Mesh(v, dev(faces, np.int32), torch.zeros_like(v), **kw)


def device_state(api, pose=None):
    st = torch.full((8,), -7.0, dtype=torch.float64, device="cuda")
    arr = None if pose is None else (C.c_double * 8)(*pose)
    assert api[0].lib().nrf_align_state_init(None if arr is None else C.addressof(arr), p(st), None) == 0
    return st


def run_sums(api, y, pp, face, mode, verts=None, faces=None, stats=True):
    """nrf_align_sums -> (partials [blocks, NV] float64, stats [4], workspace)"""
    lib = api[0].lib()
    n = len(face)
    dy, dp, df = (dev(y, F32), dev(pp, F32), dev(face, np.int32)) if n else (None, None, None)
    dv, dfc = (None, None) if verts is None else (dev(np.asarray(verts, F32).reshape(-1, 3), F32), dev(np.asarray(faces, np.int32).reshape(-1, 3), np.int32))
    st = torch.zeros((4,), dtype=torch.int32, device="cuda") if stats else None
    ws = buffer(lib.nrf_align_workspace_bytes(n, mode))
    assert lib.nrf_align_sums(p(dy), p(dp), p(df), n, mode, p(dv), 0 if verts is None else len(dv), p(dfc), 0 if verts is None else len(dfc), p(st), p(ws), ws.numel(),
                              None) == 0, lib.nrf_last_error()
    torch.cuda.synchronize()
    nb, nv = max(1, -(-n // A.TILE)), A.COLUMNS[mode]
    part = ws[:nb * nv * 8].cpu().numpy().view(F64).reshape(nb, nv)
    return part, (st.cpu().numpy().astype(np.uint32) if stats else None), ws


def run_solve(api, ws, n, mode, scale, state, iteration=0, n_history=1):
    lib = api[0].lib()
    st = device_state(api, None)
    st.copy_(torch.from_numpy(np.array(state, F64)))
    hist = torch.full((n_history, 8), -7.0, dtype=torch.float64, device="cuda")
    assert lib.nrf_align_solve(n, mode, int(scale), iteration, n_history, p(st), p(hist), p(ws), ws.numel(), None) == 0, lib.nrf_last_error()
    torch.cuda.synchronize()
    return st.cpu().numpy(), hist.cpu().numpy()


# ------------------------------------------------------------------------------------ 1. the pose and apply
def test_state_init_writes_the_identity_or_the_normalised_pose(api):
    assert np.array_equal(bits64(device_state(api)), bits64(A.IDENTITY))
    assert np.array_equal(bits64(device_state(api, POSE)), bits64(A.state_init(POSE)))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_apply_equals_the_restatement(api, n):
    lib = api[0].lib()
    rng = np.random.default_rng(n)
    x = (rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-3, 3, (n, 1))).astype(F32)
    if n > 1:
        x[0] = [np.nan, 1, np.inf]
    state = device_state(api, POSE)
    dx = dev(x, F32) if n else None
    for rotate_only in (0, 1):
        out = torch.full((n + 1, 3), -7.0, device="cuda")
        assert lib.nrf_align_apply(p(dx), n, p(state), rotate_only, p(out) if n else None, None) == 0
        want = A.apply(x, A.state_init(POSE), bool(rotate_only))
        assert np.array_equal(bits(out[:n]), bits(want)) and (out[n] == -7).all(), rotate_only
    if n:
        assert lib.nrf_align_apply(p(dx), n, p(state), 0, p(dx), None) == 0          # in place
        assert np.array_equal(bits(dx), bits(A.apply(x, A.state_init(POSE))))


# ------------------------------------------------------------------------------------ 2. the sums
def pairs(n, seed, case):
    """n pairs around the ellipsoid: y near the face f's point p"""
    rng = np.random.default_rng(seed)
    verts, faces = case["target"]
    f = rng.integers(0, len(faces), n).astype(np.int32)
    w = rng.dirichlet(np.ones(3), n)
    pp = (w[:, :, None] * verts[faces[f]].astype(F64)).sum(1)
    return (pp + 0.02 * rng.normal(size=(n, 3))).astype(F32), pp.astype(F32), f


SIZES = [0, 1, 63, 64, 65, 255, 256, 257, A.TILE - 1, A.TILE, A.TILE + 1, 257 * A.TILE + 1]          # the last: more block partials than the finish has threads


@pytest.mark.parametrize("mode", [A.POINT, A.PLANE])
@pytest.mark.parametrize("n", SIZES)
def test_sums_equal_the_restatement_at_every_size(api, case, mode, n):
    y, pp, f = pairs(n, n + mode, case)
    verts, faces = case["target"]
    part, stats, ws = run_sums(api, y, pp, f, mode, verts, faces)
    want, wstats = A.sums(y, pp, f, mode, verts, faces)
    assert part.shape == want.shape and np.array_equal(bits64(part), bits64(want)) and stats.tolist() == wstats.tolist() == [0, 0, 0, 0]
    for scale in (False, True):          # and the totals through the solve: the history's first two columns are totals
        state, hist = run_solve(api, ws, n, mode, scale, A.IDENTITY)
        wstate, wrow = A.solve(want, mode, scale, A.IDENTITY)
        assert np.array_equal(bits64(state), bits64(wstate)) and np.array_equal(bits64(hist[0]), bits64(wrow)), (scale, hist[0], wrow)


@pytest.mark.parametrize("mode", [A.POINT, A.PLANE])
def test_every_class_of_dropped_pair_is_skipped_and_counted(api, case, mode):
    n = 2 * A.TILE + 300
    y, pp, f = pairs(n, 9, case)
    verts, faces = (x.copy() for x in case["target"])
    faces[3] = [0, len(verts), 1]          # a bad face
    faces[4] = [0, -1, 1]
    verts[faces[5, 1]] = [np.nan, 0, 0]     # makes every face around that vertex non-finite
    faces[6] = [7, 7, 8]                   # no area: no normal
    f[10::97] = -1
    f[11::97] = -5
    y[12::97, 1] = np.nan
    pp[13::97, 2] = -np.inf
    f[14::97] = 3
    f[15::97] = 4
    f[16::97] = 5
    f[17::97] = 6
    f[18::97] = len(faces)                 # beyond the list: bad
    part, stats, ws = run_sums(api, y, pp, f, mode, verts, faces)
    want, wstats = A.sums(y, pp, f, mode, verts, faces)
    print("dropped:", wstats.tolist())
    assert np.array_equal(bits64(part), bits64(want)) and stats.tolist() == wstats.tolist()
    assert wstats[0] > 0 and wstats[1] > 0 and (wstats[2] > 0 and wstats[3] > 0) == (mode == A.PLANE)
    state, hist = run_solve(api, ws, n, mode, True, A.state_init(POSE))
    wstate, wrow = A.solve(want, mode, True, A.state_init(POSE))
    assert np.array_equal(bits64(state), bits64(wstate)) and np.array_equal(bits64(hist[0]), bits64(wrow)) and wrow[0] == n - wstats.sum()
    # stats are added to, and optional
    part2, none, _ = run_sums(api, y, pp, f, mode, verts, faces, stats=False)
    assert none is None and np.array_equal(bits64(part2), bits64(want))


def test_a_sum_keeps_its_bits_under_the_permutations_the_contract_names_and_the_restatement_follows_the_others(api, case):
    n = 3 * A.TILE
    y, pp, f = pairs(n, 21, case)
    f[5::7] = -1
    base, _, _ = run_sums(api, y, pp, f, A.POINT)
    # the contract: dropped pairs are skipped, so what a dropped row holds does not matter ...
    y2 = y.copy()
    y2[f < 0] = 1e30
    assert np.array_equal(bits64(run_sums(api, y2, pp, f, A.POINT)[0]), bits64(base))
    # ... and nothing more is promised: with every lane's entries reversed the device still equals the restatement of THAT order, whatever its bits
    perm = np.arange(n).reshape(3, A.TILE // A.BLOCK, A.BLOCK)[:, ::-1].reshape(-1)
    got, _, _ = run_sums(api, y[perm], pp[perm], f[perm], A.POINT)
    assert np.array_equal(bits64(got), bits64(A.sums(y[perm], pp[perm], f[perm], A.POINT)[0]))
    assert np.array_equal(bits64(base), bits64(A.sums(y, pp, f, A.POINT)[0]))


# ------------------------------------------------------------------------------------ 3. the solve
def test_solve_equals_the_restatement_on_the_host_tests_systems(api):
    import test_align_host as H
    start = A.state_init(POSE)
    for name, (y, pp) in list(H.clouds().items()) + [("collinear", (np.outer(np.arange(9.0), [0.3, -0.5, 0.8]).astype(F32), np.outer(np.arange(9.0), [0, 0.6, 0.8]).astype(F32)))]:
        f = np.zeros(len(y), np.int32)
        part, _, ws = run_sums(api, y, pp, f, A.POINT)
        for scale in (False, True):
            for init in (A.IDENTITY, start):
                state, hist = run_solve(api, ws, len(y), A.POINT, scale, init, iteration=2, n_history=4)
                wstate, wrow = A.solve(part, A.POINT, scale, init)
                assert wrow[2] == A.OK and np.array_equal(bits64(state), bits64(wstate)) and np.array_equal(bits64(hist[2]), bits64(wrow)), (name, scale)
                assert (hist[[0, 1, 3]] == -7).all()
    for name, (y, pp, f, verts, faces) in H.plane_cases().items():
        part, _, ws = run_sums(api, y, pp, f, A.PLANE, verts, faces)
        for scale in (False, True):
            state, hist = run_solve(api, ws, len(y), A.PLANE, scale, start)
            wstate, wrow = A.solve(part, A.PLANE, scale, start)
            assert wrow[2] == A.OK and np.array_equal(bits64(state), bits64(wstate)) and np.array_equal(bits64(hist[0]), bits64(wrow)), (name, scale)


def test_every_degenerate_case_sets_its_flag_and_keeps_the_state(api):
    rng = np.random.default_rng(5)
    start = A.state_init(POSE)
    y = rng.normal(size=(10, 3)).astype(F32)
    zero = np.zeros(10, np.int32)
    cases = [(y[:2], y[:2], zero[:2], A.POINT, False, None, A.FEW_PAIRS), (y[:0], y[:0], zero[:0], A.POINT, False, None, A.FEW_PAIRS),
             (y, y, np.where(np.arange(10) < 2, 0, -1).astype(np.int32), A.POINT, True, None, A.FEW_PAIRS),
             (np.repeat(y[:1], 5, 0), y[:5], zero[:5], A.POINT, False, None, A.NO_SPREAD), (y, np.zeros_like(y), zero, A.POINT, True, None, A.BAD_SCALE)]
    flat = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], F32), np.array([[0, 1, 2], [1, 3, 2]], np.int32))
    f = (np.arange(10) % 2).astype(np.int32)
    pp = y * np.array([1, 1, 0], F32)
    cases += [(y[:n], pp[:n], f[:n], A.PLANE, scale, flat, flag) for n, scale, flag in [(5, False, A.FEW_PAIRS), (6, True, A.FEW_PAIRS), (10, False, A.BAD_PIVOT),
                                                                                        (10, True, A.BAD_PIVOT)]]
    seen = set()
    for src, dst, face, mode, scale, mesh, flag in cases:
        part, _, ws = run_sums(api, src, dst, face, mode, *(mesh or (None, None)))
        state, hist = run_solve(api, ws, len(face), mode, scale, start)
        wstate, wrow = A.solve(part, mode, scale, start)
        assert wrow[2] == flag and np.array_equal(bits64(hist[0]), bits64(wrow)), (flag, hist[0], wrow)
        assert np.array_equal(bits64(state), bits64(start)) and wstate == start
        seen.add(flag)
    assert seen == {A.FEW_PAIRS, A.NO_SPREAD, A.BAD_PIVOT, A.BAD_SCALE}


# ------------------------------------------------------------------------------------ 4. the chain
@pytest.fixture(scope="module")
def chain_refs(case):
    """The restated ICP once per configuration, shared by the tests below: (method, scale, target kind) -> (state, history, states)"""
    out = {}
    for method, mode in (("plane", A.PLANE), ("point", A.POINT)):
        for scale in (False, True):
            out[method, scale, "mesh"] = A.icp(case["src"], case["target"], mode, scale, 6, max_dist=0.2)
    for scale in (False, True):
        out["point", scale, "points"] = A.icp(case["src"], case["target"][0], A.POINT, scale, 6, max_dist=0.2)
    return out


@pytest.mark.parametrize("config", [("plane", False, "mesh"), ("plane", True, "mesh"), ("point", False, "mesh"), ("point", True, "mesh"), ("point", False, "points"),
                                    ("point", True, "points")])
def test_register_icp_equals_the_restated_loop_and_two_runs_agree(api, case, chain_refs, config):
    method, scale, kind = config
    source = make_mesh(api, *case["source"])
    target = make_mesh(api, *case["target"]) if kind == "mesh" else dev(case["target"][0], F32)
    wstate, whist, wstates = chain_refs[config]
    runs = [api[3].RegisterICP(source, target, iterations=6, max_dist=0.2, method=method, scale=scale, n_points=A.N_SAMPLES, seed=A.SAMPLE_SEED) for _ in range(2)]
    for r in runs:
        assert r.History.shape == (6, 8) and r.History.dtype == torch.float64 and r.History.is_cuda and r.Transform.State.is_cuda
        assert np.array_equal(bits64(r.Transform.State), bits64(wstate)) and np.array_equal(bits64(r.History), bits64(whist)), (r.History, whist)
    err = A.pose_error(list(runs[0].Transform.State.cpu().numpy()), case)
    print(config, "pose error after 6 iterations: %.3e deg, scale %.3e, shift %.3e" % err)
    if config == ("plane", True, "mesh"):
        import test_align_host as H
        assert err[0] <= 2 * H.ICP_DEG_MEASURED and err[1] <= 2 * H.ICP_S_MEASURED and err[2] <= 2 * H.ICP_T_MEASURED


def test_the_state_after_one_and_after_five_composed_iterations(api, case, chain_refs):
    source, target = make_mesh(api, *case["source"]), make_mesh(api, *case["target"])
    grid = api[1].FaceGrid(target)          # also: a FaceGrid as the target, built once
    for its in (1, 5):
        r = api[3].RegisterICP(source, grid, iterations=its, max_dist=0.2, method="plane", scale=True, n_points=A.N_SAMPLES, seed=A.SAMPLE_SEED)
        assert np.array_equal(bits64(r.Transform.State), bits64(chain_refs["plane", True, "mesh"][2][its])), its
    # a start pose, a schedule of max_dist, points as the source, and the dropped pairs counted
    init = api[3].Transform(quaternion=POSE[:4], scale=1.05, translation=(0.01, 0.0, -0.01))
    before = init.State.clone()
    sched = [0.2, 0.1, 0.03]
    stats = torch.zeros((4,), dtype=torch.int32, device="cuda")
    r = api[3].RegisterICP(dev(case["src"], F32), target, init=init, iterations=3, max_dist=sched, method="point", stats=stats)
    first = A.state_init(POSE[:4] + [1.05, 0.01, 0.0, -0.01])
    wstate, whist, _ = A.icp(case["src"], case["target"], A.POINT, False, 3, max_dist=sched, init=first)
    assert np.array_equal(bits64(r.Transform.State), bits64(wstate)) and np.array_equal(bits64(r.History), bits64(whist)) and torch.equal(init.State, before)
    assert stats.tolist() == [int(3 * len(case["src"]) - whist[:, 0].sum()), 0, 0, 0] and stats[0] > 0


def test_a_tolerance_stops_where_the_restatement_stops(api, case):
    source, target = make_mesh(api, *case["source"]), make_mesh(api, *case["target"])
    r = api[3].RegisterICP(source, target, iterations=12, max_dist=0.2, method="plane", scale=True, n_points=A.N_SAMPLES, seed=A.SAMPLE_SEED, tolerance=1e-7,
                           check_every=2)
    wstate, whist, _ = A.icp(case["src"], case["target"], A.PLANE, True, 12, max_dist=0.2, tolerance=1e-7, check_every=2)
    assert len(whist) == 6 and r.History.shape == (6, 8)
    assert np.array_equal(bits64(r.Transform.State), bits64(wstate)) and np.array_equal(bits64(r.History), bits64(whist))


# ------------------------------------------------------------------------------------ 5. the Python layer
def test_align_points_transform_and_transform_mesh(api, case):
    import test_align_host as H
    y, pp = H.clouds()["random500"]
    r = api[3].AlignPoints(dev(y, F32), dev(pp, F32), scale=True)
    wstate, wrow = A.align_points(y, pp, True)
    assert np.array_equal(bits64(r.Transform.State), bits64(wstate)) and np.array_equal(bits64(r.History), bits64([wrow]))
    T = r.Transform
    assert np.allclose(T.Matrix.cpu().numpy(), A.matrix(wstate), rtol=0, atol=1e-14)
    assert np.array_equal(bits(T.Apply(dev(y, F32))), bits(A.apply(y, wstate)))
    back = T.Inverse().Compose(T)
    assert np.allclose(back.Matrix.cpu().numpy(), np.eye(4), atol=1e-14) and np.allclose(T.Compose(T.Inverse()).Matrix.cpu().numpy(), np.eye(4), atol=1e-14)
    twice = T.Compose(T)
    assert np.allclose(twice.Matrix.cpu().numpy(), A.matrix(wstate) @ A.matrix(wstate), atol=1e-13)
    assert np.array_equal(bits64(api[3].Transform().State), bits64(A.IDENTITY))
    verts, faces = case["target"]
    normals = dev(verts / np.linalg.norm(verts, axis=1, keepdims=True), F32)
    colors = dev(np.abs(verts), F32)
    m = api[2].Mesh(dev(verts, F32), dev(faces, np.int32), normals, Colors=colors)
    moved = api[3].TransformMesh(m, T)
    assert type(moved) is type(m) and moved.Faces is m.Faces and moved.Colors is colors and moved.Relevancy is None
    assert np.array_equal(bits(moved.Vertices), bits(A.apply(verts, wstate))) and np.array_equal(bits(moved.Normals), bits(A.apply(normals.cpu().numpy(), wstate, True)))
    assert np.array_equal(bits(m.Vertices), bits(verts))          # the input is left alone
    with pytest.raises(api[0].NrfError):
        api[3].AlignPoints(dev(y, F32), dev(pp[:10], F32))
    with pytest.raises(api[0].NrfError):
        api[3].RegisterICP(dev(y, F32), dev(pp, F32), method="plane")
    with pytest.raises(api[0].NrfError):
        api[3].RegisterICP(dev(y, F32), dev(pp, F32), method="point", iterations=3, max_dist=[0.1, 0.2])


def test_surface_distance_with_and_without_align(api, case):
    a, b = make_mesh(api, *case["source"]), make_mesh(api, *case["target"])
    kw = dict(taus=(0.005, 0.02), n_points=3000, seed=3)
    # without the keyword: the present result, the restatement composed by hand over the same samples
    clouds = []
    for verts, faces in (case["source"], case["target"]):
        area = G.sample_count(verts, faces, 0.0, 3)["total_area"]
        clouds.append(G.sample(verts, faces, F32(3000 / area), 3)[1])
    plain = api[1].SurfaceDistance(a, b, **kw)
    for name, value in G.surface_distance(clouds[0], clouds[1], kw["taus"]).items():
        assert np.array_equal(bits64(getattr(plain, name)), bits64(value)), name
    none = api[1].SurfaceDistance(a, b, align=None, **kw)
    for name in ("Accuracy", "Completeness", "Chamfer", "ChamferSq", "Hausdorff", "Precision", "Recall", "FScore"):
        assert np.array_equal(bits64(getattr(none, name)), bits64(getattr(plain, name))), name
    # "icp" is RegisterICP(a, b) at its defaults, then the distance of the moved side
    pose = api[3].RegisterICP(a, b).Transform
    by_hand = api[1].SurfaceDistance(api[3].TransformMesh(a, pose), b, **kw)
    icp = api[1].SurfaceDistance(a, b, align="icp", **kw)
    given = api[1].SurfaceDistance(a, b, align=pose, **kw)
    for name in ("Accuracy", "Completeness", "Chamfer", "ChamferSq", "Hausdorff", "Precision", "Recall", "FScore"):
        assert np.array_equal(bits64(getattr(icp, name)), bits64(getattr(by_hand, name))) and np.array_equal(bits64(getattr(given, name)), bits64(getattr(by_hand, name)))
    print(f"Chamfer {float(plain.Chamfer):.4f} as given, {float(icp.Chamfer):.4f} registered (rigid: the scale of 1.1 remains)")
    assert float(icp.Chamfer) < float(plain.Chamfer)
    pts = api[1].SurfaceDistance(dev(clouds[0], F32), dev(clouds[1], F32), taus=kw["taus"], align=pose)
    moved = api[1].SurfaceDistance(pose.Apply(dev(clouds[0], F32)), dev(clouds[1], F32), taus=kw["taus"])
    assert np.array_equal(bits64(pts.Chamfer), bits64(moved.Chamfer))
    with pytest.raises(api[0].NrfError):
        api[1].SurfaceDistance(a, b, align="umeyama")


# ------------------------------------------------------------------------------------ 6. refusals
def test_refusals_come_before_any_write(api, case):
    lib = api[0].lib()
    n = 300
    y, pp, f = pairs(n, 1, case)
    dy, dp, df = dev(y, F32), dev(pp, F32), dev(f, np.int32)
    dv, dfc = dev(case["target"][0], F32), dev(case["target"][1], np.int32)
    state = torch.full((9,), -7.0, dtype=torch.float64, device="cuda")
    hist = torch.full((4, 8), -7.0, dtype=torch.float64, device="cuda")
    out = torch.full((n, 3), -7.0, device="cuda")
    stats = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    ws = buffer(lib.nrf_align_workspace_bytes(n, A.PLANE) + 256)
    need = lib.nrf_align_workspace_bytes(n, A.PLANE)
    assert need == 256 * -(-A.COLUMNS[A.PLANE] * 8 // 256) and lib.nrf_align_workspace_bytes(-1, A.POINT) == 0 and lib.nrf_align_workspace_bytes(n, 2) == 0
    assert lib.nrf_align_workspace_bytes(257 * A.TILE + 1, A.POINT) == 256 * -(-258 * A.COLUMNS[A.POINT] * 8 // 256)

    def sums(y_=dy, p_=dp, f_=df, n_=n, mode=A.PLANE, v_=dv, nv=len(dv), fc_=dfc, nf=len(dfc), st_=stats, w_=ws.data_ptr(), wb=need):
        return lib.nrf_align_sums(p(y_), p(p_), p(f_), n_, mode, p(v_), nv, p(fc_), nf, p(st_), w_, wb, None)

    def solve(n_=n, mode=A.PLANE, scale=1, it=0, nh=4, s_=state.data_ptr(), h_=hist.data_ptr(), w_=ws.data_ptr(), wb=need):
        return lib.nrf_align_solve(n_, mode, scale, it, nh, s_, h_, w_, wb, None)
    refused = [sums(y_=None), sums(p_=None), sums(f_=None), sums(n_=-1), sums(n_=1 << 31), sums(mode=2), sums(mode=-1), sums(v_=None), sums(fc_=None), sums(nv=-1),
               sums(nf=1 << 31), sums(w_=None), sums(w_=ws.data_ptr() + 4), sums(y_=dy.data_ptr() + 2), sums(f_=df.data_ptr() + 1),
               solve(n_=-1), solve(mode=2), solve(scale=2), solve(scale=-1), solve(it=-1), solve(it=4), solve(nh=0), solve(s_=None), solve(s_=state.data_ptr() + 4),
               solve(h_=hist.data_ptr() + 4), solve(w_=None), solve(w_=ws.data_ptr() + 4),
               lib.nrf_align_apply(None, n, p(state), 0, p(out), None), lib.nrf_align_apply(p(dy), n, p(state), 0, None, None),
               lib.nrf_align_apply(p(dy), n, None, 0, p(out), None), lib.nrf_align_apply(p(dy), n, state.data_ptr() + 4, 0, p(out), None),
               lib.nrf_align_apply(p(dy), -1, p(state), 0, p(out), None), lib.nrf_align_apply(p(dy), n, p(state), 2, p(out), None),
               lib.nrf_align_apply(p(dy), n, p(state), 0, out.data_ptr() + 2, None),
               lib.nrf_align_state_init(None, None, None), lib.nrf_align_state_init(None, state.data_ptr() + 4, None)]
    for bad in ([0, 0, 0, 0, 1, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, -1, 0, 0, 0], [np.nan, 0, 0, 0, 1, 0, 0, 0], [1, 0, 0, 0, 1, np.inf, 0, 0]):
        arr = (C.c_double * 8)(*bad)
        refused.append(lib.nrf_align_state_init(C.addressof(arr), p(state), None))
    assert refused == [INVALID_ARG] * len(refused), refused
    assert lib.nrf_last_error().startswith(b"nrf_align_state_init")
    assert sums(wb=need - 1) == WORKSPACE and solve(wb=need - 1) == WORKSPACE and lib.nrf_last_error().startswith(b"nrf_align_solve")
    torch.cuda.synchronize()
    assert (state == -7).all() and (hist == -7).all() and (out == -7).all() and (stats == -7).all() and (ws == 0x5A).all()
    # point mode needs no mesh, and the same calls go through once nothing is wrong
    assert sums(mode=A.POINT, v_=None, nv=0, fc_=None, nf=0, st_=None, wb=lib.nrf_align_workspace_bytes(n, A.POINT)) == 0
    assert sums(st_=None) == 0 and lib.nrf_align_state_init(None, p(state), None) == 0 and solve(it=3) == 0
    torch.cuda.synchronize()
    want_state, want_row = A.solve(A.sums(y, pp, f, A.PLANE, *case["target"])[0], A.PLANE, True, A.IDENTITY)
    assert np.array_equal(bits64(state[:8]), bits64(want_state)) and np.array_equal(bits64(hist[3]), bits64(want_row))
    assert float(state[8]) == -7 and (hist[:3] == -7).all() and (ws[need:] == 0x5A).all()
