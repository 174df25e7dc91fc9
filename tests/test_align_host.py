"""Registration without a GPU: the numpy restatement (tests/align_ref.py) of nrf_align_sums / nrf_align_solve against independent linear algebra -- Horn's closed
form through Jacobi against the SVD solution of Kabsch / Umeyama, the Cholesky solve against np.linalg.solve --, every degenerate flag, the restated ICP loop on the
bumped ellipsoid, the pruned closest-point search the loop uses against the brute force, and the header's constants and entries against the Python side.
The tolerances are what these very runs measured on the CPU (DESIGN 8s records them) with the margin stated beside each."""
import math
import os
import re

import numpy as np
import pytest

import align_ref as A
import closest_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64

# measured on the CPU over the cases below: the largest |R - R_svd|, |s - s_svd| / s, |t - t_svd| (4x margin below)
POINT_R_MEASURED, POINT_S_MEASURED, POINT_T_MEASURED = 7.8e-16, 5.3e-16, 2.3e-15
# the largest |x - x_numpy| / max(1, |x_numpy|) of the plane solve over its cases (4x margin below)
PLANE_X_MEASURED = 1.1e-15
# the restated ICP on the ellipsoid, plane mode with scale after 6 iterations: rotation error in degrees, |s - s_true|, |t - t_true|_inf (2x margin below)
ICP_DEG_MEASURED, ICP_S_MEASURED, ICP_T_MEASURED = 6.1e-7, 1.1e-9, 4.3e-10


def svd_fit(y, p, scale):
    """Kabsch / Umeyama: (R, s, t) minimising sum |s R y + t - p|^2"""
    y, p = np.asarray(y, F64), np.asarray(p, F64)
    yb, pb = y.mean(0), p.mean(0)
    yc, pc = y - yb, p - pb
    U, D, Vt = np.linalg.svd(pc.T @ yc)
    sg = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ sg @ Vt
    s = (D * np.diag(sg)).sum() / (yc ** 2).sum() if scale else 1.0
    return R, s, pb - s * R @ yb


def rot_of(state):
    return np.array(A.quat_rot(*state[:4])).reshape(3, 3)


def clouds():
    """name -> (src, dst) f32: what the point solve must agree with the SVD on"""
    rng = np.random.default_rng(7)
    out = {}
    for k, n in enumerate((3, 4, 17, 500, 3000)):
        y = rng.normal(size=(n, 3)) * rng.uniform(0.1, 3.0, 3)
        R = A.rotation(*(lambda a: (a / np.linalg.norm(a), rng.uniform(-170, 170)))(rng.normal(size=3)))
        out[f"random{n}"] = (y, rng.uniform(0.5, 2.0) * y @ R.T + rng.normal(size=3) + 0.01 * rng.normal(size=(n, 3)))
    y = rng.normal(size=(200, 3))
    ex, ez = np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0])
    out["rot90"] = (y, y @ A.rotation(ez, 90.0).round().T)
    out["rot180"] = (y, y @ A.rotation(ex, 180.0).round().T + 1.0)          # the answer has w = 0: the start vector (1, 0, 0, 0) is orthogonal to it
    out["rot180z"] = (y, y @ A.rotation(ez, 180.0).round().T)
    out["identity"] = (y, y.copy())
    flat = y * np.array([1.0, 1.0, 0.0])
    out["planar"] = (flat, 1.3 * flat @ A.rotation(np.array([0.6, 0.0, 0.8]), 40.0).T + 0.2)
    return {k: (np.asarray(a, F32), np.asarray(b, F32)) for k, (a, b) in out.items()}


@pytest.mark.parametrize("scale", [False, True])
def test_point_solve_agrees_with_the_svd_solution(scale):
    worst = np.zeros(3)
    for name, (y, p) in clouds().items():
        state, row = A.align_points(y, p, scale)
        assert row[2] == A.OK and row[0] == len(y), name
        R, s, t = svd_fit(y, p, scale)
        err = np.array([np.abs(rot_of(state) - R).max(), abs(state[4] - s) / s, np.abs(np.array(state[5:8]) - t).max()])
        print(f"point solve {name:10s} scale={scale}: |R - R_svd| {err[0]:.2e}  |s - s_svd| / s {err[1]:.2e}  |t - t_svd| {err[2]:.2e}")
        worst = np.maximum(worst, err)
        assert abs(np.linalg.det(rot_of(state)) - 1.0) < 1e-14 and state[0] >= 0.0, name
    print("worst", worst)
    assert worst[0] <= 4 * POINT_R_MEASURED and worst[1] <= 4 * POINT_S_MEASURED and worst[2] <= 4 * POINT_T_MEASURED


def test_point_solve_of_a_collinear_cloud_reaches_the_svd_residual():
    """A line leaves the rotation about itself free: the two solutions differ, their residuals do not"""
    rng = np.random.default_rng(3)
    y = np.outer(rng.normal(size=50), [0.3, -0.5, 0.8]).astype(F32)
    p = (y.astype(F64) @ A.rotation(np.array([0.0, 0.6, 0.8]), 25.0).T + 0.1).astype(F32)
    state, row = A.align_points(y, p, True)
    assert row[2] == A.OK
    R, s, t = svd_fit(y, p, True)
    mine = ((state[4] * y.astype(F64) @ rot_of(state).T + state[5:8] - p) ** 2).sum()
    ref = ((s * y.astype(F64) @ R.T + t - p) ** 2).sum()
    print(f"collinear: residual {mine:.3e} against the SVD's {ref:.3e}")
    assert mine <= ref + 1e-12 * (p.astype(F64) ** 2).sum()          # both are rounding noise of the fp32 data's own scale


def plane_cases():
    rng = np.random.default_rng(11)
    c = A.ellipsoid_case()
    verts, faces = c["target"]
    out = {}
    for k, n in enumerate((7, 40, 2000)):
        f = rng.integers(0, len(faces), n).astype(np.int32)
        tri = verts[faces[f]].astype(F64)
        w = rng.dirichlet(np.ones(3), n)
        p = (w[:, :, None] * tri).sum(1)
        y = p + 0.01 * rng.normal(size=(n, 3))
        out[f"ellipsoid{n}"] = (y.astype(F32), p.astype(F32), f, verts, faces)
    return out


@pytest.mark.parametrize("scale", [False, True])
def test_plane_solve_agrees_with_numpy_solve(scale):
    m = 7 if scale else 6
    worst = 0.0
    for name, (y, p, f, verts, faces) in plane_cases().items():
        part, stats = A.sums(y, p, f, A.PLANE, verts, faces)
        assert not stats.any()
        T = A.totals(part)
        flag, dq, ds, dt = A.solve_plane(T, scale)
        assert flag == A.OK and T[35] == len(y), name
        H, g = A.plane_system(T)
        x = np.linalg.solve(np.array(H)[:m, :m], np.array(g)[:m])
        nrm = math.sqrt(1.0 + (x[:3] ** 2).sum() / 4.0)
        mine = np.array([2.0 * dq[1] / dq[0], 2.0 * dq[2] / dq[0], 2.0 * dq[3] / dq[0]] + dt + ([ds - 1.0] if scale else []))
        err = np.abs(mine - x).max() / max(1.0, np.abs(x).max())
        print(f"plane solve {name:14s} scale={scale}: cond {np.linalg.cond(np.array(H)[:m, :m]):.1e}  |x - x_numpy| {err:.2e}")
        worst = max(worst, err)
        assert abs(dq[0] - 1.0 / nrm) < 1e-15
    assert worst <= 4 * PLANE_X_MEASURED


def test_every_degenerate_case_sets_its_flag_and_leaves_the_state():
    rng = np.random.default_rng(5)
    start = A.state_init([0.9, 0.1, -0.2, 0.3, 1.5, 0.1, 0.2, 0.3])
    y = rng.normal(size=(10, 3)).astype(F32)

    def point(src, dst, scale, face=None):
        part, _ = A.sums(src, dst, np.zeros(len(src), np.int32) if face is None else face, A.POINT)
        return A.solve(part, A.POINT, scale, start)
    for src, dst, scale, face, flag in [(y[:2], y[:2], False, None, A.FEW_PAIRS), (y[:0], y[:0], False, None, A.FEW_PAIRS),
                                        (y, y, False, np.where(np.arange(10) < 2, 0, -1).astype(np.int32), A.FEW_PAIRS),
                                        (np.repeat(y[:1], 5, 0), y[:5], False, None, A.NO_SPREAD), (y, np.zeros_like(y), True, None, A.BAD_SCALE)]:
        state, row = point(src, dst, scale, face)
        assert row[2] == flag and state == start and row[3:7] == [0.0, 0.0, 1.0, start[4]], (flag, row)
    assert point(y, np.zeros_like(y), False)[1][2] == A.OK          # without scale a target that has collapsed still gives a translation
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], F32)
    faces = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
    f = (np.arange(10) % 2).astype(np.int32)
    p = y * np.array([1, 1, 0], F32)
    for n, scale, flag in [(5, False, A.FEW_PAIRS), (6, True, A.FEW_PAIRS), (10, False, A.BAD_PIVOT), (10, True, A.BAD_PIVOT)]:
        part, stats = A.sums(y[:n], p[:n], f[:n], A.PLANE, verts, faces)
        state, row = A.solve(part, A.PLANE, scale, start)
        assert row[2] == flag and state == start and not stats.any(), (n, scale, row)          # one plane: the rotation about its normal has no equation


def test_apply_is_the_float64_pose_rounded_once():
    rng = np.random.default_rng(2)
    x = (rng.normal(size=(300, 3)) * 10.0 ** rng.uniform(-3, 3, (300, 1))).astype(F32)
    state = A.state_init([0.3, -0.5, 0.7, 0.2, 1.7, 0.5, -2.0, 3.0])
    m = A.matrix(state)
    want = x.astype(F64) @ m[:3, :3].T + m[:3, 3]
    got = A.apply(x, state).astype(F64)
    assert np.abs(got - want).max() <= np.abs(want).max() * 2.0 ** -23          # one fp32 rounding and a few fp64 ones
    rot = A.apply(x, state, rotate_only=True).astype(F64)
    assert np.abs(rot - x.astype(F64) @ rot_of(state).T).max() <= np.abs(x).max() * 2.0 ** -23
    assert abs(math.sqrt(sum(v * v for v in state[:4])) - 1.0) < 1e-15 and A.state_init() == list(A.IDENTITY)


def test_sums_keep_their_bits_only_under_the_permutations_the_order_allows():
    """Swapping whole lanes' entries between steps of the same lane changes the order inside an accumulator; swapping two tiles changes which partial a pair joins"""
    rng = np.random.default_rng(4)
    n = 3 * A.TILE
    y, p = rng.normal(size=(n, 3)).astype(F32), rng.normal(size=(n, 3)).astype(F32)
    face = np.zeros(n, np.int32)
    base = A.bits64(A.totals(A.sums(y, p, face, A.POINT)[0]))
    dropped = face.copy()
    dropped[5::7] = -1
    keep = dropped >= 0
    # dropped pairs removed from a lane's list without disturbing the others: the same accumulations
    assert not np.array_equal(A.bits64(A.totals(A.sums(y, p, dropped, A.POINT)[0])), base)
    perm = np.arange(n).reshape(3, A.TILE // A.BLOCK, A.BLOCK)[:, ::-1].reshape(-1)          # every lane's four entries in reverse order
    assert not np.array_equal(A.bits64(A.totals(A.sums(y[perm], p[perm], face, A.POINT)[0])), base)
    # a pair that is dropped contributes nothing wherever it sits: moving the dropped rows' CONTENT does not matter
    y2 = y.copy()
    y2[~keep] = 123.0
    assert np.array_equal(A.bits64(A.totals(A.sums(y2, p, dropped, A.POINT)[0])), A.bits64(A.totals(A.sums(y, p, dropped, A.POINT)[0])))


@pytest.fixture(scope="module")
def case():
    c = A.ellipsoid_case()
    c["src"] = A.surface_samples(*c["source"])
    return c


def test_the_ellipsoid_is_the_stated_problem(case):
    verts, faces = case["target"]
    assert faces.shape == (1280, 3) and verts.shape == (642, 3) and abs(len(case["src"]) - A.N_SAMPLES) < 3 * math.sqrt(A.N_SAMPLES)
    assert np.allclose(np.abs(verts).max(0), A.SEMI_AXES * [1.0, 1.0, 1.0], rtol=0.2)
    n = np.cross(verts[faces[:, 1]] - verts[faces[:, 0]], verts[faces[:, 2]] - verts[faces[:, 0]])
    assert ((n * verts[faces].mean(1)).sum(1) > 0).all()          # counter-clockwise seen from outside


def test_pruned_closest_search_equals_the_brute_force(case):
    y = A.apply(case["src"], A.IDENTITY)
    for md in (np.inf, 0.03):
        a, b = A.closest_pruned(y, *case["target"], max_dist=md), CR.closest(y, *case["target"], max_dist=md)
        for k in ("d2", "face", "point"):
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (md, k)
        assert md == np.inf or 0 < (a["face"] < 0).sum() < len(y)


def test_icp_plane_with_scale_recovers_the_pose(case):
    state, hist, states = A.icp(case["src"], case["target"], A.PLANE, True, 6, max_dist=0.2)
    errs = [A.pose_error(s, case) for s in states]
    for k, e in enumerate(errs):
        print(f"plane + scale, after {k} iterations: rotation {e[0]:.3e} deg  |s - s_true| {e[1]:.3e}  |t - t_true| {e[2]:.3e}")
    assert (hist[:, 2] == A.OK).all() and 9.9 < errs[0][0] < 10.1
    deg, ds, dt = errs[-1]
    assert deg <= 2 * ICP_DEG_MEASURED and ds <= 2 * ICP_S_MEASURED and dt <= 2 * ICP_T_MEASURED
    assert errs[3][0] < 1e-3          # three to four iterations, as the trial found


def test_icp_point_reduces_the_rotation_error_monotonically(case):
    for target in (case["target"], case["target"][0]):
        _, hist, states = A.icp(case["src"], target, A.POINT, False, 8, max_dist=0.2, init=(1, 0, 0, 0, A.TRUE_SCALE, 0, 0, 0))
        deg = [A.pose_error(s, case)[0] for s in states]
        print("point mode, rotation error per iteration:", " ".join(f"{d:.3f}" for d in deg))
        assert all(b < a for a, b in zip(deg, deg[1:])) and (hist[:, 2] == A.OK).all()


def test_icp_tolerance_stops_at_a_check(case):
    _, hist, _ = A.icp(case["src"], case["target"], A.PLANE, True, 12, max_dist=0.2, tolerance=1e-7, check_every=2)
    assert len(hist) == 6 and hist[-1, 3] < 1e-7 and hist[-1, 4] < 1e-7 and not (hist[3, 3] < 1e-7 and hist[3, 4] < 1e-7)


def test_header_constants_and_entries_match_the_python_side():
    from nerfpp_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nerfpp_hip.h")).read()
    src = open(os.path.join(ROOT, "nerfpp_amd", "align.py")).read()

    def const(name):
        return re.search(rf"#define {name} +\(?(-?[\w.]+)", hdr)[1]
    assert [int(const(f"NRF_ALIGN_{n}")) for n in ("POINT", "PLANE", "TILE", "POINT_COLUMNS", "PLANE_COLUMNS", "JACOBI_SWEEPS")] == \
        [A.POINT, A.PLANE, A.TILE, A.COLUMNS[A.POINT], A.COLUMNS[A.PLANE], A.SWEEPS]
    assert float(const("NRF_ALIGN_JACOBI_BIG_THETA")) == A.BIG_THETA
    assert [int(const(f"NRF_ALIGN_FLAG_{n}")) for n in ("OK", "FEW_PAIRS", "NO_SPREAD", "BAD_PIVOT", "BAD_SCALE", "BAD_ROTATION")] == list(range(6))
    assert re.search(r"ALIGN_TILE, POINT_COLUMNS, PLANE_COLUMNS, JACOBI_SWEEPS = 1024, 19, 37, 8\n", src) and (_lib.NRF_ALIGN_POINT, _lib.NRF_ALIGN_PLANE) == (0, 1)
    want = [("nrf_align_state_init", ("i", "ppp")), ("nrf_align_apply", ("i", "plpipp")), ("nrf_align_workspace_bytes", ("z", "li")),
            ("nrf_align_sums", ("i", "pppliplplppzp")), ("nrf_align_solve", ("i", "liiiipppzp"))]
    at = _lib.SYMBOLS.index("nrf_mesh_voxelize")
    assert _lib.SYMBOLS[at + 1:at + 6] == [n for n, _ in want], "directly after nrf_mesh_voxelize, in the header's order"
    for name, sig in want:
        assert _lib.SIGNATURES[name] == sig and re.search(rf"NRF_API (size_t|int) {name}\(", hdr), name
    assert "CONTRACT." in hdr[hdr.index("Registration (align.hip"):hdr.index("NRF_API int nrf_align_state_init")]
