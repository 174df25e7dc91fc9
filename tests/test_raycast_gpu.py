"""Ray casting on a mesh on the MI355X: nrf_ray_cast_mesh, nrf_hemisphere_dirs and nrf_mesh_ambient_occlusion against the numpy restatement (tests/raycast_ref.py,
brute force over all (ray, face) pairs, no grid) with uint32 / integer equality -- spheres at three levels under rays of every kind, every grid shape, all cull
modes, a floor in a cell boundary, the large-face list, every condition of the brute-force fallback, invalid faces of every class -- the run-to-run guarantees, the
refusals over live buffers, and the Python layer built on it: RayCastMesh, Occluded, Visible, HemisphereDirections, AmbientOcclusion, BakeAmbientOcclusion,
ClipRaysToMesh and RayCastView.  No input here is outside the contract."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import closest_ref as CR
import geometry_ref as G
import raster_ref as R
import raycast_ref as RC
import smooth_ref as S
import texture_ref as X
import tsdf_ref as T

pytestmark = pytest.mark.gpu

F32 = np.float32
INVALID_ARG = 1
INF = float("inf")
CENTRE = np.asarray(T.SPHERE["centre"], np.float64)
SPHERE_BOX = (-0.8, -1.05, -0.7, 1.0, 0.75, 1.1)          # around the sphere of tsdf_ref.SPHERE, a little wider
GRIDS = [(1, 1, 1), (8, 8, 8), (7, 5, 3), (1024, 1, 1), (1, 1024, 1), (1, 1, 1024)]


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from nerfpp_amd import _lib as L, geometry, mesh, texture, raster
    return L, geometry, mesh, texture, raster


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, F32).view(np.uint32)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def p(t):
    return None if t is None else t.data_ptr()


def buffer(nbytes, pattern):
    ws = torch.empty((max(1, int(nbytes)),), dtype=torch.uint8, device="cuda")
    if pattern is not None:
        ws.fill_(pattern)
    return ws


def build_grid(api, verts, faces, box, dims, pattern=None):
    """nrf_face_grid_count + _build -> dict(dv, df, nv, nf, box, dims, n_refs, n_large, grid): what a cast takes"""
    lib = api[0].lib()
    verts, faces = np.asarray(verts, F32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)
    dv, df = (dev(verts, F32) if len(verts) else None), (dev(faces, np.int32) if len(faces) else None)
    box = np.ascontiguousarray(box, F32)
    ws = buffer(lib.nrf_face_grid_workspace_bytes(len(faces), *dims), pattern)
    n_refs, n_large = C.c_int64(-7), C.c_int64(-7)
    status = lib.nrf_face_grid_count(p(dv), len(verts), p(df), len(faces), box.ctypes.data, *dims, C.addressof(n_refs), C.addressof(n_large), None, p(ws), ws.numel(), None)
    assert status == 0, lib.nrf_last_error()
    g = dict(dv=dv, df=df, nv=len(verts), nf=len(faces), box=box, dims=tuple(dims), n_refs=int(n_refs.value), n_large=int(n_large.value))
    g["grid"] = buffer(lib.nrf_face_grid_bytes(g["nf"], *dims, g["n_refs"], g["n_large"]), pattern)
    status = lib.nrf_face_grid_build(p(dv), g["nv"], p(df), g["nf"], box.ctypes.data, *dims, g["n_refs"], g["n_large"], p(g["grid"]), g["grid"].numel(), p(ws), ws.numel(), None)
    assert status == 0, lib.nrf_last_error()
    return g


def mesh_args(g):
    return (p(g["dv"]), g["nv"], p(g["df"]), g["nf"], g["box"].ctypes.data, *g["dims"], g["n_refs"], g["n_large"], p(g["grid"]), g["grid"].numel())


def cast_grid(api, g, rays, cull=0, mode=0, skip=(), pattern=None, poison=-7.0):
    """One nrf_ray_cast_mesh call over poisoned outputs -> dict(t, face, uv, point, hit, stats)"""
    lib = api[0].lib()
    rays = np.ascontiguousarray(rays, F32)
    n = len(rays)
    dr = dev(rays, F32) if n else None
    closest = mode == 0
    t = torch.full((n,), poison, device="cuda") if closest else None
    face = torch.full((n,), -7, dtype=torch.int32, device="cuda") if closest else None
    uv = torch.full((n, 2), poison, device="cuda") if closest and "uv" not in skip else None
    pt = torch.full((n, 3), poison, device="cuda") if closest and "point" not in skip else None
    hit = None if closest and "hit" in skip else torch.full((n,), 77, dtype=torch.uint8, device="cuda")
    stats = torch.zeros((4,), dtype=torch.int32, device="cuda")
    ws = buffer(lib.nrf_ray_cast_workspace_bytes(n), pattern)
    status = lib.nrf_ray_cast_mesh(p(dr), n, rays.shape[1] if rays.ndim == 2 else 8, *mesh_args(g), cull, mode, p(t) if n else None, p(face) if n else None, p(uv), p(pt),
                                   p(hit) if n or not closest else None, p(stats), p(ws), ws.numel(), None)
    assert status == 0, lib.nrf_last_error()
    torch.cuda.synchronize()
    h = lambda x: None if x is None else x.cpu().numpy()
    return dict(t=h(t), face=h(face), uv=h(uv), point=h(pt), hit=h(hit), stats=stats.cpu().numpy().view(np.uint32))


def run(api, rays, verts, faces, box, dims, cull=0, skip=(), pattern=None):
    """count, build, cast in closest mode and in any mode -> the closest outputs with the any-mode hits as "any", n_refs, n_large"""
    g = build_grid(api, verts, faces, box, dims, pattern)
    out = cast_grid(api, g, rays, cull, 0, skip, pattern)
    some = cast_grid(api, g, rays, cull, 1, (), pattern)
    assert np.array_equal(some["stats"], out["stats"]), f"any mode counts {some['stats']}, closest mode {out['stats']}"
    out.update(any=some["hit"], n_refs=g["n_refs"], n_large=g["n_large"])
    return out


def assert_equal(got, want, what="", fallback=None):
    assert np.array_equal(bits(got["t"]), bits(want["t"])), f"{what}: t differs at {np.flatnonzero(bits(got['t']) != bits(want['t']))[:5]}"
    assert np.array_equal(got["face"], want["face"]), f"{what}: face differs at {np.flatnonzero(got['face'] != want['face'])[:5]}"
    if got["uv"] is not None:
        assert np.array_equal(bits(got["uv"]), bits(want["uv"])), f"{what}: uv"
    if got["point"] is not None:
        assert np.array_equal(bits(got["point"]), bits(want["point"])), f"{what}: point"
    if got["hit"] is not None:
        assert np.array_equal(got["hit"], want["hit"]), f"{what}: hit"
    if "any" in got:
        assert np.array_equal(got["any"], np.isfinite(got["t"]).astype(np.uint8)), f"{what}: any mode is not isfinite(T) at {np.flatnonzero(got['any'] != np.isfinite(got['t']))[:5]}"
    if "stats" in got and "stats" in want:
        assert np.array_equal(got["stats"][:3], [want["stats"][0], 0, 0]), f"{what}: stats {got['stats']} != {want['stats']}"
        if fallback is not None:
            ok = fallback(got["stats"][3]) if callable(fallback) else got["stats"][3] == fallback
            assert ok, f"{what}: {got['stats'][3]} rays served by the fallback"


@functools.lru_cache(maxsize=None)
def sphere_case(level):
    verts, faces = R.octa_sphere(T.SPHERE["centre"], T.SPHERE["radius"], level)
    rays, kinds = RC.mesh_rays(verts, faces, 10 + level, box=SPHERE_BOX)
    return verts, faces, rays, kinds, RC.cast(rays, verts, faces)


def open_rays(rays):
    """How many rays are valid with a non-empty range: what a condition that sends every ray to the fallback counts"""
    _, _, lo, hi, valid = RC.ray_parts(rays)
    return int((valid & (lo <= hi)).sum())


# ------------------------------------------------------------------------------------ 1. nrf_ray_cast_mesh
@pytest.mark.parametrize("level", [1, 2, 3])
def test_spheres_equal_the_restatement_on_every_grid(api, level):
    """Random rays from outside and inside, a zero direction component, axis rays that start on cell boundaries, rays at vertices and edges, rays in a face's plane,
    far finite and +inf, empty ranges, invalid rays; every grid the same bits, in closest and in any mode"""
    verts, faces, rays, kinds, want = sphere_case(level)
    assert len(faces) == 8 * 4 ** level and want["stats"].tolist() == [7, 0, 0, 0] and len(rays) <= 4096
    assert all(want["hit"][kinds[k]].sum() > 10 for k in ("outside", "inside", "zero", "axis", "vertex", "edge", "plane", "finite"))
    assert want["hit"][kinds["empty"]].sum() == 0 and want["hit"][kinds["invalid"]].sum() == 0 and (~np.isfinite(rays[:, 7])).sum() > 1000
    default = api[1].GridDims(np.array(SPHERE_BOX, F32), len(faces))
    for dims in GRIDS + [default]:
        got = run(api, rays, verts, faces, SPHERE_BOX, dims)
        assert_equal(got, want, f"level {level}, grid {dims}", fallback=0 if max(dims) <= 8 else None)
        miss = got["face"] < 0
        assert np.isinf(got["t"][miss]).all() and (got["uv"][miss] == 0).all() and (got["point"][miss] == 0).all()


@pytest.mark.parametrize("cull", [0, 1, 2])
def test_all_three_cull_modes(api, cull):
    verts, faces, rays, kinds, free = sphere_case(2)
    want = free if cull == 0 else RC.cast(rays, verts, faces, cull=cull)
    if cull:
        assert 100 < (want["face"] != free["face"]).sum(), "culling changes what many rays see"
    for dims in ((7, 5, 3), (16, 16, 16)):
        assert_equal(run(api, rays, verts, faces, SPHERE_BOX, dims, cull=cull), want, f"cull {cull}, grid {dims}", fallback=0)


def test_a_floor_quad_in_a_cell_boundary(api):
    """The plane z = 0.2 halves a box that is symmetric about it: with an even dim every point of the quad sits exactly on a cell boundary"""
    verts, faces = R.octa_sphere(T.SPHERE["centre"], T.SPHERE["radius"], 2)
    verts, faces = RC.floor_mesh(verts, faces, 0.2, 0.75)
    box = (-0.9, -0.9, -0.8, 0.9, 0.9, 1.2)
    rays, kinds = RC.mesh_rays(verts, faces, 13, box=box)
    want = RC.cast(rays, verts, faces)
    assert (want["face"] >= len(faces) - 2).sum() > 100, "the floor is what many rays hit"
    for dims in ((8, 8, 8), (2, 2, 2), (7, 5, 4), (32, 32, 64)):
        assert_equal(run(api, rays, verts, faces, box, dims), want, f"floor, grid {dims}", fallback=0 if max(dims) <= 8 else None)


def test_the_large_face_list_and_more_than_one_scan_round(api):
    """128 x 128 x 129 cells: every face of the sphere spans more than 64 such cells (the large list); 300 small faces strewn through the box are binned"""
    verts, faces, rays, _, _ = sphere_case(3)
    rng = np.random.default_rng(6)
    lo, hi = np.array(SPHERE_BOX[:3]), np.array(SPHERE_BOX[3:])
    small = (rng.uniform(lo + 0.05, hi - 0.05, (300, 1, 3)) + rng.uniform(-0.01, 0.01, (300, 3, 3))).astype(F32).reshape(-1, 3)
    verts = np.concatenate([verts, small])
    faces = np.concatenate([faces, (len(verts) - 900 + np.arange(900)).reshape(-1, 3).astype(np.int32)])
    aimed = RC.pack(np.tile(CENTRE + [0, 0, 3.0], (300, 1)), small.reshape(300, 3, 3).mean(1).astype(np.float64) - (CENTRE + [0, 0, 3.0]))
    rays = np.concatenate([rays[::3], aimed])
    got = run(api, rays, verts, faces, SPHERE_BOX, (128, 128, 129))
    want = RC.cast(rays, verts, faces)
    assert got["n_large"] == 512 and 300 <= got["n_refs"] <= 300 * 64 and (want["face"] >= 512).sum() > 20
    assert_equal(got, want, "128 x 128 x 129")


def test_a_box_smaller_than_the_mesh_sends_every_ray_to_the_fallback(api):
    verts, faces, rays, _, want = sphere_case(2)
    for box, dims in (((-0.2, -0.2, -0.2, 0.3, 0.3, 0.3), (4, 4, 4)), ((-0.8, -1.05, -0.7, 1.0, 0.75, 0.89), (8, 8, 8))):          # the second misses one vertex
        assert (verts.max(0) > np.array(box[3:])).any()
        assert_equal(run(api, rays, verts, faces, box, dims), want, f"box {box}", fallback=open_rays(rays))
    # and a mesh inside the box is served by the walk: the flag is made on the device, per call
    assert_equal(run(api, rays, verts, faces, SPHERE_BOX, (4, 4, 4)), want, "the whole box", fallback=0)


def test_origins_far_away_go_to_the_fallback(api):
    verts, faces, rays, _, _ = sphere_case(2)
    for scale in (1e3, 1e6):
        far = rays[::2].copy()
        far[:, :3] = (far[:, :3] * F32(scale)).astype(F32)
        aim = np.where(np.arange(len(far))[:, None] % 3 == 0, verts[np.arange(len(far)) % len(verts)], CENTRE.astype(F32))
        far[:, 3:6] = aim - far[:, :3]
        far[:, 6], far[:, 7] = 0, np.inf
        want = RC.cast(far, verts, faces)
        got = run(api, far, verts, faces, SPHERE_BOX, (8, 8, 8))
        assert_equal(got, want, f"origins x {scale:g}", fallback=lambda n: n > len(far) // 2)
        print(f"origins x {scale:g}: {int(want['hit'].sum())} of {len(far)} hit, {got['stats'][3]} through the fallback")
    # a mesh far from the origin of the coordinates under a fine grid: tau_k alone exceeds a quarter of a cell at every step
    shift = F32(100)
    moved = (verts + shift).astype(F32)
    r = rays.copy()
    r[:, :3] += shift
    box = tuple(np.array(SPHERE_BOX, F32) + shift)
    want = RC.cast(r, moved, faces)
    got = run(api, r, moved, faces, box, (64, 64, 64))
    assert_equal(got, want, "shifted by 100, 64^3", fallback=lambda n: n > 500)
    assert_equal(run(api, r, moved, faces, box, (2, 2, 2)), want, "shifted by 100, 2^3", fallback=0)
    # origins NEAR the origin of the coordinates aimed at that mesh pass the test of the origin; the first step inside the box finds tau_k too large
    shift = F32(300)
    moved, box = (verts + shift).astype(F32), tuple(np.array(SPHERE_BOX, F32) + shift)
    o = np.random.default_rng(4).uniform(-0.01, 0.01, (50, 3))
    aimed = RC.pack(o, (CENTRE + float(shift)) - o)
    want = RC.cast(aimed, moved, faces)
    assert want["hit"].all() and 4 * 2.0 ** -12 * 299 > 1.8 / 16
    got = run(api, aimed, moved, faces, box, (16, 16, 16))
    assert got["n_refs"] > 0, "with no binned face the walk ends after the large list"
    assert_equal(got, want, "tau_k at a step", fallback=50)


def test_the_step_cap_and_a_step_that_does_not_advance(api):
    """The two conditions the far-origin rules leave: both need binned faces (with none the walk ends after the large list)"""
    verts, faces, _, _, _ = sphere_case(1)
    rng = np.random.default_rng(6)
    lo, hi = np.array(SPHERE_BOX[:3]), np.array(SPHERE_BOX[3:])
    small = (rng.uniform(lo + 0.05, hi - 0.05, (200, 1, 3)) + rng.uniform(-0.0005, 0.0005, (200, 3, 3))).astype(F32).reshape(-1, 3)
    mv = np.concatenate([verts, small])
    mf = np.concatenate([faces, (len(verts) + np.arange(600)).reshape(-1, 3).astype(np.int32)])
    # 1024 cells along x under rays that cross all of them above the sphere: the widened box is about 1028 steps long, more than NRF_RC_MAX_STEPS
    o = np.stack([np.full(64, -0.81), np.linspace(-1.0, 0.7, 64), np.full(64, 1.05)], -1)
    rays = np.concatenate([RC.pack(o, np.tile([1.0, 0.0, 0.0], (64, 1))), RC.pack(o + [0, 0, -0.85], np.tile([1.0, 0.0, 0.0], (64, 1)))])
    want = RC.cast(rays, mv, mf)
    assert want["hit"][:64].sum() < 10 and want["hit"][64:].sum() > 30 and (1.8 + 2 * 1.8 / 1024) / (1.8 / 1024) > RC.MAX_STEPS
    got = run(api, rays, mv, mf, SPHERE_BOX, (1024, 1, 1))
    assert got["n_refs"] >= 200
    assert_equal(got, want, "step cap", fallback=lambda n: 50 <= n <= 128)
    # a scene of 2^-18 under directions of 2^127, origins inside the box: dt = h_min / |d|_inf underflows to 0 and no step advances
    s = F32(2.0 ** -18)
    tiny = (verts * s).astype(F32)
    box = tuple(np.array(SPHERE_BOX, F32) * s)
    u = rng.standard_normal((120, 3))
    u /= np.abs(u).max(-1, keepdims=True)
    rays = RC.pack((CENTRE + rng.uniform(-0.3, 0.3, (120, 3))) * float(s), u * 2.0 ** 127)
    with np.errstate(all="ignore"):
        assert F32(float(s) * 1.8 / 64) / F32(2.0 ** 127) == 0 and np.isfinite(rays[:, :6]).all()
    want = RC.cast(rays, tiny, faces)
    got = run(api, rays, tiny, faces, box, (64, 1, 1))
    assert got["n_refs"] > 0 and got["n_large"] == 0
    assert_equal(got, want, "stall", fallback=120)


def test_invalid_faces_of_every_class(api):
    verts, faces, kinds = G.adversarial_mesh()
    rays, _ = RC.mesh_rays(verts[:4], faces[:4], 2, n=100)
    want = RC.cast(rays, verts, faces)
    assert want["stats"].tolist() == [7, 3, 3, 0] and (want["face"] >= 0).sum() > 200
    for box, dims in (((-2, -2, -2, 4, 4, 4), (8, 8, 8)), ((-400, -400, -2, 400, 400, 4), (40, 40, 1)), ((-4e19, -4e19, -4e19, 4e19, 4e19, 4e19), (1, 1, 1))):
        assert_equal(run(api, rays, verts, faces, box, dims), want, f"adversarial, grid {dims}")
    verts, faces = S.dirty()
    rays, _ = RC.mesh_rays(verts[:5], faces[:3], 4, n=100)
    want = RC.cast(rays, verts, faces)
    assert want["stats"].tolist() == [7, 3, 5, 0]
    for dims in ((5, 4, 3), (30, 30, 30)):
        assert_equal(run(api, rays, verts, faces, (-0.5, -1.5, -0.5, 3.5, 2.5, 1.5), dims), want, f"dirty, grid {dims}")


def test_permutation_two_runs_poison_null_outputs_and_a_wider_stride(api):
    verts, faces, rays, _, want = sphere_case(3)
    rays = rays[::2]
    sub = {k: v[::2] for k, v in want.items() if k in ("t", "face", "uv", "point", "hit")}
    perm = np.random.default_rng(5).permutation(len(faces))
    moved = run(api, rays, verts, faces[perm], SPHERE_BOX, (12, 12, 12))
    assert np.array_equal(bits(moved["t"]), bits(sub["t"])), "t does not depend on the order of the faces"
    assert_equal(moved, RC.cast(rays, verts, faces[perm]), "permuted faces")          # Face exact as well: a tie picks the lowest index of THIS order
    hit = np.flatnonzero(sub["face"] >= 0)
    assert (perm[moved["face"][hit]] == sub["face"][hit]).mean() > 0.9, "the same faces but where an exact tie picks the lowest index of another order"
    first = run(api, rays, verts, faces, SPHERE_BOX, (12, 12, 12))
    for pattern in (0xFF, 0x00, 0x5A):
        again = run(api, rays, verts, faces, SPHERE_BOX, (12, 12, 12), pattern=pattern)
        for k in ("t", "face", "uv", "point", "hit", "any", "stats"):
            assert np.array_equal(first[k].view(np.uint32 if first[k].dtype.itemsize == 4 else np.uint8), again[k].view(np.uint32 if again[k].dtype.itemsize == 4 else np.uint8)), (pattern, k)
    assert_equal(first, sub, "12^3")
    for skip in (("uv",), ("point",), ("hit",), ("uv", "point", "hit")):
        got = run(api, rays, verts, faces, SPHERE_BOX, (12, 12, 12), skip=skip)
        assert all(got[{"uv": "uv", "point": "point", "hit": "hit"}[k]] is None for k in skip)
        assert_equal(got, sub, f"without {skip}")
    wide = np.full((len(rays), 11), np.nan, F32)          # the [n, 11] rows of nrf_pack_rays; what follows far is not read
    wide[:, :8] = rays
    assert_equal(run(api, wide, verts, faces, SPHERE_BOX, (12, 12, 12)), sub, "stride 11")


def test_empty_inputs_and_a_grid_of_another_mesh(api):
    lib = api[0].lib()
    verts, faces, rays, _, want = sphere_case(1)
    none = run(api, rays, verts, np.zeros((0, 3), np.int32), SPHERE_BOX, (4, 4, 4))
    assert (none["face"] == -1).all() and np.isinf(none["t"]).all() and (none["uv"] == 0).all() and (none["point"] == 0).all() and (none["hit"] == 0).all()
    assert none["stats"].tolist() == [7, 0, 0, 0] and (none["any"] == 0).all()
    no_verts = run(api, rays, np.zeros((0, 3), F32), faces, SPHERE_BOX, (4, 4, 4))
    assert (no_verts["face"] == -1).all() and no_verts["stats"].tolist() == [7, 0, 0, 0]
    empty = run(api, np.zeros((0, 8), F32), verts, faces, SPHERE_BOX, (4, 4, 4))
    assert len(empty["t"]) == 0 and empty["stats"].tolist() == [0, 0, 0, 0]
    # a grid buffer of another size: refused, nothing written
    g = build_grid(api, verts, faces, SPHERE_BOX, (4, 4, 4))
    other_verts, other_faces, _, _, _ = sphere_case(3)
    big = build_grid(api, other_verts, other_faces, SPHERE_BOX, (4, 4, 4))
    assert big["grid"].numel() != g["grid"].numel()
    dr = dev(rays, F32)
    n = len(rays)
    t, face = torch.full((n,), -7.0, device="cuda"), torch.full((n,), -7, dtype=torch.int32, device="cuda")
    hit = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
    ws = buffer(lib.nrf_ray_cast_workspace_bytes(n), 0x5A)

    def call(grid, nf=g["nf"], mode=0):
        return lib.nrf_ray_cast_mesh(p(dr), n, 8, p(g["dv"]), g["nv"], p(g["df"]), nf, g["box"].ctypes.data, 4, 4, 4, g["n_refs"], g["n_large"], p(grid), grid.numel(), 0, mode,
                                     p(t) if mode == 0 else None, p(face) if mode == 0 else None, None, None, p(hit), None, p(ws), ws.numel(), None)
    assert call(big["grid"]) == INVALID_ARG and lib.nrf_last_error().startswith(b"nrf_ray_cast_mesh")
    torch.cuda.synchronize()
    assert (t == -7).all() and (face == -7).all() and (hit == 77).all() and (ws == 0x5A).all()
    # a buffer of the right size that was built for another face count: the head of the buffer says so, and neither mode writes anything
    for mode in (0, 1):
        assert call(g["grid"], nf=g["nf"] - 1, mode=mode) == 0
        torch.cuda.synchronize()
        assert (t == -7).all() and (face == -7).all() and (hit == 77).all()
    assert call(g["grid"]) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(t), bits(want["t"])) and np.array_equal(face.cpu().numpy(), want["face"]) and np.array_equal(hit.cpu().numpy(), want["hit"])


# ------------------------------------------------------------------------------------ 2. directions and ambient occlusion
def test_hemisphere_directions_equal_the_restatement(api):
    lib = api[0].lib()
    rng = np.random.default_rng(0)
    n = (rng.standard_normal((300, 3)) * 10.0 ** rng.uniform(-3, 3, (300, 1))).astype(F32)
    n[::50] = np.array([[0, 0, 0], [np.nan, 0, 1], [np.inf, 0, 0], [3e19, 3e19, 0], [1e-30, 0, 0], [0, 0, 2]], F32)
    for k, seed, index0 in ((1, 0, 0), (13, 3, 5), (70, 2 ** 63 + 11, 2 ** 40 - 300)):
        want, bad = RC.hemisphere_dirs(n, k, seed, index0)
        out = torch.full((len(n), k, 3), -7.0, device="cuda")
        stats = torch.zeros((4,), dtype=torch.int32, device="cuda")
        dn = dev(n, F32)
        assert lib.nrf_hemisphere_dirs(p(dn), len(n), k, seed, index0, p(out), p(stats), None) == 0, lib.nrf_last_error()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out), bits(want)), (k, seed, index0)
        assert stats.cpu().numpy().tolist() == [bad, 0, 0, 0] and bad == 5
    got = api[1].HemisphereDirections(dev(n, F32), 13, seed=3, index0=5)
    assert np.array_equal(bits(got), bits(RC.hemisphere_dirs(n, 13, 3, 5)[0]))


def ao_case():
    """The level-2 sphere with a floor through it, seen from its vertices along outward normals and from points above the floor: partly occluded"""
    verts, faces = R.octa_sphere(T.SPHERE["centre"], T.SPHERE["radius"], 2)
    mv, mf = RC.floor_mesh(verts, faces, 0.2, 1.2)
    rng = np.random.default_rng(2)
    pts = np.concatenate([verts, np.stack([rng.uniform(-1.1, 1.1, 80), rng.uniform(-1.1, 1.1, 80), np.full(80, 0.2)], -1).astype(F32)])
    nrm = np.concatenate([(verts.astype(np.float64) - CENTRE), np.tile([0.0, 0.0, 3.0], (80, 1))]).astype(F32)
    nrm[5], nrm[9] = 0, np.nan          # bad normals: k invalid rays each
    pts[12, 1] = np.inf
    return mv, mf, pts, nrm


def ambient(api, g, pts, nrm, k, offset, max_dist, seed, index0):
    lib = api[0].lib()
    ao = torch.full((len(pts),), -7.0, device="cuda")
    stats = torch.zeros((4,), dtype=torch.int32, device="cuda")
    ws = buffer(lib.nrf_ray_cast_workspace_bytes(len(pts)), 0x5A)
    dp, dn = dev(pts, F32), dev(nrm, F32)          # held until the call has run
    status = lib.nrf_mesh_ambient_occlusion(p(dp), p(dn), len(pts), k, offset, max_dist, seed, index0, *mesh_args(g), p(ao), p(stats), p(ws), ws.numel(), None)
    assert status == 0, lib.nrf_last_error()
    torch.cuda.synchronize()
    return ao.cpu().numpy(), stats.cpu().numpy().view(np.uint32)


def composed(api, g, pts, nrm, k, offset, max_dist, seed, index0):
    """nrf_hemisphere_dirs, rays packed by torch in the header's order, nrf_ray_cast_mesh in any mode -> (ao, stats)"""
    lib = api[0].lib()
    n = len(pts)
    dn = dev(nrm, F32)
    dirs = torch.empty((n, k, 3), device="cuda")
    assert lib.nrf_hemisphere_dirs(p(dn), n, k, seed, index0, p(dirs), None, None) == 0
    nh = dev(RC.unit_normals(nrm)[0], F32)
    o = dev(pts, F32) + torch.tensor(offset, dtype=torch.float32, device="cuda") * nh
    rays = torch.zeros((n, k, 8), device="cuda")
    rays[..., 0:3], rays[..., 3:6], rays[..., 7] = o[:, None, :], dirs, max_dist
    out = cast_grid(api, g, rays.reshape(-1, 8).cpu().numpy(), 0, 1)
    hits = out["hit"].reshape(n, k).astype(np.int64).sum(1)
    return ((k - hits).astype(F32) / F32(k)).astype(F32), out["stats"]


@pytest.mark.parametrize("k", [16, 70])
def test_the_fused_ambient_occlusion_equals_its_composition_and_the_restatement(api, k):
    mv, mf, pts, nrm = ao_case()
    offset, max_dist, seed, index0 = 1e-3, 0.9, 4, 1000
    want, invalid = RC.ambient_occlusion(pts, nrm, k, offset, max_dist, mv, mf, seed, index0)
    assert invalid == 3 * k and 0.1 < want.mean() < 0.95 and len(np.unique(want)) > 8, "partly occluded"
    box = (-1.3, -1.3, -0.9, 1.3, 1.3, 1.3)
    cases = [(box, (8, 8, 8), 0), (box, (1, 1, 1), 0), (box, (64, 64, 64), None), ((-0.5, -0.5, -0.5, 0.5, 0.5, 0.5), (4, 4, 4), (len(pts) - 3) * k)]
    for b, dims, fallback in cases if k == 16 else cases[:1] + cases[3:]:
        g = build_grid(api, mv, mf, b, dims)
        ao, stats = ambient(api, g, pts, nrm, k, offset, max_dist, seed, index0)
        assert np.array_equal(bits(ao), bits(want)), (dims, np.flatnonzero(bits(ao) != bits(want))[:5])
        two, stats2 = composed(api, g, pts, nrm, k, offset, max_dist, seed, index0)
        assert np.array_equal(bits(two), bits(ao)) and np.array_equal(stats, stats2), (dims, stats, stats2)
        assert stats[0] == invalid and (fallback is None or stats[3] == fallback), (dims, stats)
    # far from the origin of the coordinates every ray of a wave goes through its brute force
    shift = F32(300)
    g = build_grid(api, (mv + shift).astype(F32), mf, tuple(np.array(box, F32) + shift), (32, 32, 32))
    far_want, _ = RC.ambient_occlusion((pts + shift).astype(F32), nrm, k, offset, max_dist, (mv + shift).astype(F32), mf, seed, index0)
    ao, stats = ambient(api, g, (pts + shift).astype(F32), nrm, k, offset, max_dist, seed, index0)
    assert np.array_equal(bits(ao), bits(far_want)) and stats[3] == (len(pts) - 3) * k


def test_ambient_occlusion_is_one_outside_a_convex_sphere_and_zero_inside(api):
    verts, faces = R.octa_sphere(T.SPHERE["centre"], T.SPHERE["radius"], 3)
    out_n = (verts.astype(np.float64) - CENTRE).astype(F32)
    m = api[2].Mesh(dev(verts, F32), dev(faces, np.int32), dev(out_n, F32))
    stats = torch.zeros((4,), dtype=torch.int32, device="cuda")
    ao = api[1].AmbientOcclusion(m, k=64, max_dist=2 * 0.7 + 0.2, stats=stats)
    assert (ao == 1.0).all() and ao.shape == (len(verts),), "nothing lies above a convex surface"
    grid = api[1].FaceGrid(m)
    flipped = api[1].AmbientOcclusion(m, k=64, max_dist=2 * 0.7 + 0.2, grid=grid, at=(m.Vertices, -m.Normals), stats=stats)
    assert (flipped == 0.0).all(), "inside, every ray meets the far side"
    assert stats.cpu().numpy().tolist() == [0, 0, 0, 0]
    # the defaults come from the box diagonal, and slabs agree with the whole
    whole = api[1].AmbientOcclusion(m, k=16, grid=grid, at=(m.Vertices, -m.Normals), seed=3)
    diag = float(np.linalg.norm(grid.Box[3:].astype(np.float64) - grid.Box[:3]))
    same = api[1].AmbientOcclusion(m, k=16, grid=grid, at=(m.Vertices, -m.Normals), seed=3, offset=api[1].AO_OFFSET * diag, max_dist=api[1].AO_MAX_DIST * diag)
    part = api[1].AmbientOcclusion(m, k=16, grid=grid, at=(m.Vertices[100:], -m.Normals[100:]), seed=3, index0=100)
    assert torch.equal(whole, same) and torch.equal(whole[100:], part) and 0 < float(whole.mean()) < 1


def test_bake_ambient_occlusion_equals_the_restatement_on_every_owned_texel(api, tmp_path):
    verts, faces = R.octa_sphere(T.SPHERE["centre"], T.SPHERE["radius"], 1)
    mv, mf = RC.floor_mesh(verts, faces, 0.2, 1.2)
    m = api[2].Mesh(dev(mv, F32), dev(mf, np.int32), torch.zeros((len(mv), 3), device="cuda"))          # vertex normals the bake must not use
    tile, k, offset, max_dist, seed = 8, 16, 2e-3, 0.8, 9
    atlas = api[3].BakeAmbientOcclusion(m, tile=tile, k=k, offset=offset, max_dist=max_dist, seed=seed, chunk_rows=5)
    tex = X.texels(mv, mf, None, tile, 0.0)
    owned = tex["face"] >= 0
    h, w = owned.shape
    pos, nrm = tex["pos"].reshape(-1, 3), (-tex["rays"][..., 3:6]).reshape(-1, 3)
    want, _ = RC.ambient_occlusion(pos, nrm, k, offset, max_dist, mv, mf, seed, 0)
    image = atlas.Image.cpu().numpy()
    assert image.shape == (h, w, 1) and owned.sum() > 300 and (image[~owned] == 0).all() and (atlas.Tile, atlas.NFaces) == (tile, len(mf))
    assert np.array_equal(bits(image[..., 0][owned]), bits(want.reshape(h, w)[owned])) and len(np.unique(image[..., 0][owned])) > 5
    one = api[3].BakeAmbientOcclusion(m, tile=tile, k=k, offset=offset, max_dist=max_dist, seed=seed)
    assert torch.equal(one.Image, atlas.Image), "the atlas does not depend on the slabs"
    # SaveOBJ multiplies it into the written image; without it the files are what they were
    colour = api[3].TextureAtlas(torch.full((h, w, 3), 0.8, device="cuda"), tile, len(mf))
    api[3].SaveOBJ(str(tmp_path / "plain.obj"), m, colour)
    api[3].SaveOBJ(str(tmp_path / "lit.obj"), m, colour, occlusion=atlas)
    plain, lit = (tmp_path / "plain.obj.png").read_bytes(), (tmp_path / "lit.obj.png").read_bytes()
    assert plain == api[3].EncodePNG(api[3].QuantizeTexture(colour.Image)) and lit == api[3].EncodePNG(api[3].QuantizeTexture(colour.Image * atlas.Image))
    assert plain != lit and (tmp_path / "plain.obj").read_text().replace("plain", "lit") == (tmp_path / "lit.obj").read_text()
    with pytest.raises(api[0].NrfError):
        api[3].SaveOBJ(str(tmp_path / "bad.obj"), m, colour, occlusion=colour)


# ------------------------------------------------------------------------------------ 3. the Python layer
def make_mesh(api, verts, faces, **kw):
    v = dev(verts, F32)
    return api[2].Mesh(v, dev(faces, np.int32), torch.zeros_like(v), **kw)


def test_ray_cast_mesh_occluded_visible_and_interpolation(api):
    verts, faces, rays, kinds, want = sphere_case(3)
    colors = (verts @ np.array([[0.3, -0.2, 0.1], [0.1, 0.25, -0.3], [-0.2, 0.1, 0.35]], F32) + np.array([0.5, 0.4, 0.6], F32)).astype(F32)
    m = make_mesh(api, verts, faces, Colors=dev(colors, F32))
    stats = torch.zeros((4,), dtype=torch.int32, device="cuda")
    res = api[1].RayCastMesh(dev(rays, F32), m, stats=stats)
    got = dict(t=res.T.cpu().numpy(), face=res.Face.cpu().numpy(), uv=res.UV.cpu().numpy(), point=res.Points.cpu().numpy(), hit=None, stats=stats.cpu().numpy().view(np.uint32))
    assert_equal(got, want, "RayCastMesh")
    grid = api[1].FaceGrid(m, bbox=SPHERE_BOX, cells=(9, 8, 7))
    s = kinds["outside"]
    pair = api[1].RayCastMesh((dev(rays[s, :3], F32), dev(rays[s, 3:6], F32)), grid, cull="back", points=False)
    assert pair.Points is None and np.array_equal(bits(pair.T), bits(want["t"][s])) and np.array_equal(pair.Face.cpu().numpy(), want["face"][s])
    lim = api[1].RayCastMesh((dev(rays[s, :3], F32), dev(rays[s, 3:6], F32)), grid, near=0.2, far=0.6)
    r2 = rays[s].copy()
    r2[:, 6], r2[:, 7] = 0.2, 0.6
    assert np.array_equal(bits(lim.T), bits(RC.cast(r2, verts, faces)["t"])) and 0 < int((lim.Face >= 0).sum()) < s.stop - s.start
    occ = api[1].Occluded(dev(rays, F32), grid)
    assert occ.dtype == torch.bool and np.array_equal(occ.cpu().numpy(), want["hit"].astype(bool))
    c = api[1].InterpolateAttributes(m, res, "Colors")
    assert np.array_equal(bits(c), bits(CR.interpolate(colors, faces, want["face"], want["uv"]))) and (c[dev(want["face"] < 0, bool)] == 0).all()
    with pytest.raises(api[0].NrfError):
        api[1].RayCastMesh(dev(rays, F32), grid, cull="both")
    with pytest.raises(api[0].NrfError):
        api[1].RayCastMesh(dev(rays[:, :7], F32), grid)
    # Visible: pairs across the sphere are blocked, pairs on one side are not, a pair that touches the surface at its end is not blocked by that surface
    rng = np.random.default_rng(3)
    u = rng.standard_normal((200, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    a, b = (CENTRE + 1.5 * u).astype(F32), (CENTRE - 1.5 * u).astype(F32)
    assert not api[1].Visible(dev(a, F32), dev(b, F32), grid).any()
    assert api[1].Visible(dev(a, F32), dev((CENTRE + 3.0 * u).astype(F32), F32), grid).all()
    cen = verts[faces].astype(np.float64).mean(1)
    outward = cen + 1.0 * (cen - CENTRE) / np.linalg.norm(cen - CENTRE, axis=1, keepdims=True)
    vis = api[1].Visible(dev(outward, F32), dev(cen, F32), grid, eps=1e-3)
    want_vis = ~RC.cast(RC.pack(outward.astype(F32), cen.astype(F32) - outward.astype(F32), near=F32(1e-3), far=F32(1.0 - 1e-3)), verts, faces)["hit"].astype(bool)
    assert np.array_equal(vis.cpu().numpy(), want_vis) and want_vis.all()


def test_clip_rays_to_mesh(api):
    verts, faces, rays, kinds, want = sphere_case(2)
    m = make_mesh(api, verts, faces)
    wide = np.zeros((len(rays), 11), F32)
    wide[:, :8] = rays
    wide[:, 8:] = 0.25
    for miss in ("keep", "empty"):
        got = api[1].ClipRaysToMesh(dev(wide, F32), m, 0.125, miss=miss).cpu().numpy()
        ref = wide.copy()
        ref[:, :8] = RC.clip_rays(rays, want["t"], 0.125, miss)
        assert got.shape == wide.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), miss
    hit = want["hit"].astype(bool)
    assert (got[hit, 7] - got[hit, 6] <= 0.25 + 1e-6).all() and (got[~hit, 6] == 1).all() and (got[~hit, 7] == 0).all() and 100 < hit.sum() < len(rays) - 100
    with pytest.raises(api[0].NrfError):
        api[1].ClipRaysToMesh(dev(wide, F32), m, 0.125, miss="drop")


# The largest relative difference between the depth of tests/raster_ref.py and the T of tests/raycast_ref.py over the pixels both hit, measured on the CPU at this
# size and view (cull none and back alike): 6.406e-04 -- the rasteriser snaps vertices to 1 / 256 of a pixel, which moves the depth of a steep face.  Four times that:
VIEW_DEPTH_MEASURED = 6.406e-4
VIEW_DEPTH_TOL = 4 * VIEW_DEPTH_MEASURED


def test_ray_cast_view_against_render_mesh(api):
    verts, faces = R.octa_sphere(T.SPHERE["centre"], T.SPHERE["radius"], 3)
    m = make_mesh(api, verts, faces)
    h, w, f = 48, 56, 60.0
    K = np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1]], F32)
    pose = np.array([[1, 0, 0, CENTRE[0] + 0.05], [0, 1, 0, CENTRE[1] - 0.03], [0, 0, 1, CENTRE[2] + 2.5]], F32)
    for cull in ("none", "back"):
        ras = api[4].RenderMesh(m, pose, w, h, K, cull=cull, attrs=())
        rc = api[4].RayCastView(m, pose, w, h, K, cull=cull)
        assert rc.DepthMap.shape == (h, w) and rc.FaceMap.shape == (h, w) and rc.BaryMap.shape == (h, w, 3) and rc.AccMap.shape == (h, w)
        rf, cf = ras.FaceMap.cpu().numpy(), rc.FaceMap.cpu().numpy()
        inner = (rf >= 0) & (ras.BaryMap.cpu().numpy().min(-1) > 0.01)
        assert inner.sum() > 800 and np.array_equal(rf[inner], cf[inner]), "the same face wherever the pixel is not on an edge"
        both = (rf >= 0) & (cf >= 0)
        da, db = ras.DepthMap.cpu().numpy().astype(np.float64), rc.DepthMap.cpu().numpy().astype(np.float64)
        rel = (np.abs(da - db)[both] / db[both]).max()
        print(f"cull {cull}: {both.sum()} pixels, largest relative depth difference {rel:.3e} (tolerance {VIEW_DEPTH_TOL:.3e})")
        assert rel <= VIEW_DEPTH_TOL
        assert (rc.AccMap.cpu().numpy() == (cf >= 0)).all() and (db[cf < 0] == 0).all() and np.abs(rc.BaryMap.cpu().numpy().sum(-1)[cf >= 0] - 1).max() < 1e-6
        assert abs(int((rf >= 0).sum()) - int((cf >= 0).sum())) <= 8, "the silhouettes agree but for a few pixels"
    # and the view is the restatement's over the very rays GetRays makes
    from nerfpp_amd.renderer import GetRays
    o, d, _ = GetRays(h, w, K.reshape(9), pose)
    want = RC.cast(RC.pack(o.reshape(-1, 3).cpu().numpy(), d.reshape(-1, 3).cpu().numpy()), verts, faces)
    rc = api[4].RayCastView(m, pose, w, h, K)
    assert np.array_equal(rc.FaceMap.cpu().numpy().reshape(-1), want["face"])
    assert np.array_equal(bits(rc.DepthMap).reshape(-1), bits(np.where(want["face"] >= 0, want["t"], F32(0))))
