"""Registering one surface onto another: Transform, TransformMesh, AlignPoints and RegisterICP over the C ABI (include/nerfpp_hip.h "Registration", align.hip).

The reference has no registration; the names follow the mirror's style.  A pose is eight doubles on the device (a unit quaternion, a scale, a translation); one ICP
iteration is apply -> closest point (geometry.ClosestOnMesh on a FaceGrid built once, or geometry.NearestPoints) -> ordered fp64 sums -> a small solve on the
device, all on the current stream.  Nothing in the loop synchronises unless a tolerance is asked for, every sum has a stated order and the solve uses + - * / sqrt
only, so two runs give the same bits and tests/align_ref.py equals every output bit for bit.
"""
import ctypes as C
import dataclasses
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as L
from . import geometry as G
from . import mesh as M
from . import points as P
from .modules import _ptr, _stream, _dev_f32

ALIGN_POINT, ALIGN_PLANE = L.NRF_ALIGN_POINT, L.NRF_ALIGN_PLANE
_METHODS = {"point": ALIGN_POINT, "plane": ALIGN_PLANE}
# NRF_ALIGN_* of the header (tests/test_align_host.py holds them to it)
ALIGN_TILE, POINT_COLUMNS, PLANE_COLUMNS, JACOBI_SWEEPS = 1024, 19, 37, 8
FLAGS = ("ok", "few pairs", "no spread", "bad pivot", "bad scale", "bad rotation")
# the columns of a History row
H_PAIRS, H_RESIDUAL, H_FLAG, H_ANGLE, H_SHIFT, H_DSCALE, H_SCALE = range(7)


def _quat_matrix(q):
    """R of a unit quaternion [4] (w, x, y, z) as a [3, 3] tensor, the header's formula"""
    w, x, y, z = q[0], q[1], q[2], q[3]
    return torch.stack([1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
                        2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
                        2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]).reshape(3, 3)


def _quat_mul(a, b):
    return torch.stack([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                        a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


class Transform:
    """A similarity x -> s R x + t held on the device.  State: [8] float64 (w, x, y, z, s, tx, ty, tz), what the C ABI reads and nrf_align_solve updates.
    Transform(device=...) is the identity; Transform(quaternion=, scale=, translation=) normalises the quaternion (nrf_align_state_init); Transform(state=tensor)
    wraps an existing state."""

    def __init__(self, quaternion=None, scale=1.0, translation=(0.0, 0.0, 0.0), state=None, device="cuda"):
        if state is not None:
            self.State = state.to(dtype=torch.float64).reshape(8).contiguous()
            assert self.State.is_cuda, "the state must live on the GPU (no CPU fallback)"
            return
        self.State = torch.empty((8,), device=device, dtype=torch.float64)
        pose = None
        if quaternion is not None or scale != 1.0 or tuple(translation) != (0.0, 0.0, 0.0):
            q = (1.0, 0.0, 0.0, 0.0) if quaternion is None else tuple(float(v) for v in quaternion)
            pose = (C.c_double * 8)(*q, float(scale), *(float(v) for v in translation))
        with torch.cuda.device(self.State.device):
            L.check(L.lib().nrf_align_state_init(C.addressof(pose) if pose is not None else None, _ptr(self.State), _stream()))

    @property
    def Matrix(self):
        """[4, 4] float64 on the device: [[s R, t], [0, 0, 0, 1]]"""
        s = self.State
        m = torch.zeros((4, 4), device=s.device, dtype=torch.float64)
        m[:3, :3] = s[4] * _quat_matrix(s[:4])
        m[:3, 3] = s[5:8]
        m[3, 3] = 1.0
        return m

    def Apply(self, points, rotate_only=False, out=None):
        """[n, 3] f32 moved through the pose (nrf_align_apply): fp64 arithmetic, rounded to fp32 once.  rotate_only: R alone, for normals.  out may be points."""
        x = _dev_f32(points).reshape(-1, 3)
        y = torch.empty_like(x) if out is None else out
        L.check(L.lib().nrf_align_apply(_ptr(x), int(x.shape[0]), _ptr(self.State), int(bool(rotate_only)), _ptr(y), _stream()))
        return y

    def Inverse(self):
        """The pose that undoes this one: (q*, 1 / s, -(1 / s) R^T t), formed on the device in float64"""
        s = self.State
        q = s[:4] * torch.tensor([1.0, -1.0, -1.0, -1.0], device=s.device, dtype=torch.float64)
        inv = 1.0 / s[4]
        t = -inv * (_quat_matrix(q) @ s[5:8])
        return Transform(state=torch.cat([q, inv.reshape(1), t]))

    def Compose(self, first):
        """The pose that applies `first` and then this one"""
        a, b = self.State, first.State.to(self.State.device)
        q = _quat_mul(a[:4], b[:4])
        q = q / torch.sqrt((q * q).sum())
        t = a[4] * (_quat_matrix(a[:4]) @ b[5:8]) + a[5:8]
        return Transform(state=torch.cat([q, (a[4] * b[4]).reshape(1), t]))


@dataclass
class RegistrationResult:
    Transform: Transform              # source -> target
    History: torch.Tensor             # [iterations run, 8] float64 on the device: pairs kept, sum of squared residuals (point: |p - y|^2, plane: (n.(p - y))^2),
                                      # flag (index into FLAGS), angle of the update, length of its shift, its scale factor, the scale after it, 0


def TransformMesh(mesh, transform):
    """A copy of `mesh` whose Vertices are moved and whose Normals are rotated (not scaled, not renormalised); Faces and every other attribute are the same tensors."""
    new = {"Vertices": transform.Apply(mesh.Vertices)}
    if getattr(mesh, "Normals", None) is not None:
        new["Normals"] = transform.Apply(mesh.Normals, rotate_only=True)
    return dataclasses.replace(mesh, **new)


def _workspace(n, mode, dev):
    return torch.empty((max(1, int(L.lib().nrf_align_workspace_bytes(int(n), mode))),), device=dev, dtype=torch.uint8)


def _sums_solve(y, p, face, mode, scale, grid, state, history, iteration, ws, stats=None, normals=None):
    """One update from the pairs (y, p): the sums, then the solve.  normals [n, 3]: plane mode with the normal of each pair given (nrf_align_sums_normals; `face`
    only says by its sign whether there is a pair), else nrf_align_sums with the faces of `grid`"""
    lib, n = L.lib(), int(y.shape[0])
    if normals is not None:
        L.check(lib.nrf_align_sums_normals(_ptr(y), _ptr(p), _ptr(normals), _ptr(face), n, _ptr(stats), _ptr(ws), ws.numel(), _stream()))
    else:
        verts, faces = (grid.Verts, grid.Faces) if grid is not None else (None, None)
        L.check(lib.nrf_align_sums(_ptr(y), _ptr(p), _ptr(face), n, mode, _ptr(verts), 0 if verts is None else int(verts.shape[0]), _ptr(faces),
                                   0 if faces is None else int(faces.shape[0]), _ptr(stats), _ptr(ws), ws.numel(), _stream()))
    L.check(lib.nrf_align_solve(n, mode, int(bool(scale)), int(iteration), int(history.shape[0]), _ptr(state), _ptr(history), _ptr(ws), ws.numel(), _stream()))


def AlignPoints(src, dst, scale=False):
    """The rigid (scale=True: similarity) fit of src [n, 3] onto dst [n, 3], row i to row i, in the least-squares sense: Horn's closed form, one nrf_align_sums and
    one nrf_align_solve from the identity.  Rows with a non-finite coordinate are left out.  -> RegistrationResult with a one-row History (its flag tells a
    degenerate input: fewer than 3 rows, coincident points)."""
    y, p = _dev_f32(src).reshape(-1, 3), _dev_f32(dst).reshape(-1, 3)
    if y.shape[0] != p.shape[0]:
        raise L.NrfError(f"AlignPoints: {int(y.shape[0])} source and {int(p.shape[0])} target points")
    dev = y.device
    t = Transform(device=dev)
    face = torch.zeros((y.shape[0],), device=dev, dtype=torch.int32)
    history = torch.zeros((1, 8), device=dev, dtype=torch.float64)
    _sums_solve(y, p, face, ALIGN_POINT, scale, None, t.State, history, 0, _workspace(y.shape[0], ALIGN_POINT, dev))
    return RegistrationResult(t, history)


def RegisterICP(source, target, init=None, iterations=30, max_dist=None, method="plane", scale=False, n_points=20000, seed=0, tolerance=None, check_every=5,
                stats=None, coherent=False, target_normals=None):
    """Iterative closest point: the pose that brings `source` onto `target` -> RegistrationResult.
    source: a Mesh (sampled once: SampleSurface(n_points=n_points, seed=seed)) or points [n, 3].  target: a Mesh, a FaceGrid or a MeshBVH (queried through ClosestOnMesh, coherent
    as there; a Mesh is binned once, over the box of its vertices) or points [m, 3] (NearestPoints over the box of the points, method="point" only).
    method "plane" minimises the distance to the tangent plane of the closest face (a few iterations from a start within some tens of degrees), "point" the distance
    to the closest point itself (Horn's closed form per iteration; slower, as a surface slides along itself).  scale=True also fits a uniform scale.
    init: a Transform to start from (default: the identity); it is not modified.  max_dist: pairs farther apart are left out; a scalar or one value per iteration, a
    coarse-to-fine schedule.  Each iteration is apply -> closest -> sums -> solve on the current stream.  tolerance=None synchronises nothing; otherwise the host
    reads the history after every check_every iterations and stops once the last update's angle (radians) and shift are both below the tolerance.
    stats: an int32 [4] device tensor the dropped pairs are added to (no pair within max_dist, non-finite, bad face, face without a normal).
    target_normals: with a target given as points, a [m, 3] tensor of its normals or "estimate" (points.EstimateNormals at its defaults) lets it take
    method="plane": the target is searched through a points.PointBVH built once (no box, no host synchronisation; coherent as KNearest's) and the update comes from
    nrf_align_sums_normals, the plane sums with the matched point's normal.  The sign of a normal changes nothing.  Without it, a cloud takes method="point" only."""
    if method not in _METHODS:
        raise L.NrfError(f"RegisterICP: method must be 'plane' or 'point', got {method!r}")
    mode = _METHODS[method]
    iterations = int(iterations)
    if iterations < 1:
        raise L.NrfError(f"RegisterICP: {iterations} iterations")
    dists = [max_dist] * iterations if max_dist is None or np.isscalar(max_dist) else [float(d) for d in max_dist]
    if len(dists) != iterations:
        raise L.NrfError(f"RegisterICP: {len(dists)} values of max_dist for {iterations} iterations")
    src = G.SampleSurface(source, n_points=n_points, seed=seed).Points if isinstance(source, M.Mesh) else _dev_f32(source).reshape(-1, 3)
    dev, n = src.device, int(src.shape[0])
    grid = points = box = pbvh = normals = None
    if isinstance(target, (M.Mesh, G.FaceGrid, G.MeshBVH)):
        grid = target if isinstance(target, (G.FaceGrid, G.MeshBVH)) else G.FaceGrid(target)
    else:
        if mode != ALIGN_POINT and target_normals is None:
            raise L.NrfError("RegisterICP: method='plane' needs the faces of the target; a target given as points takes method='point'")
        points = _dev_f32(target).reshape(-1, 3).to(dev)
        if target_normals is None:
            box = G._bbox_of(points)
        else:
            if mode != ALIGN_PLANE:
                raise L.NrfError("RegisterICP: target_normals belongs to method='plane'")
            pbvh = P.PointBVH(points)
            if isinstance(target_normals, str):
                if target_normals != "estimate":
                    raise L.NrfError(f"RegisterICP: target_normals must be a [m, 3] tensor or 'estimate', got {target_normals!r}")
                normals = P.EstimateNormals(points, bvh=pbvh).Normals
            else:
                normals = _dev_f32(target_normals).reshape(-1, 3).to(dev)
                if normals.shape[0] != points.shape[0]:
                    raise L.NrfError(f"RegisterICP: {int(normals.shape[0])} target_normals for {int(points.shape[0])} target points")
    state = Transform(device=dev).State if init is None else init.State.to(dev).clone()
    history = torch.zeros((iterations, 8), device=dev, dtype=torch.float64)
    ws = _workspace(n, mode, dev)
    moved = Transform(state=state)
    y = torch.empty_like(src)
    done = iterations
    for it in range(iterations):
        moved.Apply(src, out=y)
        nrm = None
        if grid is not None:
            res = G.ClosestOnMesh(y, grid, max_dist=dists[it], uv=False, coherent=coherent)
            p, face = res.Points, res.Face
        elif pbvh is not None:
            face = P.KNearest(y, pbvh, 1, max_dist=dists[it], coherent=coherent).Index.reshape(-1)
            at = face.clamp(min=0).to(torch.int64)
            p, nrm = (points[at], normals[at]) if points.shape[0] else (torch.zeros_like(y), torch.zeros_like(y))
        else:
            _, face = G.NearestPoints(y, points, max_dist=dists[it], bbox=box)
            p = points[face.clamp(min=0).to(torch.int64)] if points.shape[0] else torch.zeros_like(y)
        _sums_solve(y, p, face, mode, scale, grid, state, history, it, ws, stats, normals=nrm)
        if tolerance is not None and (it + 1) % int(check_every) == 0:
            row = history[it].cpu().numpy()
            if row[H_ANGLE] < tolerance and row[H_SHIFT] < tolerance:
                done = it + 1
                break
    return RegistrationResult(moved, history[:done])
