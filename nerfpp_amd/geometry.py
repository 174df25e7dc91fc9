"""Comparing surfaces in space: SampleSurface, InterpolateAttributes, NearestPoints, FaceGrid, ClosestOnMesh, TransferAttributes and SurfaceDistance over the C ABI
(include/nerfpp_hip.h, geometry.hip).

The reference has no geometry metrics; the names follow the mirror's style.  A Mesh is sampled in proportion to area (every draw a pure function of seed and index),
two point sets are compared through a uniform-grid nearest-neighbour search whose result is the minimum of a packed (distance bits, index) key -- so it depends on
neither the grid nor the order of the points -- and the sums behind Chamfer distance, Hausdorff distance and precision / recall / F-score at a distance are ordered
fp64 reductions.  tests/geometry_ref.py equals every output bit for bit and two runs agree.  That is the sampled point-to-point distance of the DTU / Tanks and Temples
benchmarks; FaceGrid / ClosestOnMesh are the exact point-to-triangle query beside it (the nearest face, the point on it, its barycentrics; tests/closest_ref.py),
which SurfaceDistance(to="surface"), TransferAttributes(source="surface") and texture.BakeTexture(source=<Mesh>) are thin layers over.  RayCastMesh / Occluded /
Visible / HemisphereDirections / AmbientOcclusion / ClipRaysToMesh ask the same FaceGrid what a ray hits (raycast.hip; tests/raycast_ref.py).  MeshBVH is a second
structure for the same two queries (bvh.hip; tests/bvh_ref.py): built without a host synchronisation, no box, dims or fallback, the same bits; every function that
takes a FaceGrid takes it.
"""
import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from . import mesh as M
from .modules import _ptr, _stream, _dev_f32

# NRF_SAMPLE_* / NRF_NN_* / NRF_STATS_* of the header (tests/test_geometry_host.py holds them to it)
SAMPLE_MAX_PER_FACE, NN_MAX_DIM, NN_MAX_CELLS, NN_MAX_RINGS, STATS_MAX_TAU = 65536, 1024, 1 << 26, 16, 4
FG_MAX_FACE_CELLS = 64          # NRF_FG_MAX_FACE_CELLS (tests/test_closest_host.py holds it to the header)
BVH_MAX_DEPTH = 64              # NRF_BVH_MAX_DEPTH (tests/test_bvh_host.py holds it to the header)
OCCUPANCY = 128.0        # what GridDims aims at by default: about 20-30 targets per occupied cell as measured; coarse enough that 16 rings reach far
_ATTRS = ("Colors", "Normals", "Relevancy")


@dataclass
class SurfaceSamples:
    Points: torch.Tensor          # [n, 3] f32
    Faces: torch.Tensor           # [n] int32: the face each point lies on
    UV: torch.Tensor              # [n, 2] f32: the point is (1 - u - v) v0 + u v1 + v v2 of that face
    Area: float                   # the mesh's area (fp64 sum of the fp32 face areas)
    Stats: Optional[torch.Tensor] = None          # [3] int32 on the device: faces with a bad index, with a non-finite vertex or area, clamped to SAMPLE_MAX_PER_FACE


@dataclass
class SurfaceDistanceResult:          # float64 device tensors, as EvaluateViews returns them; a is the prediction, b the truth
    Accuracy: torch.Tensor            # mean distance from a's points to their nearest point of b
    Completeness: torch.Tensor        # mean distance from b's points to their nearest point of a
    Chamfer: torch.Tensor             # the mean of the two
    ChamferSq: torch.Tensor           # mean squared distance a -> b plus mean squared distance b -> a
    Hausdorff: torch.Tensor           # the largest of all those distances
    Precision: torch.Tensor           # [n_tau] the share of a's points within tau of b
    Recall: torch.Tensor              # [n_tau] the share of b's points within tau of a
    FScore: torch.Tensor              # [n_tau] 2 P R / (P + R), 0 where P + R = 0
    Taus: tuple = ()


@dataclass
class ClosestResult:                  # ClosestOnMesh's; InterpolateAttributes takes it as it takes SurfaceSamples
    Dist2: torch.Tensor               # [n] f32 squared distance to the nearest face; +inf where there is none (within max_dist) or the query is not finite
    Face: torch.Tensor                # [n] int32 that face; -1 where there is none
    UV: torch.Tensor                  # [n, 2] f32: the closest point is about (1 - u - v) v0 + u v1 + v v2 of that face; zeros where there is none
    Points: torch.Tensor              # [n, 3] f32 the closest point itself

    @property
    def Faces(self):
        return self.Face


def _mesh_arrays(mesh):
    verts = _dev_f32(mesh.Vertices).reshape(-1, 3)
    faces = mesh.Faces.to(device=verts.device, dtype=torch.int32).reshape(-1, 3).contiguous()
    return verts, faces


def _workspace(nbytes, dev):
    return torch.empty((max(1, int(nbytes)),), device=dev, dtype=torch.uint8)


def _count(verts, faces, density, seed, stats, ws):
    n, area = C.c_int64(0), C.c_double(0.0)
    L.check(L.lib().nrf_mesh_sample_count(_ptr(verts), verts.shape[0], _ptr(faces), faces.shape[0], float(density), int(seed), C.addressof(n), C.addressof(area),
                                          _ptr(stats), _ptr(ws), ws.numel(), _stream()))
    return int(n.value), float(area.value)


def SampleSurface(mesh, n_points=None, density=None, seed=0):
    """Points on `mesh` drawn in proportion to area (nrf_mesh_sample_count / _emit): face f receives floor(area_f * density) points plus one more with the probability
    of the fraction, so the total is ABOUT area * density, not exactly (its standard deviation is below sqrt(area * density)).  Give density (points per unit area) or
    n_points; with n_points one extra count call at density 0 measures the area and density = n_points / area.  Each count call synchronises the stream once."""
    if (n_points is None) == (density is None):
        raise L.NrfError("SampleSurface: give exactly one of n_points and density")
    verts, faces = _mesh_arrays(mesh)
    dev = verts.device
    ws = _workspace(L.lib().nrf_mesh_sample_workspace_bytes(verts.shape[0], faces.shape[0]), dev)
    if density is None:
        _, area = _count(verts, faces, 0.0, seed, None, ws)
        density = float(n_points) / area if area > 0.0 else 0.0
    stats = torch.zeros((3,), device=dev, dtype=torch.int32)
    n, area = _count(verts, faces, density, seed, stats, ws)
    pts = torch.empty((n, 3), device=dev, dtype=torch.float32)
    face = torch.empty((n,), device=dev, dtype=torch.int32)
    uv = torch.empty((n, 2), device=dev, dtype=torch.float32)
    L.check(L.lib().nrf_mesh_sample_emit(_ptr(verts), verts.shape[0], _ptr(faces), faces.shape[0], int(seed), n, _ptr(pts), _ptr(face), _ptr(uv), _ptr(ws), ws.numel(),
                                         _stream()))
    return SurfaceSamples(pts, face, uv, area, stats)


def InterpolateAttributes(mesh, samples, name):
    """[n, C] the attribute `name` of `mesh` (Colors, Normals, Relevancy) at `samples`: (1 - u - v) a0 + u a1 + v a2 of each sample's face."""
    if name not in _ATTRS or getattr(mesh, name) is None:
        raise L.NrfError(f"InterpolateAttributes: the mesh has no {name!r}")
    attr = _dev_f32(getattr(mesh, name))
    a = attr.reshape(attr.shape[0], -1)
    at = samples.Faces.to(torch.int64)
    miss = at < 0 if isinstance(samples, (ClosestResult, RayCastResult)) else None          # a ClosestResult / RayCastResult has -1 where no face was found: zeros there
    f = mesh.Faces.to(device=a.device, dtype=torch.int64)[at if miss is None else at.clamp(min=0)]
    u, v = samples.UV[:, :1], samples.UV[:, 1:]
    out = (1.0 - u - v) * a[f[:, 0]] + u * a[f[:, 1]] + v * a[f[:, 2]]
    if miss is not None:
        out = torch.where(miss[:, None], torch.zeros_like(out), out)
    return out[:, 0] if attr.dim() == 1 else out


def _as_points(x, n_points, seed):
    if isinstance(x, M.Mesh):
        return SampleSurface(x, n_points=n_points, seed=seed).Points
    return _dev_f32(x).reshape(-1, 3)


def GridDims(bbox, n_targets, occupancy=OCCUPANCY):
    """(nx, ny, nz) of the default search grid: cells as cubic as the dims allow whose edge puts about `occupancy` targets into an occupied cell when the targets
    lie on a surface that spans the box (the cells a surface of extent L crosses number about 3 (L / h)^2), never more than 64 cells per target."""
    b = np.asarray(bbox, np.float64).reshape(6)
    ext = np.maximum(b[3:] - b[:3], 1e-30)
    n_long = min(max(math.ceil(math.sqrt(max(n_targets, 1) / (3.0 * occupancy))), 1), NN_MAX_DIM)
    cap = min(NN_MAX_CELLS, max(64 * n_targets, 1))
    while True:
        h = ext.max() / n_long
        dims = [int(min(max(math.ceil(e / h - 1e-9), 1), NN_MAX_DIM)) for e in ext]
        if dims[0] * dims[1] * dims[2] <= cap or n_long == 1:
            return tuple(dims)
        n_long = max(1, int(n_long * 0.8))


def _bbox_of(points):
    """The box of the finite points, widened to a positive extent on every axis: one host synchronisation"""
    p = points[torch.isfinite(points).all(dim=1)]
    if p.shape[0] == 0:
        return np.array([0, 0, 0, 1, 1, 1], np.float32)
    lo, hi = p.min(dim=0).values.cpu().numpy().astype(np.float64), p.max(dim=0).values.cpu().numpy().astype(np.float64)
    pad = np.maximum((hi - lo) * 1e-3, np.maximum(np.abs(hi), np.abs(lo)) * 1e-6 + 1e-30)
    return np.concatenate([lo - pad, hi + pad]).astype(np.float32)


def NearestPoints(query, target, max_dist=None, bbox=None, cells=None, stats=None):
    """For every point of query [nq, 3] its nearest point of target [nt, 3] -> (Dist2 [nq] f32 squared distance, Index [nq] int32 into target): nrf_nearest_points.
    On an exact tie the lowest index; +inf and -1 where the target has no finite point (within max_dist, where given) or the query point is not finite.
    bbox [6] (min xyz, max xyz) is where the search grid lies; points outside it are still found.  bbox=None takes the box of the target, which costs ONE host
    synchronisation; pass the renderer's box (or any box around the target) to avoid it.  cells = (nx, ny, nz) overrides GridDims.  The result depends on neither.
    stats: an int32 [3] device tensor to add {non-finite queries, non-finite targets, queries served by the brute-force fallback} to.
    target may be a points.PointBVH of the cloud: nrf_bvh_knn with k = 1 returns the same bits with no box, no host synchronisation and no fallback (bbox and cells
    are not used; of stats only entry 0 is added to -- the build counted the non-finite targets)."""
    from . import points as P
    if isinstance(target, P.PointBVH):
        res = P.KNearest(query, target, 1, max_dist=max_dist, stats=stats)
        return res.Dist2.reshape(-1), res.Index.reshape(-1)
    q, t = _dev_f32(query).reshape(-1, 3), _dev_f32(target).reshape(-1, 3)
    dev = q.device
    nq, nt = int(q.shape[0]), int(t.shape[0])
    box = _bbox_of(t) if bbox is None else np.ascontiguousarray(torch.as_tensor(bbox).detach().cpu().numpy() if torch.is_tensor(bbox) else bbox, np.float32).reshape(6)
    nx, ny, nz = GridDims(box, nt) if cells is None else (int(c) for c in cells)
    d2 = torch.empty((nq,), device=dev, dtype=torch.float32)
    idx = torch.empty((nq,), device=dev, dtype=torch.int32)
    lib = L.lib()
    ws = _workspace(lib.nrf_nearest_points_workspace_bytes(nq, nt, nx, ny, nz), dev)
    L.check(lib.nrf_nearest_points(_ptr(q), nq, _ptr(t), nt, box.ctypes.data_as(C.c_void_p), nx, ny, nz, float("inf") if max_dist is None else float(max_dist),
                                   _ptr(d2), _ptr(idx), _ptr(stats), _ptr(ws), ws.numel(), _stream()))
    return d2, idx


def _host_box(bbox):
    return np.ascontiguousarray(torch.as_tensor(bbox).detach().cpu().numpy() if torch.is_tensor(bbox) else bbox, np.float32).reshape(6)


class FaceGrid:
    """The faces of `mesh` binned into a uniform grid for ClosestOnMesh (nrf_face_grid_count / _build); build it once, query it many times.  bbox [6] is where the
    grid lies (faces and queries outside it are still found); bbox=None takes the box of the vertices, which costs ONE host synchronisation; the count call costs
    one more.  cells = (nx, ny, nz) overrides GridDims(box, n_faces).  No result depends on either.  The grid keeps its buffer and the mesh's arrays alive.
    stats: an int32 [4] device tensor whose entries 1 and 2 the faces with a corner outside the vertices and with a non-finite vertex are added to."""

    def __init__(self, mesh, bbox=None, cells=None, stats=None):
        self.Mesh = mesh
        self.Verts, self.Faces = _mesh_arrays(mesh)
        dev = self.Verts.device
        nv, nf = int(self.Verts.shape[0]), int(self.Faces.shape[0])
        self.Box = _bbox_of(self.Verts) if bbox is None else _host_box(bbox)
        self.Dims = tuple(GridDims(self.Box, nf)) if cells is None else tuple(int(c) for c in cells)
        nx, ny, nz = self.Dims
        lib = L.lib()
        ws = _workspace(lib.nrf_face_grid_workspace_bytes(nf, nx, ny, nz), dev)
        n_refs, n_large = C.c_int64(0), C.c_int64(0)
        box = self.Box.ctypes.data_as(C.c_void_p)
        L.check(lib.nrf_face_grid_count(_ptr(self.Verts), nv, _ptr(self.Faces), nf, box, nx, ny, nz, C.addressof(n_refs), C.addressof(n_large), _ptr(stats), _ptr(ws),
                                        ws.numel(), _stream()))
        self.NRefs, self.NLarge = int(n_refs.value), int(n_large.value)
        self.Buffer = torch.empty((int(lib.nrf_face_grid_bytes(nf, nx, ny, nz, self.NRefs, self.NLarge)),), device=dev, dtype=torch.uint8)
        L.check(lib.nrf_face_grid_build(_ptr(self.Verts), nv, _ptr(self.Faces), nf, box, nx, ny, nz, self.NRefs, self.NLarge, _ptr(self.Buffer), self.Buffer.numel(),
                                        _ptr(ws), ws.numel(), _stream()))


class MeshBVH:
    """A bounding-volume hierarchy over the faces of `mesh` (nrf_mesh_bvh_build), for every function that takes a FaceGrid: build it once, query it many times.  No
    box, no dims and NO host synchronisation; the results are those of a FaceGrid bit for bit, without a brute-force fallback for far queries, far ray origins or
    faces outside a box.  It keeps its buffer and the mesh's arrays alive.  stats: an int32 [4] device tensor whose entries 1 and 2 the faces with a corner outside
    the vertices and with a non-finite vertex are added to."""

    def __init__(self, mesh, stats=None):
        self.Mesh = mesh
        self.Verts, self.Faces = _mesh_arrays(mesh)
        dev = self.Verts.device
        nv, nf = int(self.Verts.shape[0]), int(self.Faces.shape[0])
        lib = L.lib()
        self.Buffer = torch.empty((int(lib.nrf_mesh_bvh_bytes(nf)),), device=dev, dtype=torch.uint8)
        ws = _workspace(lib.nrf_mesh_bvh_workspace_bytes(nf), dev)
        L.check(lib.nrf_mesh_bvh_build(_ptr(self.Verts), nv, _ptr(self.Faces), nf, _ptr(self.Buffer), self.Buffer.numel(), _ptr(stats), _ptr(ws), ws.numel(), _stream()))
        self._box = None

    @property
    def Box(self):
        """[6] f32 on the host, the box of the valid faces as the build found it (min xyz, max xyz): ONE host synchronisation at the first use, none before"""
        if self._box is None:
            w = self.Buffer[24:48].cpu().numpy().view(np.uint32).reshape(3, 2)
            self._box = np.concatenate([w[:, 0], w[:, 1]]).view(np.float32)
        return self._box

    def Order(self, points, stride=3):
        """int32 [n]: the rows of `points` ([n, stride] f32, xyz first) in the order of their Morton codes against the mesh box (nrf_bvh_point_codes and
        nrf_sort_pairs_u32): neighbours in the list are neighbours in space and walk the same nodes.  What coherent=True passes to the queries as d_order."""
        n = int(points.shape[0])
        dev = points.device
        lib = L.lib()
        codes = torch.empty((n,), device=dev, dtype=torch.int32)
        L.check(lib.nrf_bvh_point_codes(_ptr(points), n, int(stride), _ptr(self.Buffer), self.Buffer.numel(), int(self.Faces.shape[0]), _ptr(codes), _stream()))
        keys, order = torch.empty_like(codes), torch.empty_like(codes)
        ws = _workspace(lib.nrf_sort_workspace_bytes(n), dev)
        L.check(lib.nrf_sort_pairs_u32(_ptr(codes), None, n, 0, 30, _ptr(keys), _ptr(order), _ptr(ws), ws.numel(), _stream()))
        return order


def _bvh_closest(q, bvh, max_dist, stats, uv, points, coherent):
    dev, nq = q.device, int(q.shape[0])
    d2 = torch.empty((nq,), device=dev, dtype=torch.float32)
    face = torch.empty((nq,), device=dev, dtype=torch.int32)
    out_uv = torch.empty((nq, 2), device=dev, dtype=torch.float32) if uv else None
    out_p = torch.empty((nq, 3), device=dev, dtype=torch.float32) if points else None
    order = bvh.Order(q) if coherent and nq else None
    L.check(L.lib().nrf_bvh_closest_on_mesh(_ptr(q), nq, _ptr(bvh.Verts), int(bvh.Verts.shape[0]), _ptr(bvh.Faces), int(bvh.Faces.shape[0]), _ptr(bvh.Buffer),
                                            bvh.Buffer.numel(), _ptr(order), float("inf") if max_dist is None else float(max_dist), _ptr(d2), _ptr(face), _ptr(out_uv),
                                            _ptr(out_p), _ptr(stats), None, 0, _stream()))
    return ClosestResult(d2, face, out_uv, out_p)


def ClosestOnMesh(query, mesh_or_grid, max_dist=None, stats=None, bbox=None, cells=None, uv=True, points=True, coherent=False):
    """For every point of query [nq, 3] the closest point on the surface of a Mesh or its FaceGrid -> ClosestResult (nrf_closest_on_mesh): the nearest face (on an
    exact tie the lowest index), the point on it, its (u, v) and the squared distance; +inf, -1 and zeros where no face lies within max_dist or the query is not
    finite.  A Mesh is binned first (FaceGrid(mesh, bbox, cells): two host synchronisations, one with a bbox); pass a FaceGrid to query the same mesh again without
    either.  uv=False / points=False leave that output out (None).  stats: an int32 [4] device tensor; entry 0 += non-finite queries, entry 3 += queries served by the
    brute-force fallback.  A MeshBVH in place of the FaceGrid gives the same bits (nrf_bvh_closest_on_mesh; entry 3 stays as it is: there is no fallback);
    coherent=True then serves the queries in the order of their Morton codes (MeshBVH.Order), which changes no output."""
    grid = mesh_or_grid if isinstance(mesh_or_grid, (FaceGrid, MeshBVH)) else FaceGrid(mesh_or_grid, bbox=bbox, cells=cells, stats=stats)
    q = _dev_f32(query).reshape(-1, 3).to(grid.Verts.device)
    if isinstance(grid, MeshBVH):
        return _bvh_closest(q.contiguous(), grid, max_dist, stats, uv, points, coherent)
    dev, nq = q.device, int(q.shape[0])
    d2 = torch.empty((nq,), device=dev, dtype=torch.float32)
    face = torch.empty((nq,), device=dev, dtype=torch.int32)
    out_uv = torch.empty((nq, 2), device=dev, dtype=torch.float32) if uv else None
    out_p = torch.empty((nq, 3), device=dev, dtype=torch.float32) if points else None
    lib = L.lib()
    ws = _workspace(lib.nrf_closest_on_mesh_workspace_bytes(nq), dev)
    nx, ny, nz = grid.Dims
    L.check(lib.nrf_closest_on_mesh(_ptr(q), nq, _ptr(grid.Verts), int(grid.Verts.shape[0]), _ptr(grid.Faces), int(grid.Faces.shape[0]),
                                    grid.Box.ctypes.data_as(C.c_void_p), nx, ny, nz, grid.NRefs, grid.NLarge, _ptr(grid.Buffer), grid.Buffer.numel(),
                                    float("inf") if max_dist is None else float(max_dist), _ptr(d2), _ptr(face), _ptr(out_uv), _ptr(out_p), _ptr(stats), _ptr(ws),
                                    ws.numel(), _stream()))
    return ClosestResult(d2, face, out_uv, out_p)


def DistanceStats(dist2, taus=()):
    """[4 + len(taus)] float64 on the device: count, sum of d, sum of d^2, max d and count(d <= tau) over the finite entries of dist2 (nrf_distance_stats)."""
    d2 = _dev_f32(dist2).reshape(-1)
    t = np.ascontiguousarray(taus, np.float32).reshape(-1)
    out = torch.empty((4 + len(t),), device=d2.device, dtype=torch.float64)
    lib = L.lib()
    ws = _workspace(lib.nrf_distance_stats_workspace_bytes(d2.numel()), d2.device)
    L.check(lib.nrf_distance_stats(_ptr(d2), d2.numel(), t.ctypes.data_as(C.c_void_p), len(t), _ptr(out), _ptr(ws), ws.numel(), _stream()))
    return out


def TransferAttributes(src_mesh, dst_mesh, names=("Colors", "Relevancy"), max_dist=None, bbox=None, source="vertex", coherent=False):
    """A copy of dst_mesh whose attributes `names` are those of the nearest vertex of src_mesh (the ones src_mesh carries): TSDF colours onto an isosurface, relevancy
    onto another mesh.  A vertex without a neighbour (within max_dist) gets zeros.  source="surface" takes the attribute at the closest point ON src_mesh instead,
    interpolated over its face (ClosestOnMesh; src_mesh may be a FaceGrid or a MeshBVH, coherent as ClosestOnMesh's): what a coarse mesh needs from a dense one."""
    import dataclasses
    if source not in ("vertex", "surface"):
        raise L.NrfError(f"TransferAttributes: source must be 'vertex' or 'surface', got {source!r}")
    if source == "surface":
        grid = src_mesh if isinstance(src_mesh, (FaceGrid, MeshBVH)) else FaceGrid(src_mesh, bbox=bbox)
        res = ClosestOnMesh(dst_mesh.Vertices, grid, max_dist=max_dist, points=False, coherent=coherent)
        new = {name: InterpolateAttributes(grid.Mesh, res, name) for name in names if getattr(grid.Mesh, name) is not None}
        return dataclasses.replace(dst_mesh, **new)
    _, idx = NearestPoints(dst_mesh.Vertices, src_mesh.Vertices, max_dist=max_dist, bbox=bbox)
    found = idx >= 0
    at = idx.clamp(min=0).to(torch.int64)
    new = {}
    for name in names:
        a = getattr(src_mesh, name)
        if a is None:
            continue
        g = a.to(idx.device)[at]
        new[name] = torch.where(found.reshape((-1,) + (1,) * (g.dim() - 1)), g, torch.zeros_like(g))
    return dataclasses.replace(dst_mesh, **new)


def SurfaceDistance(a, b, taus=(0.01, 0.02, 0.05), n_points=100000, seed=0, max_dist=None, bbox=None, to="points", align=None, coherent=False):
    """How far apart two surfaces are, a the prediction and b the truth, each a Mesh (sampled: SampleSurface(n_points=n_points, seed=seed)) or a [N, 3] tensor of
    points (used as they are).  Returns a SurfaceDistanceResult of float64 device tensors.  With max_dist, points without a neighbour that near are left out of the
    means and count as misses in Precision / Recall.  bbox as in NearestPoints (None: two synchronisations, one per direction).
    to="surface" measures the samples of each side against the FACES of the other where that side is a Mesh (ClosestOnMesh: the exact point-to-triangle distance,
    whose floor is zero, not the other side's sampling density); a side given as points is still searched as points.  A side may also be a MeshBVH (or a FaceGrid)
    of its mesh: it is sampled through its mesh and, with to="surface", searched through the structure as it is (coherent as ClosestOnMesh's).
    align: a nerfpp_amd.align.Transform moves side a into b's frame first (a Mesh through TransformMesh, points through Transform.Apply); "icp" finds that pose with
    align.RegisterICP(a, b) at its defaults (call it yourself for any other setting).  None, the default, measures the two sides as they are."""
    if len(taus) > STATS_MAX_TAU:
        raise L.NrfError(f"SurfaceDistance: {len(taus)} thresholds, at most {STATS_MAX_TAU}")
    if to not in ("points", "surface"):
        raise L.NrfError(f"SurfaceDistance: to must be 'points' or 'surface', got {to!r}")
    if align is not None:
        from . import align as A
        if isinstance(align, str) and align != "icp":
            raise L.NrfError(f"SurfaceDistance: align must be None, 'icp' or a Transform, got {align!r}")
        pose = A.RegisterICP(a, b, method="plane" if isinstance(b, (M.Mesh, FaceGrid, MeshBVH)) else "point").Transform if isinstance(align, str) else align
        if isinstance(a, (FaceGrid, MeshBVH)):
            a = a.Mesh          # a moved mesh needs a structure of its own
        a = A.TransformMesh(a, pose) if isinstance(a, M.Mesh) else pose.Apply(a)
    pa, pb = (_as_points(x.Mesh if isinstance(x, (FaceGrid, MeshBVH)) else x, n_points, seed) for x in (a, b))

    def dist2(p, other, other_points):
        if to == "surface" and isinstance(other, (M.Mesh, FaceGrid, MeshBVH)):
            return ClosestOnMesh(p, other, max_dist=max_dist, bbox=bbox, uv=False, points=False, coherent=coherent).Dist2
        return NearestPoints(p, other_points, max_dist=max_dist, bbox=bbox)[0]
    sa = DistanceStats(dist2(pa, b, pb), taus)
    sb = DistanceStats(dist2(pb, a, pa), taus)
    acc, comp = sa[1] / sa[0], sb[1] / sb[0]
    # tensor / tensor: a division by a Python scalar is carried out as a multiplication by its reciprocal, which is not the correctly rounded quotient
    na, nb = (torch.full((), float(x.shape[0]), device=sa.device, dtype=torch.float64) for x in (pa, pb))
    p, r = sa[4:] / na, sb[4:] / nb
    f = torch.where(p + r > 0, 2.0 * p * r / (p + r), torch.zeros_like(p))
    return SurfaceDistanceResult(acc, comp, 0.5 * (acc + comp), sa[2] / sa[0] + sb[2] / sb[0], torch.maximum(sa[3], sb[3]), p, r, f, tuple(float(t) for t in taus))


# ---------------------------------------------------------------------------------------------- ray casting (include/nerfpp_hip.h "Ray casting on a mesh", raycast.hip)
RC_CLOSEST, RC_ANY = 0, 1
RC_CULL = {"none": 0, "back": 1, "front": 2}
RC_TAU_LOG2, RC_MAX_STEPS, RC_MAX_STRIDE = -12, 1024, 64         # NRF_RC_* / NRF_HEMI_* of the header (tests/test_raycast_host.py holds them to it)
HEMI_ATTEMPTS, HEMI_MAX_K, HEMI_MAX_INDEX, HEMI_MIN_LEN2 = 8, 65536, 1 << 40, 2.0 ** -20
AO_OFFSET, AO_MAX_DIST = 1e-3, 0.25          # AmbientOcclusion's defaults as shares of the box diagonal


@dataclass
class RayCastResult:                  # RayCastMesh's; InterpolateAttributes takes it as it takes a ClosestResult
    T: torch.Tensor                   # [n] f32 the ray parameter of the first hit in units of d (the renderer's z); +inf on a miss or an invalid ray
    Face: torch.Tensor                # [n] int32 the face hit; -1 on a miss
    UV: Optional[torch.Tensor]        # [n, 2] f32: the hit is about (1 - u - v) v0 + u v1 + v v2 of that face; zeros on a miss
    Points: Optional[torch.Tensor]    # [n, 3] f32 the surface point itself

    @property
    def Faces(self):
        return self.Face


def _as_grid(mesh_or_grid, stats=None):
    return mesh_or_grid if isinstance(mesh_or_grid, (FaceGrid, MeshBVH)) else FaceGrid(mesh_or_grid, stats=stats)


def _packed_rays(rays, near, far, dev, who):
    """rays: packed rows [n, >= 8] (o, d, near, far, ...; their own ranges are kept) or a pair (origins [n, 3], dirs [n, 3]) packed here with near / far"""
    if isinstance(rays, (tuple, list)):
        o, d = (_dev_f32(x).reshape(-1, 3).to(dev) for x in rays)
        if o.shape[0] != d.shape[0]:
            raise L.NrfError(f"{who}: {int(o.shape[0])} origins and {int(d.shape[0])} directions")
        r = torch.empty((o.shape[0], 8), device=dev, dtype=torch.float32)
        r[:, 0:3], r[:, 3:6] = o, d
        r[:, 6] = torch.as_tensor(near, dtype=torch.float32, device=dev)
        r[:, 7] = torch.as_tensor(far, dtype=torch.float32, device=dev)
        return r
    r = _dev_f32(rays).to(dev)
    if r.dim() != 2 or not 8 <= r.shape[1] <= RC_MAX_STRIDE:
        raise L.NrfError(f"{who}: packed rays are [n, 8 .. {RC_MAX_STRIDE}] (o, d, near, far, ...), got {tuple(r.shape)}")
    return r.contiguous()


def _ray_cast(who, rays, grid, cull, mode, uv, points, stats, coherent=False):
    if cull not in RC_CULL:
        raise L.NrfError(f"{who}: cull must be one of {sorted(RC_CULL)}, got {cull!r}")
    dev, n = rays.device, int(rays.shape[0])
    closest = mode == RC_CLOSEST
    t = torch.empty((n,), device=dev, dtype=torch.float32) if closest else None
    face = torch.empty((n,), device=dev, dtype=torch.int32) if closest else None
    out_uv = torch.empty((n, 2), device=dev, dtype=torch.float32) if closest and uv else None
    out_p = torch.empty((n, 3), device=dev, dtype=torch.float32) if closest and points else None
    hit = None if closest else torch.empty((n,), device=dev, dtype=torch.uint8)
    lib = L.lib()
    if isinstance(grid, MeshBVH):
        order = grid.Order(rays, int(rays.shape[1])) if coherent and n else None          # by the rays' origins
        L.check(lib.nrf_bvh_ray_cast_mesh(_ptr(rays), n, int(rays.shape[1]), _ptr(grid.Verts), int(grid.Verts.shape[0]), _ptr(grid.Faces), int(grid.Faces.shape[0]),
                                          _ptr(grid.Buffer), grid.Buffer.numel(), _ptr(order), RC_CULL[cull], mode, _ptr(t), _ptr(face), _ptr(out_uv), _ptr(out_p),
                                          _ptr(hit), _ptr(stats), None, 0, _stream()))
        return t, face, out_uv, out_p, hit
    ws = _workspace(lib.nrf_ray_cast_workspace_bytes(n), dev)
    nx, ny, nz = grid.Dims
    L.check(lib.nrf_ray_cast_mesh(_ptr(rays), n, int(rays.shape[1]), _ptr(grid.Verts), int(grid.Verts.shape[0]), _ptr(grid.Faces), int(grid.Faces.shape[0]),
                                  grid.Box.ctypes.data_as(C.c_void_p), nx, ny, nz, grid.NRefs, grid.NLarge, _ptr(grid.Buffer), grid.Buffer.numel(), RC_CULL[cull], mode,
                                  _ptr(t), _ptr(face), _ptr(out_uv), _ptr(out_p), _ptr(hit), _ptr(stats), _ptr(ws), ws.numel(), _stream()))
    return t, face, out_uv, out_p, hit


def RayCastMesh(rays, mesh_or_grid, near=0.0, far=float("inf"), cull="none", uv=True, points=True, stats=None, coherent=False):
    """The first face every ray hits on a Mesh or its FaceGrid -> RayCastResult (nrf_ray_cast_mesh, closest mode).  rays: the library's packed rows [n, >= 8]
    (o, d, near, far, ...: what BatchifyRays and AtlasTexels use; each row's own range holds and near / far here are ignored) or a pair (origins, dirs) with near / far
    scalars or [n].  d is not normalised and T is in units of d, the renderer's z.  The range is [max(near, 0), far]; on an exact tie in T the lowest face index;
    +inf, -1 and zeros on a miss, an empty range or an invalid ray.  cull: "none", "back" (only faces counter-clockwise seen from the origin, RenderMesh's "back") or
    "front".  A Mesh is binned first (FaceGrid(mesh): two host synchronisations); pass a FaceGrid to cast again without them.  A grid whose box does not hold the
    mesh is still exact, through the brute-force fallback.  stats: an int32 [4] device tensor; entry 0 += invalid rays, entry 3 += rays served by the fallback.
    A MeshBVH in place of the FaceGrid gives the same bits without any fallback (nrf_bvh_ray_cast_mesh); coherent=True then serves the rays in the order of the
    Morton codes of their origins, which changes no output."""
    grid = _as_grid(mesh_or_grid, stats)
    r = _packed_rays(rays, near, far, grid.Verts.device, "RayCastMesh")
    t, face, out_uv, out_p, _ = _ray_cast("RayCastMesh", r, grid, cull, RC_CLOSEST, uv, points, stats, coherent)
    return RayCastResult(t, face, out_uv, out_p)


def Occluded(rays, mesh_or_grid, near=0.0, far=float("inf"), cull="none", stats=None, coherent=False):
    """[n] bool: whether a ray hits anything within its range (nrf_ray_cast_mesh, any mode: the walk stops at the first face it meets).  Arguments as RayCastMesh's;
    the answer equals isfinite(RayCastMesh(...).T)."""
    grid = _as_grid(mesh_or_grid, stats)
    r = _packed_rays(rays, near, far, grid.Verts.device, "Occluded")
    return _ray_cast("Occluded", r, grid, cull, RC_ANY, False, False, stats, coherent)[4].to(torch.bool)


def Visible(points_a, points_b, mesh_or_grid, eps=1e-4, stats=None, coherent=False):
    """[n] bool: whether the segment from points_a[i] to points_b[i] is free of the mesh.  The ray is o = a, d = b - a with the range [eps, 1 - eps] in units of the
    segment's length, so a segment that starts or ends ON the surface is not blocked by that very surface.  A pair that coincides (d = 0) or is not finite is an
    invalid ray, a miss: reported visible and counted in stats[0]."""
    grid = _as_grid(mesh_or_grid, stats)
    dev = grid.Verts.device
    a, b = _dev_f32(points_a).reshape(-1, 3).to(dev), _dev_f32(points_b).reshape(-1, 3).to(dev)
    return ~Occluded((a, b - a), grid, near=float(eps), far=1.0 - float(eps), stats=stats, coherent=coherent)


def HemisphereDirections(normals, k, seed=0, index0=0, stats=None):
    """[n, k, 3] f32 unit directions around each normal, distributed by the cosine law (nrf_hemisphere_dirs): direction j of normal i is a pure function of
    (seed, index0 + i, j), so a slab of a longer list draws what the whole list would.  A zero or non-finite normal gives zeros and is counted in stats[0]."""
    nrm = _dev_f32(normals).reshape(-1, 3)
    n = int(nrm.shape[0])
    dirs = torch.empty((n, int(k), 3), device=nrm.device, dtype=torch.float32)
    L.check(L.lib().nrf_hemisphere_dirs(_ptr(nrm), n, int(k), int(seed), int(index0), _ptr(dirs), _ptr(stats), _stream()))
    return dirs


def _box_diagonal(box):
    b = np.asarray(box, np.float64)
    return float(np.linalg.norm(b[3:] - b[:3]))


def AmbientOcclusion(mesh, k=64, max_dist=None, offset=None, seed=0, grid=None, at=None, index0=0, stats=None):
    """[n] f32 in [0, 1]: the share of k cosine-weighted rays that leave each point unoccluded (nrf_mesh_ambient_occlusion: directions and walk fused, no ray is
    written); 1 is open sky.  The points are the vertices of `mesh` with mesh.Normals, or at = (points [n, 3], normals [n, 3]).  Ray j of point i starts
    `offset` above the point along its unit normal and is `max_dist` long; the defaults are AO_OFFSET = 1e-3 and AO_MAX_DIST = 0.25 of the diagonal of the grid's
    box: above the rounding of a hit's own surface, and the reach within which a wall darkens a corner.  grid: a FaceGrid of the occluding mesh (default:
    FaceGrid(mesh), two host synchronisations).  The value is an integer count over k, so it is exact; (seed, index0 + i, j) decide a direction, so slabs agree with
    the whole.  A point with a zero or non-finite normal gets 1 and its k rays are counted in stats[0]; stats[3] += rays served by the fallback.
    grid=<MeshBVH>: the composition the header states equal to the fused call, HemisphereDirections and the BVH's any-hit cast slab by slab (the rays of a slab are
    written); the default offset and max_dist then read the mesh box from the tree's head, one host synchronisation (pass both to avoid it)."""
    grid = FaceGrid(mesh, stats=stats) if grid is None else grid
    dev = grid.Verts.device
    if at is None:
        if mesh.Normals is None:
            raise L.NrfError("AmbientOcclusion: the mesh has no Normals (mesh.VertexNormals gives them), and no at=(points, normals) was passed")
        pts, nrm = mesh.Vertices, mesh.Normals
    else:
        pts, nrm = at
    pts, nrm = _dev_f32(pts).reshape(-1, 3).to(dev), _dev_f32(nrm).reshape(-1, 3).to(dev)
    if pts.shape[0] != nrm.shape[0]:
        raise L.NrfError(f"AmbientOcclusion: {int(pts.shape[0])} points and {int(nrm.shape[0])} normals")
    diag = _box_diagonal(grid.Box)
    off = AO_OFFSET * diag if offset is None else float(offset)
    md = AO_MAX_DIST * diag if max_dist is None else float(max_dist)
    n = int(pts.shape[0])
    if isinstance(grid, MeshBVH):
        return _bvh_ambient_occlusion(pts, nrm, int(k), off, md, int(seed), int(index0), grid, stats)
    ao = torch.empty((n,), device=dev, dtype=torch.float32)
    lib = L.lib()
    ws = _workspace(lib.nrf_ray_cast_workspace_bytes(n), dev)
    nx, ny, nz = grid.Dims
    L.check(lib.nrf_mesh_ambient_occlusion(_ptr(pts), _ptr(nrm), n, int(k), off, md, int(seed), int(index0), _ptr(grid.Verts), int(grid.Verts.shape[0]), _ptr(grid.Faces),
                                           int(grid.Faces.shape[0]), grid.Box.ctypes.data_as(C.c_void_p), nx, ny, nz, grid.NRefs, grid.NLarge, _ptr(grid.Buffer),
                                           grid.Buffer.numel(), _ptr(ao), _ptr(stats), _ptr(ws), ws.numel(), _stream()))
    return ao


AO_SLAB_RAYS = 1 << 22          # rays of one slab of the composed ambient occlusion: 128 MiB of packed rows


def _bvh_ambient_occlusion(pts, nrm, k, offset, max_dist, seed, index0, bvh, stats):
    """nrf_mesh_ambient_occlusion's rays, formed as its header states them and cast through the BVH in any mode.  n-hat = n / sqrtf((nx*nx + ny*ny) + nz*nz) and
    o = p + offset * n-hat in single fp32 tensor operations, each rounded once as the kernel's are"""
    n, dev = int(pts.shape[0]), pts.device
    if not max_dist >= 0.0:
        raise L.NrfError(f"AmbientOcclusion: max_dist must be >= 0 or +inf (got {max_dist})")
    if not math.isfinite(offset):
        raise L.NrfError(f"AmbientOcclusion: offset must be finite (got {offset})")
    ao = torch.empty((n,), device=dev, dtype=torch.float32)
    kf = torch.full((), float(k), device=dev, dtype=torch.float32)
    off = torch.full((), offset, device=dev, dtype=torch.float32)
    per = max(1, AO_SLAB_RAYS // k)
    for i0 in range(0, n, per):
        p, nr = pts[i0:i0 + per], nrm[i0:i0 + per]
        m = int(p.shape[0])
        l2 = (nr[:, 0] * nr[:, 0] + nr[:, 1] * nr[:, 1]) + nr[:, 2] * nr[:, 2]
        ok = torch.isfinite(nr).all(dim=1) & (l2 > 0) & torch.isfinite(l2)
        nh = torch.where(ok[:, None], nr / torch.sqrt(torch.where(ok, l2, torch.ones_like(l2)))[:, None], torch.zeros_like(nr))
        rays = torch.zeros((m, k, 8), device=dev, dtype=torch.float32)
        rays[:, :, 0:3] = (p + off * nh)[:, None, :]
        rays[:, :, 3:6] = HemisphereDirections(nr, k, seed=seed, index0=index0 + i0)
        rays[:, :, 7] = max_dist
        hit = _ray_cast("AmbientOcclusion", rays.reshape(-1, 8), bvh, "none", RC_ANY, False, False, stats)[4]
        hits = hit.reshape(m, k).sum(dim=1, dtype=torch.int32)
        ao[i0:i0 + per] = (k - hits).to(torch.float32) / kf
    return ao


def ClipRaysToMesh(rays, mesh_or_grid, band, miss="keep", cull="none", stats=None, coherent=False):
    """A copy of the packed rays [n, >= 8] whose ranges are narrowed around the mesh: on a hit at T, near = max(near, T - band) and far = min(far, T + band); on a miss
    the range is kept (miss="keep") or made empty (miss="empty": near 1, far 0).  band is in units of T, that is of each ray's own d (world units where d is a unit
    vector; BatchifyRays' z otherwise).  The result feeds BatchifyRays as it is: a mesh extracted at one iteration narrows the sampling of every later render."""
    if miss not in ("keep", "empty"):
        raise L.NrfError(f"ClipRaysToMesh: miss must be 'keep' or 'empty', got {miss!r}")
    if isinstance(rays, (tuple, list)):
        raise L.NrfError("ClipRaysToMesh: pass packed rays [n, >= 8]; a pair of origins and directions has no range to narrow")
    grid = _as_grid(mesh_or_grid, stats)
    r = _packed_rays(rays, 0.0, 0.0, grid.Verts.device, "ClipRaysToMesh")
    t = _ray_cast("ClipRaysToMesh", r, grid, cull, RC_CLOSEST, False, False, stats, coherent)[0]
    out = r.clone()
    hit = torch.isfinite(t)
    b = torch.as_tensor(band, dtype=torch.float32, device=r.device)
    near, far = torch.maximum(r[:, 6], t - b), torch.minimum(r[:, 7], t + b)
    if miss == "empty":
        out[:, 6] = torch.where(hit, near, torch.ones_like(near))
        out[:, 7] = torch.where(hit, far, torch.zeros_like(far))
    else:
        out[:, 6] = torch.where(hit, near, r[:, 6])
        out[:, 7] = torch.where(hit, far, r[:, 7])
    return out
