"""Point clouds: PointBVH, KNearest, EstimateNormals, SurfaceVariation, StatisticalOutliers and RadiusOutliers over the C ABI (include/nerfpp_hip.h "Point
clouds", points.hip).

The reference has no point-cloud tools; the names follow the mirror's style.  A PointBVH is the mesh BVH's build with the point itself as the leaf: no box, no
dims, no host synchronisation and no brute-force fallback for an outlier or a far query.  KNearest returns, per query, the k smallest packed (distance bits, index)
keys in ascending order, so the result depends on neither the tree nor the order of the queries; normals, eigenvalues, scores and statistics are fp64 arithmetic in
a stated order.  tests/points_ref.py equals every output bit for bit and two runs agree.  geometry.NearestPoints takes a PointBVH as its target (k = 1, the grid's
bits) and align.RegisterICP(target_normals=...) runs plane-mode ICP against a cloud.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from .modules import _ptr, _stream, _dev_f32

KNN_MAX_K, JACOBI_SWEEPS = 32, 6          # NRF_KNN_MAX_K, NRF_POINTS_JACOBI_SWEEPS (tests/test_points_host.py holds them to the header)


def _workspace(nbytes, dev):
    return torch.empty((max(1, int(nbytes)),), device=dev, dtype=torch.uint8)


@dataclass
class KNNResult:
    Dist2: torch.Tensor               # [nq, k] f32 squared distances, ascending; +inf in an empty slot
    Index: torch.Tensor               # [nq, k] int32 into the cloud; -1 in an empty slot
    Count: torch.Tensor               # [nq] int32 filled slots


@dataclass
class NormalsResult:
    Normals: torch.Tensor             # [n, 3] f32 unit normals; zeros where the neighbourhood is degenerate
    Eigenvalues: torch.Tensor         # [n, 3] f32 ascending eigenvalues of the neighbourhood's scatter matrix (sums, not divided by its size); zeros where degenerate
    Valid: torch.Tensor               # [n] bool
    Index: Optional[torch.Tensor] = None          # [n, k] int32 the neighbours used


class PointBVH:
    """A bounding-volume hierarchy over the points [n, 3] of a cloud (nrf_point_bvh_build): build it once, query it many times.  No box, no dims and NO host
    synchronisation.  It keeps its buffer and the points alive.  stats: an int32 [4] device tensor whose entry 2 the points with a non-finite coordinate are added to."""

    def __init__(self, points, stats=None):
        self.Points = _dev_f32(points).reshape(-1, 3).contiguous()
        dev, n = self.Points.device, int(self.Points.shape[0])
        lib = L.lib()
        self.Buffer = torch.empty((int(lib.nrf_point_bvh_bytes(n)),), device=dev, dtype=torch.uint8)
        ws = _workspace(lib.nrf_point_bvh_workspace_bytes(n), dev)
        with torch.cuda.device(dev):
            L.check(lib.nrf_point_bvh_build(_ptr(self.Points), n, _ptr(self.Buffer), self.Buffer.numel(), _ptr(stats), _ptr(ws), ws.numel(), _stream()))
        self._box = None

    @property
    def Box(self):
        """[6] f32 on the host, the box of the finite points as the build found it (min xyz, max xyz): ONE host synchronisation at the first use, none before"""
        if self._box is None:
            w = self.Buffer[24:48].cpu().numpy().view(np.uint32).reshape(3, 2)
            self._box = np.concatenate([w[:, 0], w[:, 1]]).view(np.float32)
        return self._box

    def Order(self, points, stride=3):
        """int32 [n]: the rows of `points` ([n, stride] f32, xyz first) in the order of their Morton codes against the cloud's box (nrf_point_bvh_codes and
        nrf_sort_pairs_u32).  What coherent=True passes to KNearest as d_order."""
        n = int(points.shape[0])
        dev = points.device
        lib = L.lib()
        codes = torch.empty((n,), device=dev, dtype=torch.int32)
        L.check(lib.nrf_point_bvh_codes(_ptr(points), n, int(stride), _ptr(self.Buffer), self.Buffer.numel(), int(self.Points.shape[0]), _ptr(codes), _stream()))
        keys, order = torch.empty_like(codes), torch.empty_like(codes)
        ws = _workspace(lib.nrf_sort_workspace_bytes(n), dev)
        L.check(lib.nrf_sort_pairs_u32(_ptr(codes), None, n, 0, 30, _ptr(keys), _ptr(order), _ptr(ws), ws.numel(), _stream()))
        return order


def KNearest(query, target_or_bvh, k, max_dist=None, exclude_self=False, coherent=False, stats=None):
    """For every point of query [nq, 3] its k nearest points of a cloud [n, 3] or its PointBVH -> KNNResult (nrf_bvh_knn): ascending in (distance, index), on an
    exact tie the lower index first; empty slots (+inf, -1) where fewer than k finite points lie within max_dist or the query is not finite.  exclude_self: query i
    IS point i of the cloud and is left out of its own row.  coherent=True serves the queries in the order of their Morton codes (PointBVH.Order), which changes no
    output.  A cloud is built into a PointBVH first; nothing here synchronises.  stats: an int32 [4] device tensor; entry 0 += non-finite queries."""
    k = int(k)
    if not 1 <= k <= KNN_MAX_K:
        raise L.NrfError(f"KNearest: k = {k} (1 .. {KNN_MAX_K})")
    bvh = target_or_bvh if isinstance(target_or_bvh, PointBVH) else PointBVH(target_or_bvh)
    q = _dev_f32(query).reshape(-1, 3).to(bvh.Points.device).contiguous()
    dev, nq = q.device, int(q.shape[0])
    d2 = torch.empty((nq, k), device=dev, dtype=torch.float32)
    idx = torch.empty((nq, k), device=dev, dtype=torch.int32)
    cnt = torch.empty((nq,), device=dev, dtype=torch.int32)
    order = bvh.Order(q) if coherent and nq else None
    with torch.cuda.device(dev):
        L.check(L.lib().nrf_bvh_knn(_ptr(q), nq, _ptr(bvh.Points), int(bvh.Points.shape[0]), _ptr(bvh.Buffer), bvh.Buffer.numel(), _ptr(order), k,
                                    float("inf") if max_dist is None else float(max_dist), int(bool(exclude_self)), _ptr(d2), _ptr(idx), _ptr(cnt), _ptr(stats), None, 0,
                                    _stream()))
    return KNNResult(d2, idx, cnt)


def EstimateNormals(points, k=16, toward=None, bvh=None, coherent=False):
    """Normals and local shape of a cloud [n, 3] from each point's k nearest neighbours (KNearest with exclude_self, then nrf_points_normals: the eigenvector of the
    smallest eigenvalue of the neighbourhood's scatter matrix, fp64, rounded once) -> NormalsResult.  toward: a viewpoint [3] or one per point [n, 3]; normals are
    flipped to face it.  Without, the component of largest magnitude is made positive: a stated sign, NOT a consistent orientation.  bvh: the cloud's PointBVH, where
    one exists already.  Valid is False (and the normal zero) where fewer than 3 points, coincident or collinear points or a non-finite value leave no plane."""
    bvh = PointBVH(points) if bvh is None else bvh
    pts = bvh.Points
    dev, n = pts.device, int(pts.shape[0])
    nn = KNearest(pts, bvh, k, exclude_self=True, coherent=coherent)
    tw, stride = None, 0
    if toward is not None:
        tw = _dev_f32(toward).to(dev).contiguous()
        if tw.numel() == 3:
            tw, stride = tw.reshape(3), 0
        elif tuple(tw.shape) == (n, 3):
            stride = 3
        else:
            raise L.NrfError(f"EstimateNormals: toward must be [3] or [{n}, 3], got {tuple(tw.shape)}")
    normals = torch.empty((n, 3), device=dev, dtype=torch.float32)
    eigen = torch.empty((n, 3), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        L.check(L.lib().nrf_points_normals(_ptr(pts), n, _ptr(nn.Index), int(k), _ptr(tw), stride, _ptr(normals), _ptr(eigen), None, _stream()))
    return NormalsResult(normals, eigen, (normals != 0).any(dim=1), nn.Index)


def SurfaceVariation(result):
    """[n] f32: l0 / (l0 + l1 + l2) of a NormalsResult, 0 on a plane, 1/3 where the neighbourhood has no direction (Pauly et al. 2002); 0 where it is not Valid"""
    e = result.Eigenvalues
    s = e.sum(dim=1)
    return torch.where(s > 0, e[:, 0] / s.clamp(min=torch.finfo(torch.float32).tiny), torch.zeros_like(s))


def ValueStats(values):
    """[4] float64 on the device: count, sum, sum of squares and max(0, largest) over the finite entries of values (nrf_value_stats; an ordered sum, no atomics)"""
    v = _dev_f32(values).reshape(-1).contiguous()
    out = torch.empty((4,), device=v.device, dtype=torch.float64)
    lib = L.lib()
    ws = _workspace(lib.nrf_value_stats_workspace_bytes(v.numel()), v.device)
    with torch.cuda.device(v.device):
        L.check(lib.nrf_value_stats(_ptr(v), v.numel(), _ptr(out), _ptr(ws), ws.numel(), _stream()))
    return out


def MeanNeighborDistance(dist2):
    """[n] f32: the mean distance over the filled slots of each row of a KNNResult.Dist2 (nrf_knn_mean_distance); +inf where a row is empty"""
    d2 = _dev_f32(dist2).contiguous()
    n, k = int(d2.shape[0]), int(d2.shape[1])
    score = torch.empty((n,), device=d2.device, dtype=torch.float32)
    with torch.cuda.device(d2.device):
        L.check(L.lib().nrf_knn_mean_distance(_ptr(d2), n, k, _ptr(score), _stream()))
    return score


def StatisticalOutliers(points, k=16, ratio=2.0, bvh=None):
    """(keep [n] bool, scores [n] f32): a point's score is the mean distance to its k nearest neighbours; it is kept iff score <= mean + ratio * std of the finite
    scores (std = sqrt(max(sum2 / count - mean^2, 0))).  The threshold is formed on the device in float64 from nrf_value_stats: nothing synchronises before the
    caller indexes with the mask.  A point without a neighbour (score +inf) is dropped."""
    bvh = PointBVH(points) if bvh is None else bvh
    nn = KNearest(bvh.Points, bvh, k, exclude_self=True)
    scores = MeanNeighborDistance(nn.Dist2)
    st = ValueStats(scores)
    cnt = st[0].clamp(min=1.0)
    mean = st[1] / cnt
    std = torch.sqrt((st[2] / cnt - mean * mean).clamp(min=0.0))
    return scores.to(torch.float64) <= mean + float(ratio) * std, scores


def RadiusOutliers(points, radius, min_neighbors, bvh=None):
    """keep [n] bool: a point is kept iff at least min_neighbors OTHER points lie within radius of it (KNearest's Count with k = min_neighbors, max_dist = radius)"""
    m = int(min_neighbors)
    if not 1 <= m <= KNN_MAX_K:
        raise L.NrfError(f"RadiusOutliers: min_neighbors = {m} (1 .. {KNN_MAX_K})")
    bvh = PointBVH(points) if bvh is None else bvh
    return KNearest(bvh.Points, bvh, m, max_dist=radius, exclude_self=True).Count >= m
