"""LeRF relevancy in 3D: PointRelevancy, RelevancyGrid, LocateQuery, VertexRelevancy, SegmentMesh, LatticeComponents and LocateObject over the C ABI
(include/nerfpp_hip.h, lerf_query.hip, components.hip).

The reference reads its language field through rendered images only (LeRFRenderer::Render -> Relevancy).  Here a point set, a lattice or a mesh is labelled by
Relevancy(normalize(le(x)), positive, negatives) of every point -- the formula of nrf_lerf_relevancy -- with LeRF's own density sigma_le beside it.  The fused
precisions never form the 768-wide embedding: ||W a|| comes from the Gram matrix W^T W and the prompt logits from U = W^T q.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .mesh import Mesh, _lattice_points_at, _resolution, _submesh
from .modules import _ptr, _stream, _dev_f32


def _lerf_bbox(lerf_renderer, bbox):
    if bbox is None:
        bbox = lerf_renderer.LangEmbedFn.GetBoundingBox()
    b = torch.as_tensor(bbox).detach().cpu().numpy() if torch.is_tensor(bbox) else bbox
    return np.ascontiguousarray(np.asarray(b, np.float32).reshape(6))


def _relevancy_composed(lerf_renderer, x, positive_id):
    """A LeRFRenderer without a library handle: RunLENetwork (F32) in chunks, normalise, Relevancy -- (rel [p, 2], sigma_le [p])."""
    from .renderer import Relevancy
    pos, neg = lerf_renderer.GetLeRFPrompts()
    if pos is None or neg is None:
        raise L.NrfError("PointRelevancy: no prompts are set (SetLeRFPrompts)")
    p = x.shape[0]
    rel = torch.empty((p, 2), device=x.device, dtype=torch.float32)
    sigma = torch.empty((p,), device=x.device, dtype=torch.float32)
    step = int(lerf_renderer.point_chunk)
    for i in range(0, p, step):
        raw = lerf_renderer.RunLENetwork(x[i:i + step][:, None, :])[:, 0, :]
        sigma[i:i + step] = raw[:, -1]
        e = raw[:, :-1]
        e = e / torch.linalg.vector_norm(e, dim=-1, keepdim=True).clamp_min(1e-8)
        rel[i:i + step] = Relevancy(e.contiguous(), pos, neg, positive_id)
    return rel, sigma


def PointRelevancy(lerf_renderer, pts, positive_id=0, precision=L.NRF_PREC_F16_SPLIT, return_sigma=False, slab_points=None):
    """nrf_lerf_point_relevancy: rel [..., 2] at pts [..., 3] for the renderer's prompts (SetLeRFPrompts); with return_sigma, (rel, sigma_le [...]).
    sigma_le == RunLENetwork(F32)[..., -1] bit for bit in every precision (0 outside the language grid's box)."""
    x = _dev_f32(pts)
    if x.shape[-1] != 3:
        raise L.NrfError(f"PointRelevancy: pts must be [..., 3], got {tuple(x.shape)}")
    lead = tuple(x.shape[:-1])
    x = x.reshape(-1, 3).contiguous()
    p = x.shape[0]
    if p == 0:
        rel, sigma = torch.empty((0, 2), device=x.device, dtype=torch.float32), torch.empty((0,), device=x.device, dtype=torch.float32)
    elif not lerf_renderer._r:
        rel, sigma = _relevancy_composed(lerf_renderer, x, positive_id)
    else:
        lib = L.lib()
        slab = 0 if slab_points is None else int(slab_points)
        rel = torch.empty((p, 2), device=x.device, dtype=torch.float32)
        sigma = torch.empty((p,), device=x.device, dtype=torch.float32) if return_sigma else None
        ws = torch.empty((max(1, int(lib.nrf_lerf_point_relevancy_workspace_bytes(lerf_renderer._r, p, int(precision), slab))),), device=x.device, dtype=torch.uint8)
        L.check(lib.nrf_lerf_point_relevancy(lerf_renderer._r, _ptr(x), p, int(positive_id), int(precision), _ptr(sigma) if sigma is not None else None,
                                             _ptr(rel), slab, _ptr(ws), ws.numel(), _stream()))
    rel = rel.reshape(lead + (2,))
    return (rel, sigma.reshape(lead)) if return_sigma else rel


def RelevancyGrid(lerf_renderer, bbox=None, resolution=256, positive_id=0, precision=L.NRF_PREC_F16_SPLIT, slab_points=None):
    """nrf_lerf_relevancy_grid: (rel [nz, ny, nx, 2], sigma_le [nz, ny, nx]) on the lattice of DensityGrid (P = bmin + i * step, x fastest).  bbox defaults to the
    language grid's box; resolution is an int or (nx, ny, nz)."""
    nx, ny, nz = _resolution(resolution)
    bb = _lerf_bbox(lerf_renderer, bbox)
    dev = torch.device("cuda", torch.cuda.current_device())
    if not lerf_renderer._r:
        from .mesh import _lattice_points
        rel, sigma = PointRelevancy(lerf_renderer, _lattice_points(bb, nx, ny, nz, dev), positive_id, precision, return_sigma=True)
        return rel.reshape(nz, ny, nx, 2), sigma.reshape(nz, ny, nx)
    lib = L.lib()
    slab = 0 if slab_points is None else int(slab_points)
    rel = torch.empty((nz, ny, nx, 2), device=dev, dtype=torch.float32)
    sigma = torch.empty((nz, ny, nx), device=dev, dtype=torch.float32)
    ws = torch.empty((max(1, int(lib.nrf_lerf_relevancy_grid_workspace_bytes(lerf_renderer._r, nx, ny, nz, int(precision), slab))),), device=dev, dtype=torch.uint8)
    L.check(lib.nrf_lerf_relevancy_grid(lerf_renderer._r, bb.ctypes.data_as(C.c_void_p), nx, ny, nz, int(positive_id), int(precision), _ptr(sigma), _ptr(rel), slab,
                                        _ptr(ws), ws.numel(), _stream()))
    return rel, sigma


def LocateQuery(lerf_renderer, bbox=None, resolution=128, sigma_threshold=1.0, top_k=1, positive_id=0, precision=L.NRF_PREC_F16_SPLIT):
    """Where in the scene is the positive prompt: the top_k lattice points of RelevancyGrid by rel[..., 0] among those with sigma_le >= sigma_threshold (ties: the
    lower flat index first).  Returns dict(positions [k, 3], relevancy [k, 2], indices [k] int64 flat indices into [nz, ny, nx]); empty when no point passes."""
    nx, ny, nz = _resolution(resolution)
    bb = _lerf_bbox(lerf_renderer, bbox)
    rel, sigma = RelevancyGrid(lerf_renderer, bb, (nx, ny, nz), positive_id, precision)
    r = rel.reshape(-1, 2)
    idx = torch.nonzero(sigma.reshape(-1) >= sigma_threshold).reshape(-1)
    if idx.numel() and int(top_k) > 0:
        # stable descending sort of the candidates (in ascending index order): equal scores keep the lower index first
        order = torch.sort(r[idx, 0], descending=True, stable=True).indices[:int(top_k)]
        idx = idx[order]
    else:
        idx = idx[:0]
    return dict(positions=_lattice_points_at(bb, nx, ny, nz, idx), relevancy=r[idx], indices=idx.to(torch.int64))


def VertexRelevancy(lerf_renderer, mesh, positive_id=0, precision=L.NRF_PREC_F16_SPLIT):
    """rel [V, 2] at mesh.Vertices (PointRelevancy)."""
    return PointRelevancy(lerf_renderer, mesh.Vertices, positive_id, precision)


def SegmentMesh(mesh, vertex_relevancy, threshold):
    """The sub-mesh of the faces whose three vertices have rel[..., 0] >= threshold; the kept vertices in ascending original order, faces re-indexed.  Normals,
    colours and relevancy follow their vertices (Relevancy = vertex_relevancy).  Any torch device."""
    rel = torch.as_tensor(vertex_relevancy).to(mesh.Vertices.device)
    keep_v = rel.reshape(-1, 2)[:, 0] >= threshold
    faces = mesh.Faces.to(torch.int64)
    keep_f = keep_v[faces].all(dim=1) if faces.numel() else torch.zeros((0,), dtype=torch.bool, device=faces.device)
    return _submesh(mesh, keep_f, rel.reshape(-1, 2))


def LatticeComponents(mask, connectivity=14):
    """nrf_lattice_components: (labels [nz, ny, nx] int32, K) of the set (non-zero) points of mask [nz, ny, nx] (x fastest); -1 where the mask is 0.  connectivity 6,
    14 (the isosurface's Kuhn edges: the components of sigma > iso are the solids whose surfaces Isosurface emits) or 26; neighbours never wrap.  Components are
    numbered 0 .. K-1 by their smallest flat index, so the labels are the same on every run."""
    m = torch.as_tensor(mask)
    if m.dim() != 3:
        raise L.NrfError(f"LatticeComponents: mask must be [nz, ny, nx], got {tuple(m.shape)}")
    dev = m.device if m.is_cuda else torch.device("cuda", torch.cuda.current_device())
    m = (m.to(dev) != 0).to(torch.uint8).contiguous()
    nz, ny, nx = (int(v) for v in m.shape)
    lib = L.lib()
    labels = torch.empty((nz, ny, nx), device=dev, dtype=torch.int32)
    ws = torch.empty((max(1, int(lib.nrf_lattice_components_workspace_bytes(nx, ny, nz))),), device=dev, dtype=torch.uint8)
    k = C.c_int64()
    L.check(lib.nrf_lattice_components(_ptr(m), nx, ny, nz, int(connectivity), _ptr(labels), C.byref(k), _ptr(ws), ws.numel(), _stream()))
    return labels, int(k.value)


def LocateObject(lerf_renderer, bbox=None, resolution=128, sigma_threshold=1.0, relevancy_threshold=0.5, positive_id=0, precision=L.NRF_PREC_F16_SPLIT,
                 connectivity=14):
    """The region the positive prompt points at, not just its best point: of the lattice points of RelevancyGrid with sigma_le >= sigma_threshold and
    rel[..., 0] >= relevancy_threshold (0.5: the positive prompt beats every negative in the pairwise softmax), the connected component (LatticeComponents) of the
    seed, the masked point of highest rel[..., 0] (ties: the lowest flat index -- LocateQuery's rule).  Returns dict(mask [nz, ny, nx] bool, count, seed_index (flat,
    into [nz, ny, nx]), seed_position [3], relevancy [2] of the seed, bbox [6]: the world box of the component's index extents, ready for ExtractMesh(bbox=...)).
    When no point passes: count 0, an empty mask, and None for the rest."""
    nx, ny, nz = _resolution(resolution)
    bb = _lerf_bbox(lerf_renderer, bbox)
    rel, sigma = RelevancyGrid(lerf_renderer, bb, (nx, ny, nz), positive_id, precision)
    mask = (sigma >= sigma_threshold) & (rel[..., 0] >= relevancy_threshold)
    idx = torch.nonzero(mask.reshape(-1)).reshape(-1)
    if idx.numel() == 0:
        return dict(mask=mask, count=0, seed_index=None, seed_position=None, relevancy=None, bbox=None)
    r = rel.reshape(-1, 2)
    seed = idx[torch.sort(r[idx, 0], descending=True, stable=True).indices[0]]          # candidates in ascending index order: equal scores keep the lower index
    labels, _ = LatticeComponents(mask, connectivity)
    comp = labels == labels.reshape(-1)[seed]
    zyx = torch.nonzero(comp)
    lo, hi = zyx.min(dim=0).values, zyx.max(dim=0).values
    corners = torch.stack([(lo[0] * ny + lo[1]) * nx + lo[2], (hi[0] * ny + hi[1]) * nx + hi[2]])
    return dict(mask=comp, count=int(zyx.shape[0]), seed_index=int(seed), seed_position=_lattice_points_at(bb, nx, ny, nz, seed), relevancy=r[seed],
                bbox=_lattice_points_at(bb, nx, ny, nz, corners).reshape(6))
