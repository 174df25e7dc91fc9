"""Looking at a mesh from a camera: RenderMesh, RenderMeshView, VisibleFaces, FilterVisible and EvaluateMesh over the C ABI (include/nerfpp_hip.h, raster.hip).

The reference has no rasteriser; the names follow the mirror's style.  nrf_raster_mesh is a deterministic z-buffer of the project's own Mesh through the project's own
camera (the inverse of GetRays, the projection TSDFVolume.Integrate uses): depth in the unit of DepthMap / AccMap, the face every pixel sees, its barycentrics and the
perspective-correct interpolation of the vertex attributes.  Coverage is exact integer arithmetic and the depth a stated fp32 operation order, so
tests/raster_ref.py equals every output bit for bit, two runs agree, and the order of the face list does not matter.
"""
import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from . import mesh as M
from .dataset import _k9, _m12
from .modules import _ptr, _stream, _dev_f32

SUBPIXEL, GUARD, MAX_ATTR, WIDE_PIXELS = 256, 16384, 8, 256          # NRF_RASTER_* of the header (tests/test_raster_host.py holds them to it)
_CULL = {"none": 0, "back": 1}
_ATTRS = ("Colors", "Normals", "Relevancy")


@dataclass
class MeshRender:
    DepthMap: torch.Tensor                       # [H, W] f32: the ray parameter of GetRays' directions at the surface, 0 where no face is seen
    AccMap: torch.Tensor                         # [H, W] f32: 1 on a hit, 0 elsewhere (DepthMap / AccMap reads like a render's)
    FaceMap: torch.Tensor                        # [H, W] int32: the index of the face seen, -1 where none
    BaryMap: torch.Tensor                        # [H, W, 3] f32: screen-space barycentrics b0, b1, b2 of the pixel centre in that face
    RGBMap: Optional[torch.Tensor] = None        # [H, W, 3] from Mesh.Colors
    NormalMap: Optional[torch.Tensor] = None     # [H, W, 3] from Mesh.Normals, re-normalised
    RelevancyMap: Optional[torch.Tensor] = None  # [H, W, 2] (or [H, W]) from Mesh.Relevancy
    Stats: Optional[torch.Tensor] = None         # [4] int32 on the device: faces drawn, clipped, degenerate or culled, with a bad index


def RenderMesh(mesh, pose, W, H, K, near=1e-3, cull="none", attrs=_ATTRS):
    """nrf_raster_mesh of `mesh` from `pose` ([3|4, 4] camera-to-world) through K at W x H (argument order as RenderView's).  cull: "none" draws both sides, "back" only
    the faces seen from outside.  attrs: which of Colors, Normals, Relevancy to interpolate where the mesh carries them; they travel as one [V, C] array in one call.
    No host synchronisation."""
    if cull not in _CULL:
        raise L.NrfError(f"RenderMesh: cull must be one of {sorted(_CULL)}, got {cull!r}")
    unknown = [a for a in attrs if a not in _ATTRS]
    if unknown:
        raise L.NrfError(f"RenderMesh: unknown attributes {unknown} (of {list(_ATTRS)})")
    verts = _dev_f32(mesh.Vertices).reshape(-1, 3)
    faces = mesh.Faces.to(device=verts.device, dtype=torch.int32).reshape(-1, 3).contiguous()
    nv, nf, h, w = int(verts.shape[0]), int(faces.shape[0]), int(H), int(W)
    cols = [(a, _dev_f32(getattr(mesh, a)).reshape(nv, -1)) for a in _ATTRS if a in attrs and getattr(mesh, a) is not None]
    n_attr = sum(int(c.shape[1]) for _, c in cols)
    if n_attr > MAX_ATTR:
        raise L.NrfError(f"RenderMesh: {n_attr} attribute channels, at most {MAX_ATTR}")
    attr = torch.cat([c for _, c in cols], dim=1).contiguous() if n_attr else None
    dev = verts.device
    depth = torch.empty((h, w), device=dev, dtype=torch.float32)
    face = torch.empty((h, w), device=dev, dtype=torch.int32)
    bary = torch.empty((h, w, 3), device=dev, dtype=torch.float32)
    out = torch.empty((h, w, n_attr), device=dev, dtype=torch.float32) if n_attr else None
    stats = torch.zeros((4,), device=dev, dtype=torch.int32)          # the uint32 counts of one call are at most F < 2^31
    lib = L.lib()
    ws = torch.empty((max(1, int(lib.nrf_raster_workspace_bytes(nv, nf, h, w))),), device=dev, dtype=torch.uint8)
    k, m = _k9(K), _m12(pose)
    L.check(lib.nrf_raster_mesh(_ptr(verts), nv, _ptr(faces), nf, _ptr(attr), n_attr, h, w, k.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p), float(near),
                                _CULL[cull], _ptr(depth), _ptr(face), _ptr(bary), _ptr(out), _ptr(stats), _ptr(ws), ws.numel(), _stream()))
    res = MeshRender(depth, (face >= 0).to(torch.float32), face, bary, Stats=stats)
    at = 0
    for name, c in cols:
        n = int(c.shape[1])
        img = out[..., at:at + n]
        at += n
        if name == "Colors":
            res.RGBMap = img.contiguous()
        elif name == "Normals":
            res.NormalMap = M._safe_normalize(img)
        else:
            res.RelevancyMap = (img[..., 0] if getattr(mesh, name).dim() == 1 else img).contiguous()
    return res


def RayCastView(mesh, pose, W, H, K, near=0.0, far=float("inf"), cull="none", stats=None):
    """The view of RenderMesh by ray casting: GetRays(H, W, K, pose) through geometry.RayCastMesh (mesh: a Mesh or its geometry.FaceGrid) -> MeshRender with DepthMap,
    AccMap, FaceMap and BaryMap in RenderMesh's units (the depth is the ray parameter of GetRays' directions, 0 where nothing is hit), so the two can be compared
    pixel for pixel.  They are two definitions that round differently: the rasteriser decides coverage in integer sub-pixels and interpolates 1 / z, the ray cast
    intersects in space, so faces can differ along silhouettes and shared edges, and BaryMap here holds the SURFACE barycentrics (1 - u - v, u, v) of the hit, not
    the screen-space ones.  Unlike the rasteriser it has no near plane or guard band and sees faces behind other cameras' clip limits."""
    from . import geometry as G
    from .renderer import GetRays
    grid = mesh if isinstance(mesh, (G.FaceGrid, G.MeshBVH)) else G.FaceGrid(mesh, stats=stats)
    h, w = int(H), int(W)
    o, d, _ = GetRays(h, w, _k9(K), _m12(pose).reshape(3, 4), device=grid.Verts.device)
    res = G.RayCastMesh((o.reshape(-1, 3), d.reshape(-1, 3)), grid, near=near, far=far, cull=cull, points=False, stats=stats)
    hit = res.Face >= 0
    depth = torch.where(hit, res.T, torch.zeros_like(res.T)).reshape(h, w)
    u, v = res.UV[:, 0], res.UV[:, 1]
    bary = torch.where(hit[:, None], torch.stack([(1.0 - u) - v, u, v], dim=-1), torch.zeros((1, 3), device=u.device)).reshape(h, w, 3)
    return MeshRender(depth, hit.to(torch.float32).reshape(h, w), res.Face.reshape(h, w), bary, Stats=stats)


def RenderMeshView(mesh, view, rparams=None, **kw):
    """RenderMesh at a dataset.View (H, W, K, Pose are read); with rparams its RenderFactor is honoured through RenderViewDims, so the maps line up with
    RenderView(renderer, view.Pose, view.W, view.H, view.K, rparams)."""
    from .renderer import RenderViewDims
    h1, w1, k1 = RenderViewDims(view.H, view.W, view.K, 0 if rparams is None else rparams.RenderFactor)
    return RenderMesh(mesh, view.Pose, w1, h1, k1, **kw)


def VisibleFaces(mesh, views, **kw):
    """[F] bool: the faces that own at least one pixel of some view (RenderMeshView(mesh, view, **kw).FaceMap).  No host synchronisation."""
    kw.setdefault("attrs", ())
    nf = int(mesh.Faces.shape[0])
    seen = torch.zeros((nf + 1,), device=mesh.Vertices.device, dtype=torch.bool)          # slot 0 takes the -1 of the pixels that see nothing
    for v in views:
        seen[RenderMeshView(mesh, v, **kw).FaceMap.reshape(-1).to(torch.int64) + 1] = True
    return seen[1:]


def FilterVisible(mesh, views, **kw):
    """The sub-mesh of VisibleFaces(mesh, views, **kw): what some camera actually sees, without the interior shells of a density isosurface.  Vertices stay in
    ascending original order; normals, colours and relevancy follow them."""
    return M._submesh(mesh, VisibleFaces(mesh, views, **kw), mesh.Relevancy)


def EvaluateMesh(mesh, renderer, views, rparams, background=None, acc_min=0.5, texture=None, **kw):
    """Score a mesh against the field it came from: every dataset.View is rendered twice, the field by RenderView and the mesh by RenderMeshView (same dims and K, so
    RenderFactor is honoured).  Returns float64 device tensors as EvaluateViews does, {name: [n_views], "mean_" + name: its mean} for
      psnr, ssim   metrics.PSNR / SSIM of the mesh's RGBMap over `background` (3 values; None: white if rparams.WhiteBkgr, else black) against the render's RGBMap;
      depth_error  the mean |depth_mesh - DepthMap / AccMap| over the pixels both hit (the render where AccMap >= acc_min); NaN where none is;
      iou          intersection over union of the two hit masks.
    The mesh needs Colors -- or, with texture (a texture.TextureAtlas of three channels baked for this mesh), its RGBMap comes from the atlas through
    texture.RenderMeshViewTextured and Colors is not read.  NDC and LeRF renderers are refused as FuseViews refuses them."""
    from . import metrics
    from .renderer import LeRFRenderer, RenderView
    if isinstance(renderer, LeRFRenderer):
        raise L.NrfError("EvaluateMesh: a LeRF renderer renders no colour; score against its NeRFRenderer")
    if rparams.Ndc:
        raise L.NrfError("EvaluateMesh: the depth of an NDC render is not metric (rparams.Ndc must be False)")
    if texture is None and mesh.Colors is None:
        raise L.NrfError("EvaluateMesh: the mesh has no Colors to compare with the render")
    if texture is not None and int(texture.Image.shape[-1]) != 3:
        raise L.NrfError(f"EvaluateMesh: the texture must hold 3 channels to compare with the render, got {int(texture.Image.shape[-1])}")
    bg = (1.0, 1.0, 1.0) if background is None and rparams.WhiteBkgr else (0.0, 0.0, 0.0) if background is None else tuple(float(b) for b in background)
    kw["attrs"] = ("Colors",)
    names = ("psnr", "ssim", "depth_error", "iou")
    scores = {n: [] for n in names}
    dev = torch.device("cuda", torch.cuda.current_device())
    for v in views:
        o = RenderView(renderer, v.Pose, v.W, v.H, v.K, rparams).Outputs
        if texture is None:
            m = RenderMeshView(mesh, v, rparams, **kw)
        else:
            from .texture import RenderMeshViewTextured
            m = RenderMeshViewTextured(mesh, texture, v, rparams, **kw)
        h, w = m.DepthMap.shape
        acc_m = m.AccMap
        rgb_m = m.RGBMap + (1.0 - acc_m)[..., None] * torch.tensor(bg, device=acc_m.device, dtype=torch.float32)
        rgb_r = o.RGBMap.reshape(h, w, 3)
        acc_r, depth_r = o.AccMap.reshape(h, w), o.DepthMap.reshape(h, w)
        hit_m, hit_r = acc_m > 0, acc_r >= acc_min
        both = (hit_m & hit_r).to(torch.float64)
        err = (m.DepthMap - depth_r / acc_r).abs().to(torch.float64)
        scores["psnr"].append(metrics.PSNR(rgb_m, rgb_r))
        scores["ssim"].append(metrics.SSIM(rgb_m, rgb_r))
        scores["depth_error"].append(torch.where(both > 0, err, torch.zeros_like(err)).sum() / both.sum())
        scores["iou"].append(both.sum() / (hit_m | hit_r).to(torch.float64).sum())
    out = {}
    for n in names:
        out[n] = torch.stack(scores[n]) if scores[n] else torch.empty((0,), device=dev, dtype=torch.float64)
        out["mean_" + n] = out[n].mean()
    return out
