"""Depth fusion: TSDFVolume, FuseViews, ExtractMeshTSDF and OrbitViews over the C ABI (include/nerfpp_hip.h, tsdf.hip).

The reference has no mesh export; the names follow the mirror's style.  The rendered depth of a ring of views (Outputs.DepthMap / AccMap / RGBMap of RenderView) is
fused into a truncated signed distance volume on the lattice of DensityGrid, and the zero level of that volume is meshed by the existing Isosurface: the surface sits at
level 0 with no density threshold to guess, floaters count for what a camera actually sees of them, and the colours are what the views saw.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import mesh as M
from .dataset import View, _k9, _m12
from .modules import _ptr, _stream, _dev_f32

MIN_TRUNC_STEPS = 4.0          # Extract's observed-neighbourhood filter reaches 1.5 steps per axis; at 3 steps the CPU model shows holes in a perfect sphere
DEFAULT_TRUNC_STEPS = 5.0


class TsdfView(C.Structure):          # nrf_tsdf_view
    _fields_ = [("d_depth", C.c_void_p), ("d_acc", C.c_void_p), ("d_rgb", C.c_void_p), ("h", C.c_int), ("w", C.c_int), ("K", C.c_float * 9), ("c2w", C.c_float * 12)]


class TSDFVolume:
    """tsdf [nz, ny, nx] (1 = free or unseen), weight [nz, ny, nx] and -- colors=True -- color [4, nz, ny, nx] (r, g, b, colour weight) on the lattice of DensityGrid
    over bbox.  trunc: the truncation distance in world units; None = 5 x the largest axis step, below 4 x it is refused.  acc_min: the accumulated opacity from which a
    pixel counts as a surface hit (its depth is DepthMap / AccMap); carve: pixels below it are background observations that pull the voxels on their ray to +1."""

    def __init__(self, bbox, resolution=256, trunc=None, colors=True, max_weight=64.0, acc_min=0.5, carve=True, device=None):
        self.nx, self.ny, self.nz = M._resolution(resolution)
        if min(self.nx, self.ny, self.nz) < 2:
            raise L.NrfError(f"TSDFVolume: resolution {resolution!r} needs at least 2 lattice points per axis")
        b = torch.as_tensor(bbox).detach().cpu().numpy() if torch.is_tensor(bbox) else np.asarray(bbox)
        if b.size != 6:
            raise L.NrfError(f"TSDFVolume: bbox must hold 6 values (min xyz, max xyz), got shape {tuple(b.shape)}")
        self.bbox = np.ascontiguousarray(b, np.float32).reshape(6)
        if not (np.isfinite(self.bbox).all() and (self.bbox[3:] > self.bbox[:3]).all()):
            raise L.NrfError(f"TSDFVolume: empty, inverted or non-finite box {self.bbox.tolist()}")
        self.step = (self.bbox[3:] - self.bbox[:3]) / (np.array([self.nx, self.ny, self.nz]) - 1).astype(np.float32)          # fp32, as the kernels form it
        largest = np.float32(self.step.max())
        self.trunc = float(np.float32(DEFAULT_TRUNC_STEPS) * largest if trunc is None else np.float32(trunc))
        if not (np.isfinite(self.trunc) and np.float32(self.trunc) >= np.float32(MIN_TRUNC_STEPS) * largest):
            raise L.NrfError(f"TSDFVolume: trunc {self.trunc:g} is below {MIN_TRUNC_STEPS:g} x the largest lattice step {float(largest):g}: Extract's observed-"
                             "neighbourhood filter would open holes in the surface")
        self.max_weight, self.acc_min, self.carve = float(max_weight), float(acc_min), bool(carve)
        if not (self.max_weight >= 1.0 and np.isfinite(self.acc_min) and self.acc_min > 0.0):
            raise L.NrfError(f"TSDFVolume: max_weight {max_weight!r} must be >= 1 and acc_min {acc_min!r} finite and > 0")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        shape = (self.nz, self.ny, self.nx)
        self.tsdf = torch.ones(shape, device=dev, dtype=torch.float32)
        self.weight = torch.zeros(shape, device=dev, dtype=torch.float32)
        self.color = torch.zeros((4,) + shape, device=dev, dtype=torch.float32) if colors else None

    def Reset(self):
        self.tsdf.fill_(1.0)
        self.weight.zero_()
        if self.color is not None:
            self.color.zero_()

    def _view(self, depth, K, pose, acc, rgb, keep):
        d = _dev_f32(depth)
        if d.dim() != 2 or d.numel() == 0:
            raise L.NrfError(f"TSDFVolume.Integrate: depth must be [h, w], got {tuple(d.shape)}")
        h, w = (int(v) for v in d.shape)
        a = None if acc is None else _dev_f32(acc).reshape(-1)
        c = None if rgb is None else _dev_f32(rgb).reshape(-1)
        if (a is not None and a.numel() != h * w) or (c is not None and c.numel() != h * w * 3):
            raise L.NrfError(f"TSDFVolume.Integrate: acc must be [{h}, {w}] and rgb [{h}, {w}, 3]")
        keep += [d, a, c]          # the tensors live until the call has been enqueued on their stream
        v = TsdfView()
        v.d_depth, v.d_acc, v.d_rgb = d.data_ptr(), (a.data_ptr() if a is not None else None), (c.data_ptr() if c is not None else None)
        v.h, v.w = h, w
        v.K = (C.c_float * 9)(*_k9(K).tolist())
        v.c2w = (C.c_float * 12)(*_m12(pose).tolist())
        return v

    def IntegrateViews(self, views):
        """One nrf_tsdf_integrate over `views`: dicts or tuples of (depth [h, w], K [3, 3], pose [3|4, 4], acc [h, w] or None, rgb [h, w, 3] or None), fused in list
        order, 16 per launch.  No host synchronisation."""
        keep, recs = [], []
        for v in views:
            if isinstance(v, dict):
                v = (v["depth"], v["K"], v["pose"], v.get("acc"), v.get("rgb"))
            depth, K, pose, acc, rgb = (tuple(v) + (None, None))[:5]
            recs.append(self._view(depth, K, pose, acc, rgb, keep))
        arr = (TsdfView * max(len(recs), 1))(*recs)
        L.check(L.lib().nrf_tsdf_integrate(_ptr(self.tsdf), _ptr(self.weight), _ptr(self.color), self.nx, self.ny, self.nz, self.bbox.ctypes.data_as(C.c_void_p),
                                           C.cast(arr, C.c_void_p), len(recs), self.trunc, self.acc_min, self.max_weight, int(self.carve), _stream()))

    def Integrate(self, depth, K, pose, acc=None, rgb=None):
        self.IntegrateViews([(depth, K, pose, acc, rgb)])

    def Field(self):
        """-tsdf: inside positive, the convention of Isosurface."""
        return -self.tsdf

    def Observed(self, pts):
        """nrf_tsdf_observed: [p] bool, the points whose 27 nearest lattice points were all observed."""
        x = _dev_f32(pts).reshape(-1, 3)
        ok = torch.empty((x.shape[0],), device=x.device, dtype=torch.uint8)
        L.check(L.lib().nrf_tsdf_observed(_ptr(self.weight), self.nx, self.ny, self.nz, self.bbox.ctypes.data_as(C.c_void_p), _ptr(x), x.shape[0], _ptr(ok), _stream()))
        return ok.to(torch.bool)

    def SampleColor(self, pts):
        """nrf_tsdf_sample_color: [p, 3], the colour volume at pts (trilinear over the corners that hold a colour; 0 where none does)."""
        if self.color is None:
            raise L.NrfError("TSDFVolume.SampleColor: the volume was made with colors=False")
        x = _dev_f32(pts).reshape(-1, 3)
        rgb = torch.empty((x.shape[0], 3), device=x.device, dtype=torch.float32)
        L.check(L.lib().nrf_tsdf_sample_color(_ptr(self.color), self.nx, self.ny, self.nz, self.bbox.ctypes.data_as(C.c_void_p), _ptr(x), x.shape[0], _ptr(rgb), _stream()))
        return rgb

    def Extract(self, keep_largest=None, min_component_faces=0):
        """Isosurface(Field(), bbox, 0) -> the faces whose three vertices are observed (the zero level between the observed band behind a surface and the never-observed
        interior is no surface) -> FilterComponents if asked -> colours from the colour volume.  Normals are the isosurface's lattice normals."""
        verts, faces, normals = M.Isosurface(self.Field(), self.bbox, 0.0)
        ok = self.Observed(verts)
        out = M._submesh(M.Mesh(verts, faces, normals), ok[faces.to(torch.int64)].all(dim=-1))
        if keep_largest is not None or min_component_faces > 0:
            out = M.FilterComponents(out, keep_largest, min_component_faces)
        if self.color is not None:
            out.Colors = self.SampleColor(out.Vertices)
        return out


def FuseViews(renderer, views, rparams, volume=None, bbox=None, resolution=256, **volume_args):
    """Render every view (dataset.View: H, W, K, Pose are read) with RenderView and fuse its DepthMap, AccMap and RGBMap into `volume` (default: a new
    TSDFVolume(bbox, resolution, **volume_args), bbox as DensityGrid's) with the dims and K of RenderViewDims, so RenderFactor is honoured.  One nrf_tsdf_integrate
    for all views; no host synchronisation of its own."""
    from .renderer import LeRFRenderer, RenderView, RenderViewDims
    if isinstance(renderer, LeRFRenderer):
        raise L.NrfError("FuseViews: a LeRF renderer renders no colour; fuse the views of its NeRFRenderer")
    if rparams.Ndc:
        raise L.NrfError("FuseViews: the depth of an NDC render is not metric (rparams.Ndc must be False)")
    if volume is None:
        volume = TSDFVolume(M._bbox(renderer, bbox), resolution, **volume_args)
    recs = []
    for v in views:
        h1, w1, k1 = RenderViewDims(v.H, v.W, v.K, rparams.RenderFactor)
        o = RenderView(renderer, v.Pose, v.W, v.H, v.K, rparams).Outputs
        recs.append((o.DepthMap.reshape(h1, w1), k1, v.Pose, o.AccMap.reshape(h1, w1), o.RGBMap.reshape(h1, w1, 3)))
    volume.IntegrateViews(recs)
    return volume


def ExtractMeshTSDF(renderer, views, rparams, resolution=256, bbox=None, keep_largest=None, min_component_faces=0, **volume_args):
    """FuseViews into a new volume, then TSDFVolume.Extract -> Mesh."""
    return FuseViews(renderer, views, rparams, None, bbox, resolution, **volume_args).Extract(keep_largest, min_component_faces)


def OrbitViews(n, h, w, K, radius, elevations=(-30.0, 30.0)):
    """n Views of h x w on scene.pose_spherical(360 i / n, elevations[i % len(elevations)], radius): a ring around the origin, alternating the elevations."""
    from .scene import pose_spherical
    k = np.ascontiguousarray(np.asarray(K.detach().cpu().numpy() if torch.is_tensor(K) else K, np.float32).reshape(3, 3))
    return [View(int(h), int(w), k, pose_spherical(360.0 * i / n, float(elevations[i % len(elevations)]), float(radius))) for i in range(int(n))]
