"""Texture atlases for meshes: AtlasLayout, AtlasTexels, BakeTexture, SampleTexture, RenderMeshTextured, RenderMeshViewTextured and SaveOBJ over the C ABI
(include/nerfpp_hip.h, texture.hip).

The reference has no textures; the names follow the mirror's style.  A simplified mesh keeps one colour per surviving vertex, so its colour resolution falls with its
face count; an atlas puts it back: every face owns half a T x T tile of one image, baked from the field at the texel's own surface point.  The layout is integer
arithmetic on (face count, tile) alone and every kernel a stated fp32 operation order, so tests/texture_ref.py equals every output bit for bit.
"""
import ctypes as C
import math
import os
import struct
import zlib
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from . import raster as R
from .dataset import _k9, _m12
from .modules import _ptr, _stream, _dev_f32

MIN_TILE, MAX_TILE, MAX_SIZE, MAX_CHANNELS = 4, 64, 16384, 8          # NRF_ATLAS_* / NRF_TEXTURE_MAX_CHANNELS of the header (tests/test_texture_host.py holds them to it)
NEAREST, BILINEAR = 0, 1                                              # NRF_TEXTURE_*
_FILTER = {"nearest": NEAREST, "bilinear": BILINEAR}
SLAB_TEXELS = 1 << 21          # BakeTexture's default slab: 92 MB of packed rays
POINT_CHUNK = 1 << 18          # mode="point": points per RunNetwork call


def AtlasLayout(n_faces, tile):
    """(width, height, cols, rows) of the atlas of n_faces faces at `tile` texels: nrf_atlas_dims on the host, with its refusals."""
    f, t = int(n_faces), int(tile)
    if not MIN_TILE <= t <= MAX_TILE:
        raise L.NrfError(f"AtlasLayout: tile {t} ({MIN_TILE} .. {MAX_TILE} texels)")
    if not 0 <= f <= 2 ** 31 - 2:
        raise L.NrfError(f"AtlasLayout: {f} faces (0 .. 2^31 - 2)")
    cells = (f + 1) // 2
    cols = math.isqrt(cells)
    cols += cols * cols < cells
    rows = -(-cells // cols) if cols else 0
    if cols * t > MAX_SIZE or rows * t > MAX_SIZE:
        raise L.NrfError(f"AtlasLayout: {f} faces at tile {t} need an atlas of {cols * t} x {rows * t} texels; a side is at most {MAX_SIZE}, so "
                         f"{2 * (MAX_SIZE // t) ** 2} faces fit")
    return cols * t, rows * t, cols, rows


@dataclass
class TextureAtlas:
    Image: torch.Tensor                       # [H, W, C] f32: the atlas of AtlasLayout(NFaces, Tile)
    Tile: int
    NFaces: int                               # the face count the layout was made for: an atlas belongs to one face order
    Acc: Optional[torch.Tensor] = None        # [H, W] f32: the AccMap of a mode="render" bake

    def __post_init__(self):
        w, h, _, _ = AtlasLayout(self.NFaces, self.Tile)
        if self.Image.dim() != 3 or tuple(self.Image.shape[:2]) != (h, w) or not 1 <= self.Image.shape[2] <= MAX_CHANNELS:
            raise L.NrfError(f"TextureAtlas: {self.NFaces} faces at tile {self.Tile} need an image [{h}, {w}, 1 .. {MAX_CHANNELS}], got {tuple(self.Image.shape)}")

    def check(self, mesh, who):
        if int(mesh.Faces.shape[0]) != self.NFaces:
            raise L.NrfError(f"{who}: the atlas was baked for {self.NFaces} faces, the mesh has {int(mesh.Faces.shape[0])} (an atlas belongs to one face order)")


def _mesh_arrays(mesh):
    verts = _dev_f32(mesh.Vertices).reshape(-1, 3)
    faces = mesh.Faces.to(device=verts.device, dtype=torch.int32).reshape(-1, 3).contiguous()
    return verts, faces


def AtlasTexels(mesh, tile, offset=0.0, rows=None):
    """nrf_atlas_texels over the atlas rows `rows` = (row0, count) (None: all) -> (face [r, W] int32, bary [r, W, 3], pos [r, W, 3], rays [r, W, 11]): per texel its
    owner face (-1: none), barycentrics, surface point and the packed short ray from `offset` above the surface down the normal.  mesh.Normals are used where the
    mesh has them, the face normal otherwise.  No host synchronisation."""
    verts, faces = _mesh_arrays(mesh)
    nf, t = int(faces.shape[0]), int(tile)
    w, h, _, _ = AtlasLayout(nf, t)
    row0, n = (0, h) if rows is None else (int(rows[0]), int(rows[1]))
    normals = None if getattr(mesh, "Normals", None) is None else _dev_f32(mesh.Normals).reshape(-1, 3)
    dev = verts.device
    face = torch.empty((max(n, 0), w), device=dev, dtype=torch.int32)
    bary, pos = torch.empty((max(n, 0), w, 3), device=dev), torch.empty((max(n, 0), w, 3), device=dev)
    rays = torch.empty((max(n, 0), w, 11), device=dev)
    L.check(L.lib().nrf_atlas_texels(_ptr(verts), int(verts.shape[0]), _ptr(faces), nf, _ptr(normals), t, float(offset), row0, n, _ptr(face), _ptr(bary), _ptr(pos),
                                     _ptr(rays), _stream()))
    return face, bary, pos, rays


def _colour_source(source, mode, rparams, offset, attribute="Colors", max_dist=None):
    """-> (colour(pos [n, 3], rays [n, 11]) -> (rgb [n, C], acc [n] or None), the offset of the rays)"""
    from . import geometry as G
    from .mesh import Mesh
    from .renderer import LeRFRenderer, NeRFRenderer
    from .tsdf import TSDFVolume
    if isinstance(source, (Mesh, G.FaceGrid, G.MeshBVH)):
        grid = source if isinstance(source, (G.FaceGrid, G.MeshBVH)) else G.FaceGrid(source)          # binned once per bake
        if attribute not in ("Colors", "Relevancy") or getattr(grid.Mesh, attribute) is None:
            raise L.NrfError(f"BakeTexture: the source mesh has no {attribute!r} to bake (attribute is 'Colors' or 'Relevancy')")

        def closest(pos, rays):
            res = G.ClosestOnMesh(pos, grid, max_dist=max_dist, points=False)
            return G.InterpolateAttributes(grid.Mesh, res, attribute).reshape(pos.shape[0], -1), None
        return closest, 0.0
    if isinstance(source, LeRFRenderer):
        raise L.NrfError("BakeTexture: a LeRF renderer renders no colour; bake from its NeRFRenderer")
    if isinstance(source, TSDFVolume):
        return (lambda pos, rays: (source.SampleColor(pos), None)), 0.0
    if isinstance(source, NeRFRenderer):
        if mode == "point":
            def point(pos, rays):
                out = torch.empty_like(pos)
                for i in range(0, pos.shape[0], POINT_CHUNK):
                    raw = source.RunNetwork(pos[i:i + POINT_CHUNK, None, :], rays[i:i + POINT_CHUNK, 3:6].contiguous())
                    out[i:i + POINT_CHUNK] = torch.sigmoid(raw[:, 0, :3])          # RawToOutputs's rgb, as ExtractMesh colours a vertex
                return out, None
            return point, 0.0
        if mode != "render":
            raise L.NrfError(f"BakeTexture: mode must be 'point' or 'render', got {mode!r}")
        if rparams is None or offset is None:
            raise L.NrfError("BakeTexture(mode='render'): pass rparams and the offset of the short rays in world units")
        if rparams.Ndc:
            raise L.NrfError("BakeTexture: the rays of a bake are metric (rparams.Ndc must be False)")

        def render(pos, rays):
            o = source.BatchifyRays(rays, None, rparams.NSamples, chunk=int(rparams.Chunk), n_importance=rparams.NImportance, white_bkgr=rparams.WhiteBkgr,
                                    precision=rparams.Precision, return_weights=False).Outputs
            return o.RGBMap, o.AccMap
        return render, float(offset)
    if callable(source):
        return (lambda pos, rays: (source(pos, rays[:, 3:6].contiguous()), None)), 0.0
    raise L.NrfError(f"BakeTexture: no way to take colour from {type(source).__name__} (a NeRFRenderer, a TSDFVolume, a Mesh or a callable (pos, dir) -> [n, C])")


def BakeTexture(mesh, source, tile=8, mode="point", rparams=None, offset=None, chunk_rows=None, attribute="Colors", max_dist=None):
    """Bake the atlas of `mesh` at `tile` texels from `source`, slab by slab of chunk_rows atlas rows (default: about SLAB_TEXELS texels); texels without an owner
    get 0.  No host synchronisation of its own.  source:
      a NeRFRenderer, mode="point"   sigmoid(RunNetwork(P, -N)[..., :3]) at the texel's surface point P seen along -N: what ExtractMesh does per vertex;
      a NeRFRenderer, mode="render"  BatchifyRays over AtlasTexels' short rays (rparams.NSamples / NImportance / WhiteBkgr / Precision / Chunk, no cone): the colour
                                     a camera `offset` (world units, required) above the surface on its normal sees; the AccMap is kept as Acc.  NDC is refused;
      a TSDFVolume                   its colour volume at P (nrf_tsdf_sample_color);
      a callable                     source(pos [n, 3], dir [n, 3]) -> [n, C], C <= 8, dir = -N;
      a Mesh (or its FaceGrid)       its `attribute` ("Colors" or "Relevancy") interpolated at the closest point of ITS surface to P (geometry.ClosestOnMesh): the
                                     detail of a dense mesh carried onto a simplified one.  The source is binned once per bake (two host synchronisations; none
                                     with a FaceGrid); texels with no face within max_dist get 0.
    LeRF renderers are refused as FuseViews refuses them."""
    colour, off = _colour_source(source, mode, rparams, offset, attribute, max_dist)
    nf, t = int(mesh.Faces.shape[0]), int(tile)
    w, h, _, _ = AtlasLayout(nf, t)
    step = max(1, SLAB_TEXELS // max(w, 1)) if chunk_rows is None else int(chunk_rows)
    if step < 1:
        raise L.NrfError(f"BakeTexture: chunk_rows must be >= 1, got {chunk_rows}")
    dev = mesh.Vertices.device
    image, acc = None, None
    for r0 in range(0, h, step):
        n = min(step, h - r0)
        face, _, pos, rays = AtlasTexels(mesh, t, off, (r0, n))
        rgb, a = colour(pos.reshape(-1, 3), rays.reshape(-1, 11))
        rgb = rgb.reshape(n, w, -1).to(torch.float32)
        owned = face >= 0
        if image is None:
            image = torch.zeros((h, w, int(rgb.shape[-1])), device=dev, dtype=torch.float32)
            acc = None if a is None else torch.zeros((h, w), device=dev, dtype=torch.float32)
        image[r0:r0 + n] = torch.where(owned[..., None], rgb, torch.zeros_like(rgb))
        if a is not None:
            acc[r0:r0 + n] = torch.where(owned, a.reshape(n, w), torch.zeros_like(a.reshape(n, w)))
    if image is None:          # no faces: an empty atlas
        image = torch.zeros((0, 0, 3), device=dev, dtype=torch.float32)
    return TextureAtlas(image, t, nf, acc)


def BakeAmbientOcclusion(mesh, tile=8, k=64, max_dist=None, offset=None, seed=0, grid=None, chunk_rows=None, stats=None):
    """The ambient-occlusion atlas of `mesh` at `tile` texels -> a one-channel TextureAtlas: geometry.AmbientOcclusion at every owned texel's surface point with its
    FACE normal (AtlasTexels of the mesh without vertex normals), slab by slab of chunk_rows atlas rows as BakeTexture works; texels without an owner get 0.  The
    occluder is grid (a geometry.FaceGrid; default FaceGrid(mesh): two host synchronisations).  k, max_dist, offset, seed as AmbientOcclusion's; the direction j of
    the texel (Y, X) is drawn for the index Y * width + X, so the atlas does not depend on chunk_rows.  SaveOBJ(..., occlusion=atlas) multiplies it into the colours."""
    import dataclasses
    from . import geometry as G
    grid = G.FaceGrid(mesh, stats=stats) if grid is None else grid
    flat = dataclasses.replace(mesh, Normals=None)
    nf, t = int(mesh.Faces.shape[0]), int(tile)
    w, h, _, _ = AtlasLayout(nf, t)
    step = max(1, SLAB_TEXELS // max(w, 1)) if chunk_rows is None else int(chunk_rows)
    if step < 1:
        raise L.NrfError(f"BakeAmbientOcclusion: chunk_rows must be >= 1, got {chunk_rows}")
    image = torch.zeros((h, w, 1), device=mesh.Vertices.device, dtype=torch.float32)
    for r0 in range(0, h, step):
        n = min(step, h - r0)
        face, _, pos, rays = AtlasTexels(flat, t, 0.0, (r0, n))
        normals = -rays.reshape(-1, 11)[:, 3:6]          # the ray of a texel looks down its normal
        ao = G.AmbientOcclusion(mesh, k=k, max_dist=max_dist, offset=offset, seed=seed, grid=grid, at=(pos.reshape(-1, 3), normals), index0=r0 * w, stats=stats)
        image[r0:r0 + n, :, 0] = torch.where(face >= 0, ao.reshape(n, w), torch.zeros_like(ao.reshape(n, w)))
    return TextureAtlas(image, t, nf)


def _filter(filter, who):
    if filter not in _FILTER:
        raise L.NrfError(f"{who}: filter must be one of {sorted(_FILTER)}, got {filter!r}")
    return _FILTER[filter]


def SampleTexture(atlas, face, bary, filter="bilinear"):
    """nrf_texture_sample: [..., C], the atlas at (face [...] int32, bary [..., 3]) pairs -- SampleSurface's faces with (1 - u - v, u, v), or a FaceMap with
    perspective-corrected barycentrics.  A face < 0 or >= NFaces gives 0."""
    flt = _filter(filter, "SampleTexture")
    img = _dev_f32(atlas.Image)
    f = face.to(device=img.device, dtype=torch.int32).contiguous()
    b = _dev_f32(bary).to(img.device)
    if tuple(b.shape) != tuple(f.shape) + (3,):
        raise L.NrfError(f"SampleTexture: bary must be {tuple(f.shape) + (3,)}, got {tuple(b.shape)}")
    c = int(img.shape[2]) if img.dim() == 3 else 3
    out = torch.empty(tuple(f.shape) + (c,), device=img.device, dtype=torch.float32)
    L.check(L.lib().nrf_texture_sample(_ptr(img) if img.numel() else None, atlas.NFaces, atlas.Tile, c, _ptr(f), _ptr(b), f.numel(), flt, _ptr(out), _stream()))
    return out


def RenderMeshTextured(mesh, atlas, pose, W, H, K, filter="bilinear", **kw):
    """RenderMesh(mesh, pose, W, H, K, attrs=(), **kw), then nrf_texture_shade: the same MeshRender with RGBMap [H, W, C] looked up in the atlas at every pixel's
    surface point (perspective-corrected barycentrics), 0 where no face is seen.  mesh.Colors is not read.  No host synchronisation."""
    flt = _filter(filter, "RenderMeshTextured")
    atlas.check(mesh, "RenderMeshTextured")
    kw["attrs"] = ()
    res = R.RenderMesh(mesh, pose, W, H, K, **kw)
    verts, faces = _mesh_arrays(mesh)
    img = _dev_f32(atlas.Image)
    h, w = res.FaceMap.shape
    c = int(img.shape[2])
    out = torch.empty((h, w, c), device=verts.device, dtype=torch.float32)
    k, m = _k9(K), _m12(pose)
    L.check(L.lib().nrf_texture_shade(_ptr(verts), int(verts.shape[0]), _ptr(faces), int(faces.shape[0]), _ptr(res.FaceMap), _ptr(res.BaryMap), h, w,
                                      k.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p), _ptr(img) if img.numel() else None, atlas.Tile, c, flt, _ptr(out),
                                      _stream()))
    res.RGBMap = out
    return res


def RenderMeshViewTextured(mesh, atlas, view, rparams=None, **kw):
    """RenderMeshTextured at a dataset.View, with the dims and K of RenderViewDims as RenderMeshView."""
    from .renderer import RenderViewDims
    h1, w1, k1 = RenderViewDims(view.H, view.W, view.K, 0 if rparams is None else rparams.RenderFactor)
    return RenderMeshTextured(mesh, atlas, view.Pose, w1, h1, k1, **kw)


def _png_chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def EncodePNG(rgb_u8):
    """The bytes of an 8-bit RGB PNG of rgb_u8 [H, W, 3] uint8 (H, W >= 1): filter 0 on every row, one IDAT; zlib and struct of the standard library only."""
    a = np.ascontiguousarray(rgb_u8, np.uint8)
    if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise L.NrfError(f"EncodePNG: needs [H, W, 3] uint8 with H, W >= 1, got {a.shape}")
    h, w, _ = a.shape
    rows = np.concatenate([np.zeros((h, 1), np.uint8), a.reshape(h, w * 3)], axis=1)
    return (b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + _png_chunk(b"IDAT", zlib.compress(rows.tobytes(), 6))
            + _png_chunk(b"IEND", b""))


def QuantizeTexture(image):
    """[H, W, 3] uint8 of the first three channels of an atlas image (a single channel is repeated): clamp(round(255 c)), as SavePLY quantises a colour."""
    c = image.detach().cpu().numpy().astype(np.float64)
    c = np.repeat(c[..., :1], 3, axis=-1) if c.shape[-1] < 3 else c[..., :3]
    return np.clip(np.rint(np.nan_to_num(c) * 255.0), 0, 255).astype(np.uint8)


def SaveOBJ(path, mesh, atlas, occlusion=None):
    """Write `path` (v, vn where the mesh has normals, three vt per face, f a/ta/na ...), path + ".mtl" (map_Kd) and path + ".png" (the atlas as 8-bit RGB).  The vt
    of a corner is ((X + 0.5) / width, 1 - (Y + 0.5) / height) of the centre of the texel (X, Y) the layout gives that corner.  occlusion: a one-channel atlas of
    the same mesh and tile (BakeAmbientOcclusion) that is multiplied into the image before it is quantised; without it the files are what they always were."""
    atlas.check(mesh, "SaveOBJ")
    if occlusion is not None:
        occlusion.check(mesh, "SaveOBJ")
        if occlusion.Tile != atlas.Tile or int(occlusion.Image.shape[-1]) != 1:
            raise L.NrfError(f"SaveOBJ: the occlusion atlas must hold one channel at tile {atlas.Tile}, got {int(occlusion.Image.shape[-1])} at tile {occlusion.Tile}")
    nf, t = atlas.NFaces, atlas.Tile
    w, h, cols, _ = AtlasLayout(nf, t)
    if nf == 0:
        raise L.NrfError("SaveOBJ: the mesh has no faces, so its atlas has no texels to write")
    v = mesh.Vertices.detach().cpu().numpy().astype(np.float64).reshape(-1, 3)
    fc = mesh.Faces.detach().cpu().numpy().astype(np.int64).reshape(-1, 3)
    nm = None if getattr(mesh, "Normals", None) is None else mesh.Normals.detach().cpu().numpy().astype(np.float64).reshape(-1, 3)
    f = np.arange(nf)
    cell, odd = f >> 1, (f & 1).astype(bool)
    x0, y0 = (cell % cols) * t, (cell // cols) * t
    n = t - 3
    ci, cj = np.array([0, n, 0]), np.array([0, 0, n])          # the corners' indices in the face's own frame
    X = np.where(odd[:, None], x0[:, None] + t - 1 - ci, x0[:, None] + ci)
    Y = np.where(odd[:, None], y0[:, None] + t - 1 - cj, y0[:, None] + cj)
    uv = np.stack([(X + 0.5) / w, 1.0 - (Y + 0.5) / h], -1).reshape(-1, 2)
    name = os.path.basename(path)
    lines = [f"mtllib {name}.mtl", "usemtl atlas"]
    lines += ["v %.9g %.9g %.9g" % tuple(p) for p in v]
    if nm is not None:
        lines += ["vn %.9g %.9g %.9g" % tuple(p) for p in nm]
    lines += ["vt %.17g %.17g" % tuple(p) for p in uv]
    for k, (a, b, c) in enumerate(fc + 1):
        ta = 3 * k + 1
        lines.append(f"f {a}/{ta}/{a} {b}/{ta + 1}/{b} {c}/{ta + 2}/{c}" if nm is not None else f"f {a}/{ta} {b}/{ta + 1} {c}/{ta + 2}")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    with open(path + ".mtl", "w") as fh:
        fh.write(f"newmtl atlas\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 0\nmap_Kd {name}.png\n")
    with open(path + ".png", "wb") as fh:
        fh.write(EncodePNG(QuantizeTexture(atlas.Image if occlusion is None else atlas.Image * occlusion.Image.to(atlas.Image.device))))
