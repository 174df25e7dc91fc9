"""Mesh export: DensityGrid, Isosurface, ExtractMesh and SavePLY over the C ABI (include/nerfpp_hip.h, mesh.hip).

The reference has no mesh export; the names follow the mirror's style.  The density lattice is the exact-fp32 sigma of the renderer's network
(== RunNetwork(..., NRF_PREC_F32)[..., 3] bit for bit); the isosurface is marching tetrahedra on the Kuhn split of each cell, in an order fixed by integer
prefix scans (two extractions give the same arrays).
"""
import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from .modules import _HashBase, _ptr, _stream, _dev_f32

COLOR_CHUNK = 1 << 18        # vertices per RunNetwork call of ExtractMesh


@dataclass
class Mesh:
    Vertices: torch.Tensor                    # [V, 3] f32
    Faces: torch.Tensor                       # [F, 3] int32, counter-clockwise seen from outside
    Normals: torch.Tensor                     # [V, 3] f32, outward unit normals (0 where the lattice gradient vanishes)
    Colors: Optional[torch.Tensor] = None     # [V, 3] f32 in [0, 1]
    Relevancy: Optional[torch.Tensor] = None  # [V, 2] (or [V]) f32: LeRF relevancy of the vertices (query.VertexRelevancy); SavePLY writes column 0


def _resolution(resolution):
    r = (int(resolution),) * 3 if np.isscalar(resolution) else tuple(int(v) for v in resolution)
    if len(r) != 3:
        raise L.NrfError(f"resolution must be an int or (nx, ny, nz), got {resolution!r}")
    return r


def _lattice_points_at(bb, nx, ny, nz, idx):
    """P(i) of flat lattice indices idx (x fastest) as nrf_density_grid forms them: bmin + (float)i * step, step = (bmax - bmin) / (n - 1), fp32 per operation."""
    b = torch.as_tensor(np.asarray(bb, np.float32), device=idx.device)
    n = torch.tensor([nx, ny, nz], device=idx.device)
    step = (b[3:] - b[:3]) / (n - 1).to(torch.float32)
    i = idx.to(torch.int64)
    ijk = torch.stack([i % nx, (i // nx) % ny, i // (nx * ny)], dim=-1).to(torch.float32)
    return b[:3] + ijk * step


def _lattice_points(bb, nx, ny, nz, device):
    return _lattice_points_at(bb, nx, ny, nz, torch.arange(nx * ny * nz, device=device))


def _bbox(renderer, bbox):
    if bbox is None:
        if not isinstance(renderer.EmbedFn, _HashBase):
            raise L.NrfError("DensityGrid: a box is required for a renderer without a hash grid")
        bbox = renderer.EmbedFn.GetBoundingBox()
    b = torch.as_tensor(bbox).detach().cpu().numpy() if torch.is_tensor(bbox) else bbox
    return np.ascontiguousarray(np.asarray(b, np.float32).reshape(6))


def DensityGrid(renderer, bbox=None, resolution=256, slab_points=None):
    """nrf_density_grid: sigma [nz, ny, nx] (x fastest) at P = bmin + i * step, step = (bmax - bmin) / (n - 1) per axis.  bbox defaults to the hash
    embedder's GetBoundingBox(); resolution is an int or (nx, ny, nz)."""
    nx, ny, nz = _resolution(resolution)
    bb = _bbox(renderer, bbox)
    slab = 0 if slab_points is None else int(slab_points)
    lib = L.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    sigma = torch.empty((nz, ny, nx), device=dev, dtype=torch.float32)
    ws = torch.empty((int(lib.nrf_density_grid_workspace_bytes(renderer._r, nx, ny, nz, slab)),), device=dev, dtype=torch.uint8)
    L.check(lib.nrf_density_grid(renderer._r, bb.ctypes.data_as(C.c_void_p), nx, ny, nz, _ptr(sigma), slab, _ptr(ws), ws.numel(), _stream()))
    return sigma


def Isosurface(sigma, bbox, threshold):
    """nrf_isosurface_count / _emit: the surface f = threshold of a lattice sigma [nz, ny, nx] over bbox -> (Vertices [V, 3] f32, Faces [F, 3] int32,
    Normals [V, 3] f32).  Inside is f > threshold; faces wind counter-clockwise seen from outside.  Raises on a non-finite lattice value."""
    f = _dev_f32(sigma)
    if f.dim() != 3:
        raise L.NrfError(f"Isosurface: sigma must be [nz, ny, nx], got {tuple(f.shape)}")
    nz, ny, nx = (int(v) for v in f.shape)
    bb = np.ascontiguousarray(np.asarray(bbox, np.float32).reshape(6))
    lib = L.lib()
    ws = torch.empty((int(lib.nrf_isosurface_workspace_bytes(nx, ny, nz)),), device=f.device, dtype=torch.uint8)
    nv, nt, nbad = C.c_int64(), C.c_int64(), C.c_int64()
    L.check(lib.nrf_isosurface_count(_ptr(f), nx, ny, nz, bb.ctypes.data_as(C.c_void_p), threshold, C.byref(nv), C.byref(nt), C.byref(nbad),
                                     _ptr(ws), ws.numel(), _stream()))
    verts = torch.empty((nv.value, 3), device=f.device, dtype=torch.float32)
    faces = torch.empty((nt.value, 3), device=f.device, dtype=torch.int32)
    normals = torch.empty_like(verts)
    L.check(lib.nrf_isosurface_emit(_ptr(f), nx, ny, nz, bb.ctypes.data_as(C.c_void_p), threshold, _ptr(verts), _ptr(faces), _ptr(normals),
                                    nv, nt, _ptr(ws), ws.numel(), _stream()))
    return verts, faces, normals


def DensityGradient(renderer, pts):
    """nrf_density_grad: (sigma [...], grad [..., 3]) at pts [..., 3].  sigma == RunNetwork(pts, ..., NRF_PREC_F32)[..., 3] bit for bit; grad = d sigma / d x,
    the analytic gradient of the hash grid + NeRFSmall sigma net (0 where sigma is masked to 0).  Hash-grid renderers only."""
    if not hasattr(renderer, "EmbedFn") or not isinstance(renderer.EmbedFn, _HashBase) or not hasattr(renderer, "NeRF"):
        raise L.NrfError(f"unsupported: DensityGradient is built for hash-grid renderers with NeRFSmall, not {type(renderer).__name__} on "
                         f"{type(getattr(renderer, 'EmbedFn', None)).__name__}")
    x = _dev_f32(pts)
    if x.shape[-1] != 3:
        raise L.NrfError(f"DensityGradient: pts must be [..., 3], got {tuple(x.shape)}")
    lead = tuple(x.shape[:-1])
    x = x.reshape(-1, 3).contiguous()
    sigma = torch.empty(lead, device=x.device, dtype=torch.float32)
    grad = torch.empty(lead + (3,), device=x.device, dtype=torch.float32)
    L.check(L.lib().nrf_density_grad(renderer._r, _ptr(x), x.shape[0], _ptr(sigma), _ptr(grad), None, 0, _stream()))
    return sigma, grad


def _safe_normalize(v, eps=1e-8):
    return v / torch.linalg.vector_norm(v, dim=-1, keepdim=True).clamp_min(eps)


def ExtractMesh(renderer, threshold, resolution=256, bbox=None, colors=True, precision=L.NRF_PREC_F32, normals="lattice"):
    """DensityGrid -> Isosurface -> per-vertex colour: sigmoid of RunNetwork's rgb at the vertex seen along -normal (a ray hitting the surface head-on), in chunks.
    normals="lattice": the isosurface's central-difference normals; "field": -safe_normalize(DensityGradient(vertices)), the field's own analytic normal
    (also the colour's view direction)."""
    if normals not in ("lattice", "field"):
        raise L.NrfError(f"ExtractMesh: normals must be 'lattice' or 'field', got {normals!r}")
    bb = _bbox(renderer, bbox)
    sigma = DensityGrid(renderer, bb, resolution)
    verts, faces, lattice_normals = Isosurface(sigma, bb, threshold)
    del sigma
    normals = lattice_normals if normals == "lattice" else -_safe_normalize(DensityGradient(renderer, verts)[1])
    rgb = None
    if colors:
        rgb = torch.empty_like(verts)
        for i in range(0, verts.shape[0], COLOR_CHUNK):
            v = verts[i:i + COLOR_CHUNK]
            raw = renderer.RunNetwork(v[:, None, :], (-normals[i:i + COLOR_CHUNK]).contiguous(), precision)
            rgb[i:i + COLOR_CHUNK] = torch.sigmoid(raw[:, 0, :3])          # RawToOutputs's rgb (NeRFRenderer.h:250)
    return Mesh(verts, faces, normals, rgb)


def SavePLY(path, mesh):
    """Binary little-endian PLY: x y z nx ny nz (float), red green blue (uchar, clamp(round(255 c))) when the mesh has colours, relevancy (float, column 0 of
    Relevancy) when it has one, faces as `list uchar int vertex_indices`."""
    v = mesh.Vertices.detach().cpu().numpy().astype("<f4")
    n = mesh.Normals.detach().cpu().numpy().astype("<f4")
    fc = mesh.Faces.detach().cpu().numpy().astype("<i4")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if mesh.Colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    if mesh.Relevancy is not None:
        fields += [("relevancy", "<f4")]
    rec = np.empty(v.shape[0], dtype=np.dtype(fields))
    for k, name in enumerate(("x", "y", "z")):
        rec[name] = v[:, k]
        rec["n" + name] = n[:, k]
    if mesh.Colors is not None:
        c = np.clip(np.rint(mesh.Colors.detach().cpu().numpy().astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
        for k, name in enumerate(("red", "green", "blue")):
            rec[name] = c[:, k]
    if mesh.Relevancy is not None:
        r = mesh.Relevancy.detach().cpu()
        rec["relevancy"] = (r[:, 0] if r.dim() == 2 else r.reshape(-1)).numpy().astype("<f4")
    frec = np.empty(fc.shape[0], dtype=np.dtype([("n", "u1"), ("idx", "<i4", (3,))]))
    frec["n"] = 3
    frec["idx"] = fc
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}"]
    head += [f"property float {name}" for name, _ in fields[:6]]
    if mesh.Colors is not None:
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    if mesh.Relevancy is not None:
        head += ["property float relevancy"]
    head += [f"element face {fc.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(rec.tobytes())
        fh.write(frec.tobytes())
