"""Mesh export: DensityGrid, Isosurface, ExtractMesh, MeshComponents, FilterComponents and SavePLY over the C ABI (include/nerfpp_hip.h, mesh.hip,
components.hip).

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


def ExtractMesh(renderer, threshold, resolution=256, bbox=None, colors=True, precision=L.NRF_PREC_F32, normals="lattice", keep_largest=None,
                min_component_faces=0):
    """DensityGrid -> Isosurface -> per-vertex colour: sigmoid of RunNetwork's rgb at the vertex seen along -normal (a ray hitting the surface head-on), in chunks.
    normals="lattice": the isosurface's central-difference normals; "field": -safe_normalize(DensityGradient(vertices)), the field's own analytic normal
    (also the colour's view direction).  keep_largest / min_component_faces: FilterComponents on the bare isosurface, before the field normals and the colours,
    so a dropped floater costs no network evaluation."""
    if normals not in ("lattice", "field"):
        raise L.NrfError(f"ExtractMesh: normals must be 'lattice' or 'field', got {normals!r}")
    bb = _bbox(renderer, bbox)
    sigma = DensityGrid(renderer, bb, resolution)
    verts, faces, lattice_normals = Isosurface(sigma, bb, threshold)
    del sigma
    if keep_largest is not None or min_component_faces > 0:
        kept = FilterComponents(Mesh(verts, faces, lattice_normals), keep_largest, min_component_faces)
        verts, faces, lattice_normals = kept.Vertices, kept.Faces, kept.Normals
    normals = lattice_normals if normals == "lattice" else -_safe_normalize(DensityGradient(renderer, verts)[1])
    rgb = None
    if colors:
        rgb = torch.empty_like(verts)
        for i in range(0, verts.shape[0], COLOR_CHUNK):
            v = verts[i:i + COLOR_CHUNK]
            raw = renderer.RunNetwork(v[:, None, :], (-normals[i:i + COLOR_CHUNK]).contiguous(), precision)
            rgb[i:i + COLOR_CHUNK] = torch.sigmoid(raw[:, 0, :3])          # RawToOutputs's rgb (NeRFRenderer.h:250)
    return Mesh(verts, faces, normals, rgb)


def _submesh(mesh, keep_faces, relevancy=None):
    """The sub-mesh of the faces keep_faces [F] bool: the vertices they use in ascending original order, faces re-indexed; normals, colours and `relevancy` [V, ...]
    follow their vertices.  Any torch device."""
    faces = mesh.Faces.to(torch.int64)[keep_faces]
    used = torch.zeros((mesh.Vertices.shape[0],), dtype=torch.bool, device=faces.device)
    used[faces.reshape(-1)] = True
    old = torch.nonzero(used).reshape(-1)
    remap = torch.full((used.shape[0],), -1, dtype=torch.int64, device=faces.device)
    remap[old] = torch.arange(old.numel(), dtype=torch.int64, device=faces.device)

    def sub(t):
        return None if t is None else t[old]
    return Mesh(mesh.Vertices[old], remap[faces].to(mesh.Faces.dtype), mesh.Normals[old], sub(mesh.Colors), sub(relevancy))


def MeshComponents(mesh_or_faces, n_verts=None):
    """nrf_mesh_components: (labels [V] int32, K) of a Mesh or of faces [F, 3] over n_verts vertices (default: the largest index + 1).  Vertices that share a face
    share a label, a vertex used by no face gets -1; components are numbered 0 .. K-1 by their smallest vertex id, so the labels are the same on every run.  The
    component of a face is the label of its first vertex.  An index outside [0, n_verts) raises."""
    if isinstance(mesh_or_faces, Mesh):
        faces, v = mesh_or_faces.Faces, int(mesh_or_faces.Vertices.shape[0]) if n_verts is None else int(n_verts)
    else:
        faces = torch.as_tensor(mesh_or_faces)
        v = (int(faces.max()) + 1 if faces.numel() else 0) if n_verts is None else int(n_verts)
    dev = faces.device if faces.is_cuda else torch.device("cuda", torch.cuda.current_device())
    faces = faces.to(device=dev, dtype=torch.int32).reshape(-1, 3).contiguous()
    lib = L.lib()
    labels = torch.empty((v,), device=dev, dtype=torch.int32)
    ws = torch.empty((max(1, int(lib.nrf_mesh_components_workspace_bytes(v, faces.shape[0]))),), device=dev, dtype=torch.uint8)
    k = C.c_int64()
    L.check(lib.nrf_mesh_components(_ptr(faces), v, faces.shape[0], _ptr(labels), C.byref(k), _ptr(ws), ws.numel(), _stream()))
    return labels, int(k.value)


def FilterComponents(mesh, keep_largest=None, min_faces=0, labels=None):
    """The sub-mesh of whole connected components; the size of a component is its face count.  keep_largest=k keeps the k largest (ties: the lower label first),
    min_faces drops the smaller ones; given both, a component must pass both.  Kept vertices stay in ascending original order, faces are re-indexed, normals,
    colours and relevancy follow their vertices.  labels: MeshComponents(mesh)[0] when not given; with labels the function runs on any torch device and calls no
    kernel of the library."""
    labels = MeshComponents(mesh)[0] if labels is None else torch.as_tensor(labels)
    labels = labels.to(device=mesh.Faces.device, dtype=torch.int64)
    face_label = labels[mesh.Faces[:, 0].to(torch.int64)]
    sizes = torch.bincount(face_label, minlength=int(labels.max()) + 1 if labels.numel() else 0)
    keep = sizes >= int(min_faces)
    if keep_largest is not None:
        # stable descending sort of the sizes (in label order): equal sizes keep the lower label first
        top = torch.sort(sizes, descending=True, stable=True).indices[:max(int(keep_largest), 0)]
        largest = torch.zeros_like(keep)
        largest[top] = True
        keep &= largest
    return _submesh(mesh, keep[face_label], mesh.Relevancy)


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
