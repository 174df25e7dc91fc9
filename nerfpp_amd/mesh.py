"""Mesh export: DensityGrid, Isosurface, ExtractMesh, MeshComponents, FilterComponents, SimplifyMesh, SimplifyToFaces, BuildAdjacency, MeshTopology,
VertexNormals, SmoothMesh, SmoothAttributes and SavePLY over the C ABI (include/nerfpp_hip.h, mesh.hip, components.hip, simplify.hip, smooth.hip).

The reference has no mesh export; the names follow the mirror's style.  The density lattice is the exact-fp32 sigma of the renderer's network
(== RunNetwork(..., NRF_PREC_F32)[..., 3] bit for bit); the isosurface is marching tetrahedra on the Kuhn split of each cell, in an order fixed by integer
prefix scans (two extractions give the same arrays).  Simplification is vertex clustering on a uniform grid with coincident faces settled by their net orientation;
every output is fixed by integers and single-rounding steps (tests/simplify_ref.py restates them).
"""
import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from .modules import _HashBase, _ptr, _stream, _dev_f32

COLOR_CHUNK = 1 << 18        # vertices per RunNetwork call of ExtractMesh
# NRF_SIMPLIFY_* of the header (tests/test_simplify_host.py holds them to it)
SIMPLIFY_MAX_DIM, SIMPLIFY_MAX_CELLS, SIMPLIFY_POS_MEAN, SIMPLIFY_POS_MEMBER = 1024, 1 << 27, 0, 1
_POSITIONS = {"mean": SIMPLIFY_POS_MEAN, "member": SIMPLIFY_POS_MEMBER}
# NRF_ADJ_* / NRF_SMOOTH_* / NRF_NORMALS_* of the header (tests/test_smooth_host.py holds them to it)
ADJ_BOUNDARY, ADJ_NONMANIFOLD, ADJ_SHORT_ROW, SMOOTH_MAX_CHANNELS = 1, 2, 32, 4
SMOOTH_FREE, SMOOTH_FIXED, SMOOTH_CURVE = 0, 1, 2
NORMALS_AREA, NORMALS_UNIT = 0, 1
_BOUNDARIES = {"free": SMOOTH_FREE, "fixed": SMOOTH_FIXED, "curve": SMOOTH_CURVE}
_WEIGHTINGS = {"area": NORMALS_AREA, "unit": NORMALS_UNIT}
_ATTRIBUTES = ("Colors", "Relevancy")


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
                min_component_faces=0, simplify_cell=None, smooth_iterations=0, union_resolution=None):
    """DensityGrid -> Isosurface -> per-vertex colour: sigmoid of RunNetwork's rgb at the vertex seen along -normal (a ray hitting the surface head-on), in chunks.
    normals="lattice": the isosurface's central-difference normals; "field": -safe_normalize(DensityGradient(vertices)), the field's own analytic normal
    (also the colour's view direction).  keep_largest / min_component_faces: FilterComponents on the bare isosurface, before the field normals and the colours,
    so a dropped floater costs no network evaluation.  simplify_cell: SimplifyMesh(cell_size=simplify_cell) after that filter and before the field normals and the
    colours, for the same reason; the lattice normals of the result are those of each cluster's representative.  smooth_iterations > 0: SmoothMesh(iterations=
    smooth_iterations) with its defaults after both and before the colours; the normals are then VertexNormals of the smoothed faces whatever `normals` says (neither
    the lattice's nor the field's belong to the moved geometry).  0 (the default) issues no call.  union_resolution: voxel.RemeshUnion(resolution=union_resolution)
    after the component filter and before the simplification, the normals and the colours: the interior shells of the isosurface vanish into the solid around them
    without any camera, and the normals are those of the remesh's lattice.  None (the default) issues no call."""
    if normals not in ("lattice", "field"):
        raise L.NrfError(f"ExtractMesh: normals must be 'lattice' or 'field', got {normals!r}")
    smooth_iterations = int(smooth_iterations)
    if smooth_iterations < 0:
        raise L.NrfError(f"ExtractMesh: smooth_iterations must be >= 0, got {smooth_iterations}")
    bb = _bbox(renderer, bbox)
    sigma = DensityGrid(renderer, bb, resolution)
    verts, faces, lattice_normals = Isosurface(sigma, bb, threshold)
    del sigma
    if keep_largest is not None or min_component_faces > 0:
        kept = FilterComponents(Mesh(verts, faces, lattice_normals), keep_largest, min_component_faces)
        verts, faces, lattice_normals = kept.Vertices, kept.Faces, kept.Normals
    if union_resolution is not None:
        from .voxel import RemeshUnion
        union = RemeshUnion(Mesh(verts, faces, lattice_normals), resolution=union_resolution)
        verts, faces, lattice_normals = union.Vertices, union.Faces, union.Normals
    if simplify_cell is not None:
        small = SimplifyMesh(Mesh(verts, faces, lattice_normals), cell_size=simplify_cell)
        verts, faces, lattice_normals = small.Vertices, small.Faces, small.Normals
    if smooth_iterations > 0:
        smooth = SmoothMesh(Mesh(verts, faces, lattice_normals), iterations=smooth_iterations)
        verts, normals = smooth.Vertices, smooth.Normals
    else:
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


def _finite_box(verts):
    """(lo [3], hi [3]) float32 numpy: the box of the finite vertices ((0, 0) where there is none): one host synchronisation"""
    v = verts[torch.isfinite(verts).all(dim=1)]
    if v.shape[0] == 0:
        return np.zeros(3, np.float32), np.zeros(3, np.float32)
    return v.min(dim=0).values.cpu().numpy().astype(np.float32), v.max(dim=0).values.cpu().numpy().astype(np.float32)


def _cube_dims(extent, n_long):
    """Per axis the number of cells of edge max(extent) / n_long that cover it, 1 .. SIMPLIFY_MAX_DIM: as cubic as whole numbers of cells allow"""
    ext = np.asarray(extent, np.float64)
    cell = float(ext.max()) / n_long if ext.max() > 0 else 1.0
    return tuple(int(min(max(math.ceil(e / cell - 1e-9), 1), SIMPLIFY_MAX_DIM)) for e in ext)


def _simplify_grid(verts, cell_size, resolution, bbox):
    """(box [6] float32 numpy, (nx, ny, nz)) of SimplifyMesh"""
    if (cell_size is None) == (resolution is None):
        raise L.NrfError("SimplifyMesh: give exactly one of cell_size and resolution")
    if bbox is None:
        lo, hi = _finite_box(verts)
    else:
        b = np.asarray(torch.as_tensor(bbox).detach().cpu().numpy() if torch.is_tensor(bbox) else bbox, np.float32).reshape(6)
        lo, hi = b[:3].copy(), b[3:].copy()
    if cell_size is not None:
        cell = float(cell_size)
        if not (math.isfinite(cell) and cell > 0.0):
            raise L.NrfError(f"SimplifyMesh: cell_size must be finite and > 0, got {cell_size!r}")
        ext = hi.astype(np.float64) - lo.astype(np.float64)
        dims = tuple(int(min(max(math.ceil(e / cell), 1), SIMPLIFY_MAX_DIM)) for e in ext)
        hi = (lo.astype(np.float64) + np.asarray(dims, np.float64) * cell).astype(np.float32)          # cube cells; an axis of zero extent is one cell thick
    else:
        dims = _resolution(resolution)
        ext = hi.astype(np.float64) - lo.astype(np.float64)
        if (ext <= 0).any():          # an axis of zero extent is widened by one cell: the largest cell edge of the other axes, 1 where there is none
            edge = max([e / n for e, n in zip(ext, dims) if e > 0], default=1.0)
            hi = np.where(ext > 0, hi, (lo.astype(np.float64) + edge).astype(np.float32)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([lo, hi]), np.float32), dims


class _Simplifier:
    """One mesh, one workspace, any number of count calls and the emit call after the last of them"""
    def __init__(self, mesh):
        self.verts = _dev_f32(mesh.Vertices).reshape(-1, 3)
        self.faces = mesh.Faces.to(device=self.verts.device, dtype=torch.int32).reshape(-1, 3).contiguous()
        self.nv, self.nf = int(self.verts.shape[0]), int(self.faces.shape[0])
        self.ws = None

    def count(self, box, dims):
        lib = L.lib()
        need = int(lib.nrf_mesh_simplify_workspace_bytes(self.nv, self.nf, *dims))
        if self.ws is None or self.ws.numel() < need:
            self.ws = None          # the old one goes first
            self.ws = torch.empty((max(1, need),), device=self.verts.device, dtype=torch.uint8)
        self.stats = torch.zeros((4,), device=self.verts.device, dtype=torch.int32)
        nv, nf = C.c_int64(0), C.c_int64(0)
        L.check(lib.nrf_mesh_simplify_count(_ptr(self.verts), self.nv, _ptr(self.faces), self.nf, box.ctypes.data_as(C.c_void_p), *dims, C.addressof(nv), C.addressof(nf),
                                            _ptr(self.stats), _ptr(self.ws), self.ws.numel(), _stream()))
        self.box, self.dims, self.out = box, dims, (int(nv.value), int(nf.value))
        return self.out

    def emit(self, position):
        dev = self.verts.device
        nv, nf = self.out
        verts = torch.empty((nv, 3), device=dev, dtype=torch.float32)
        faces = torch.empty((nf, 3), device=dev, dtype=torch.int32)
        rep = torch.empty((nv,), device=dev, dtype=torch.int32)
        face_src = torch.empty((nf,), device=dev, dtype=torch.int32)
        cluster = torch.empty((self.nv,), device=dev, dtype=torch.int32)
        L.check(L.lib().nrf_mesh_simplify_emit(_ptr(self.verts), self.nv, _ptr(self.faces), self.nf, self.box.ctypes.data_as(C.c_void_p), *self.dims, position, nv, nf,
                                               _ptr(verts), _ptr(faces), _ptr(rep), _ptr(face_src), _ptr(cluster), _ptr(self.ws), self.ws.numel(), _stream()))
        return verts, faces, rep, face_src, cluster


def _position(position):
    if position not in _POSITIONS:
        raise L.NrfError(f"position must be 'mean' or 'member', got {position!r}")
    return _POSITIONS[position]


def _simplified(mesh, s, position, return_maps):
    verts, faces, rep, face_src, cluster = s.emit(position)
    at = rep.to(torch.int64)

    def gather(t):
        return None if t is None else t.to(verts.device)[at]
    out = Mesh(verts, faces, gather(mesh.Normals), gather(mesh.Colors), gather(mesh.Relevancy))
    return (out, (cluster, face_src, rep, s.stats)) if return_maps else out


def SimplifyMesh(mesh, cell_size=None, resolution=None, bbox=None, position="mean", return_maps=False):
    """Vertex clustering (nrf_mesh_simplify_count / _emit): the vertices of every cell of a uniform grid become one vertex, faces with two corners in one cell
    disappear, and of the faces that land on the same three cells the one their net orientation names survives (none where the orientations cancel, so a pocket
    folded onto itself leaves no fin).  Give exactly one of cell_size (cube cells: n = clamp(ceil(extent / cell_size), 1, 1024) per axis, bmax = bmin + n * cell_size)
    and resolution (an int or (nx, ny, nz) over the box).  bbox [6] defaults to the box of the mesh's finite vertices (one host synchronisation); an axis of zero
    extent is widened by one cell.  position="mean": the mean of the vertices a cell's surviving or collapsed faces use, on a 2^-20 fixed-point lattice inside the
    cell, so it does not depend on their order; "member": the coordinates of the representative, the input vertex nearest that mean (lowest index on a tie).
    Normals, Colors and Relevancy are the representative's.  Kept faces stay in input order with their winding, output vertices ascend in cell index, and two runs
    give the same bits.  An empty result is a valid empty Mesh.  return_maps: also (cluster [V] int32: the output vertex of every input vertex or -1, face_src [F']
    int32: the input face of every output face, rep [V'] int32: the representative, stats [4] int32: faces with a bad index, with a non-finite vertex, collapsed,
    removed as coincident).  Vertex clustering does not preserve topology in general."""
    pos = _position(position)
    s = _Simplifier(mesh)
    box, dims = _simplify_grid(s.verts, cell_size, resolution, bbox)
    s.count(box, dims)
    return _simplified(mesh, s, pos, return_maps)


def SimplifyToFaces(mesh, target_faces, position="mean"):
    """(mesh, n): SimplifyMesh(mesh, resolution=dims) on the grid of n cells along the longest axis of the box of the finite vertices -- and as many cells of that
    edge as cover each other axis, so the cells are as cubic as whole numbers allow; (n, n, n) for a cubic box -- for the largest n tried whose face count is
    <= target_faces.  n is bisected in [1, 1024] with count calls only (at most 10, one more before the emit); grids beyond the library's cell limit are not tried.
    The face count is NOT strictly monotone in n (a finer grid can cancel a pocket a coarser one kept), so a larger n that also qualifies may exist; n = 1 always
    qualifies, with 0 faces."""
    pos = _position(position)
    s = _Simplifier(mesh)
    lo_v, hi_v = _finite_box(s.verts)
    ext = hi_v.astype(np.float64) - lo_v.astype(np.float64)

    def grid(n):
        return _simplify_grid(s.verts, None, _cube_dims(ext, n), np.concatenate([lo_v, hi_v]))
    lo, hi = 1, SIMPLIFY_MAX_DIM + 1          # lo qualifies, hi does not (or is out of range)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        box, dims = grid(mid)
        if dims[0] * dims[1] * dims[2] <= SIMPLIFY_MAX_CELLS and s.count(box, dims)[1] <= int(target_faces):
            lo = mid
        else:
            hi = mid
    s.count(*grid(lo))
    return _simplified(mesh, s, pos, False), lo


@dataclass
class MeshAdjacency:
    """nrf_mesh_adjacency_*: the rows of the header's ADJACENCY, device tensors"""
    FaceStart: torch.Tensor      # [V + 1] int64
    FaceList: torch.Tensor       # [3 * valid faces] int32: per vertex its valid faces, ascending
    NbrStart: torch.Tensor       # [V + 1] int64
    Nbr: torch.Tensor            # [2 * edges] int32: per vertex its distinct neighbours, ascending
    NbrFaces: torch.Tensor       # [2 * edges] int32: the faces on that edge (1 boundary, 2 interior, more non-manifold)
    Flags: torch.Tensor          # [V] uint8: ADJ_BOUNDARY | ADJ_NONMANIFOLD, 0 for an unused vertex
    Stats: torch.Tensor          # [8] int64: bad-index faces, repeated-corner faces, used vertices, edges, boundary edges, non-manifold edges, longest rows
    NumVerts: int
    NumFaces: int

    @property
    def stats(self):
        """Stats as a dict of Python ints (one host synchronisation)"""
        names = ("bad_index", "repeated_corner", "used_vertices", "edges", "boundary_edges", "nonmanifold_edges", "longest_face_row", "longest_nbr_row")
        return dict(zip(names, (int(v) for v in self.Stats.cpu().tolist())))


def _faces_of(mesh_or_faces, n_verts, who):
    """(faces [F, 3] int32 contiguous on the GPU, V) of a Mesh or of faces over n_verts vertices (default: the largest index + 1)"""
    if isinstance(mesh_or_faces, Mesh):
        faces, v = mesh_or_faces.Faces, int(mesh_or_faces.Vertices.shape[0]) if n_verts is None else int(n_verts)
    else:
        faces = torch.as_tensor(mesh_or_faces)
        v = (max(int(faces.max()) + 1, 0) if faces.numel() else 0) if n_verts is None else int(n_verts)
    if faces.numel() % 3 != 0 or v < 0:
        raise L.NrfError(f"{who}: faces must be [F, 3] and n_verts >= 0, got {tuple(faces.shape)} and {v}")
    dev = faces.device if faces.is_cuda else torch.device("cuda", torch.cuda.current_device())
    return faces.to(device=dev, dtype=torch.int32).reshape(-1, 3).contiguous(), v


def BuildAdjacency(mesh_or_faces, n_verts=None):
    """nrf_mesh_adjacency_count / _emit: the MeshAdjacency of a Mesh or of faces [F, 3] over n_verts vertices (default: the largest index + 1).  A face with a
    corner outside [0, n_verts) or with two equal corners is left out and counted.  Every array but FaceList is the same for any order of the faces; two runs give
    the same bits."""
    faces, v = _faces_of(mesh_or_faces, n_verts, "BuildAdjacency")
    f, dev, lib = int(faces.shape[0]), faces.device, L.lib()
    ws = torch.empty((max(1, int(lib.nrf_mesh_adjacency_workspace_bytes(v, f))),), device=dev, dtype=torch.uint8)
    ni, nn = C.c_int64(0), C.c_int64(0)
    L.check(lib.nrf_mesh_adjacency_count(_ptr(faces), v, f, C.addressof(ni), C.addressof(nn), _ptr(ws), ws.numel(), _stream()))
    ni, nn = int(ni.value), int(nn.value)
    adj = MeshAdjacency(torch.empty((v + 1,), device=dev, dtype=torch.int64), torch.empty((ni,), device=dev, dtype=torch.int32),
                        torch.empty((v + 1,), device=dev, dtype=torch.int64), torch.empty((nn,), device=dev, dtype=torch.int32),
                        torch.empty((nn,), device=dev, dtype=torch.int32), torch.empty((v,), device=dev, dtype=torch.uint8),
                        torch.empty((8,), device=dev, dtype=torch.int64), v, f)
    L.check(lib.nrf_mesh_adjacency_emit(_ptr(faces), v, f, ni, nn, _ptr(adj.FaceStart), _ptr(adj.FaceList), _ptr(adj.NbrStart), _ptr(adj.Nbr), _ptr(adj.NbrFaces),
                                        _ptr(adj.Flags), _ptr(adj.Stats), _ptr(ws), ws.numel(), _stream()))
    return adj


def MeshTopology(mesh_or_adjacency):
    """How a mesh hangs together, from the adjacency's statistics (one host synchronisation): vertices_used, edges, faces_valid, boundary_edges,
    nonmanifold_edges, euler = vertices_used - edges + faces_valid, closed (no boundary edge) and manifold (no edge with more than two faces)."""
    adj = mesh_or_adjacency if isinstance(mesh_or_adjacency, MeshAdjacency) else BuildAdjacency(mesh_or_adjacency)
    s = adj.stats
    faces_valid = adj.NumFaces - s["bad_index"] - s["repeated_corner"]
    return dict(vertices_used=s["used_vertices"], edges=s["edges"], faces_valid=faces_valid, boundary_edges=s["boundary_edges"],
                nonmanifold_edges=s["nonmanifold_edges"], euler=s["used_vertices"] - s["edges"] + faces_valid, closed=s["boundary_edges"] == 0,
                manifold=s["nonmanifold_edges"] == 0)


def _adjacency_for(mesh, adjacency, who):
    adj = BuildAdjacency(mesh) if adjacency is None else adjacency
    if not isinstance(adj, MeshAdjacency) or adj.NumVerts != int(mesh.Vertices.shape[0]) or adj.NumFaces != int(mesh.Faces.shape[0]):
        raise L.NrfError(f"{who}: the adjacency is not a MeshAdjacency of this mesh's {int(mesh.Vertices.shape[0])} vertices and {int(mesh.Faces.shape[0])} faces")
    return adj


def VertexNormals(mesh, weighting="area", adjacency=None):
    """nrf_mesh_vertex_normals: [V, 3] unit normals from the faces -- per vertex the sum of its faces' e1 x e2 ("area": weighted by twice the face area; "unit":
    every face alike), added in ascending face index and normalised; 0 for a vertex without a face or with a vanishing sum.  Outward for the counter-clockwise
    faces of this package.  Deterministic, not invariant under a permutation of the faces."""
    if weighting not in _WEIGHTINGS:
        raise L.NrfError(f"VertexNormals: weighting must be 'area' or 'unit', got {weighting!r}")
    adj = _adjacency_for(mesh, adjacency, "VertexNormals")
    verts = _dev_f32(mesh.Vertices).reshape(-1, 3)
    faces = mesh.Faces.to(device=verts.device, dtype=torch.int32).reshape(-1, 3).contiguous()
    out = torch.empty_like(verts)
    L.check(L.lib().nrf_mesh_vertex_normals(_ptr(verts), verts.shape[0], _ptr(faces), faces.shape[0], _ptr(adj.FaceStart), _ptr(adj.FaceList), adj.FaceList.numel(),
                                            _WEIGHTINGS[weighting], _ptr(out), _stream()))
    return out


def _smooth_args(who, iterations, lam, mu, boundary):
    iterations, lam, mu = int(iterations), float(lam), float(mu)
    if boundary not in _BOUNDARIES:
        raise L.NrfError(f"{who}: boundary must be 'free', 'fixed' or 'curve', got {boundary!r}")
    if iterations < 0 or not (math.isfinite(lam) and math.isfinite(mu)):
        raise L.NrfError(f"{who}: iterations must be >= 0 and lam, mu finite, got {iterations}, {lam}, {mu}")
    return iterations, lam, mu, _BOUNDARIES[boundary]


def _smooth(who, x, adj, iterations, lam, mu, boundary):
    """nrf_mesh_smooth of x [V] or [V, C], C <= SMOOTH_MAX_CHANNELS -> a new tensor of x's shape"""
    x = _dev_f32(x)
    v = adj.NumVerts
    if x.dim() not in (1, 2) or x.shape[0] != v or not 1 <= (x.shape[1] if x.dim() == 2 else 1) <= SMOOTH_MAX_CHANNELS:
        raise L.NrfError(f"{who}: a smoothed array must be [{v}] or [{v}, 1 .. {SMOOTH_MAX_CHANNELS}], got {tuple(x.shape)}")
    x = x.contiguous()
    out, tmp = torch.empty_like(x), torch.empty_like(x)
    L.check(L.lib().nrf_mesh_smooth(_ptr(x), _ptr(out), _ptr(tmp), v, x.shape[1] if x.dim() == 2 else 1, iterations, lam, mu, boundary, _ptr(adj.NbrStart), _ptr(adj.Nbr),
                                    _ptr(adj.NbrFaces), _ptr(adj.Flags), adj.Nbr.numel(), _stream()))
    return out


def _attributes(who, mesh, names):
    names = (names,) if isinstance(names, str) else tuple(names)
    for n in names:
        if n not in _ATTRIBUTES or getattr(mesh, n) is None:
            raise L.NrfError(f"{who}: {n!r} is not an attribute this mesh carries (of {_ATTRIBUTES})")
    return names


def SmoothMesh(mesh, iterations=10, lam=0.5, mu=-0.53, boundary="curve", attributes=(), recompute_normals=True, adjacency=None):
    """nrf_mesh_smooth on the vertices: Taubin's lambda|mu filter -- per iteration a step x += lam * (mean of the neighbours - x), then one with mu < -lam that undoes
    the shrinkage; mu=0 is the plain Laplacian, which shrinks.  boundary: "free" treats every vertex alike, "fixed" leaves the vertices of boundary edges where they
    are, "curve" smooths them along the boundary only (over their neighbours across boundary edges).  Faces are unchanged.  attributes: names of "Colors" /
    "Relevancy" to smooth by the same call; the others are carried as they are.  Normals are VertexNormals of the new geometry unless recompute_normals=False.
    adjacency: BuildAdjacency(mesh) when not given.  Sums run over the neighbours in ascending index, no atomics: two runs give the same bits."""
    iterations, lam, mu, mode = _smooth_args("SmoothMesh", iterations, lam, mu, boundary)
    names = _attributes("SmoothMesh", mesh, attributes)
    adj = _adjacency_for(mesh, adjacency, "SmoothMesh")
    out = Mesh(_smooth("SmoothMesh", mesh.Vertices.reshape(-1, 3), adj, iterations, lam, mu, mode), mesh.Faces, mesh.Normals, mesh.Colors, mesh.Relevancy)
    for n in names:
        setattr(out, n, _smooth("SmoothMesh", getattr(mesh, n), adj, iterations, lam, mu, mode))
    if recompute_normals:
        out.Normals = VertexNormals(out, adjacency=adj)
    return out


def SmoothAttributes(mesh, names, iterations, lam=0.5, mu=0.0, boundary="free", adjacency=None):
    """nrf_mesh_smooth on the named attributes ("Colors", "Relevancy") alone: vertices, faces and normals are the input's own tensors.  Made to denoise
    query.VertexRelevancy before query.SegmentMesh; the defaults are the plain Laplacian, which only averages."""
    iterations, lam, mu, mode = _smooth_args("SmoothAttributes", iterations, lam, mu, boundary)
    names = _attributes("SmoothAttributes", mesh, names)
    adj = _adjacency_for(mesh, adjacency, "SmoothAttributes")
    out = Mesh(mesh.Vertices, mesh.Faces, mesh.Normals, mesh.Colors, mesh.Relevancy)
    for n in names:
        setattr(out, n, _smooth("SmoothAttributes", getattr(mesh, n), adj, iterations, lam, mu, mode))
    return out


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
