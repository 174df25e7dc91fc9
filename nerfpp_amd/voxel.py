"""What is inside a mesh: WindingGrid, MeshToSDF, SDFVolume, RemeshUnion, VoxelVolume and VolumeIoU over the C ABI (include/nerfpp_hip.h, voxel.hip).

The reference has no voxeliser; the names follow the mirror's style.  nrf_mesh_voxelize scan-converts the project's own Mesh onto the lattice of DensityGrid: an
integer winding number per lattice point (an orthographic raster along +z with the rasteriser's exact coverage, then a suffix sum down every column) and a truncated
distance with the nearest face (a scatter of ClosestOnMesh's point-to-triangle function over each face's dilated lattice box).  Both are integer atomics over stated
fp32 operations, so tests/voxel_ref.py equals every output bit for bit, two runs agree, and the order of the face list does not matter.  The signed lattice goes to
the existing Isosurface: a closed, uniformly sampled remesh, offset surfaces, the union of nested shells without any camera, and volumetric IoU.
"""
import ctypes as C
import dataclasses
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as L
from . import mesh as M
from .geometry import _host_box, _mesh_arrays, _workspace
from .modules import _ptr, _stream, _dev_f32

WIDE_COLUMNS, WIDE_POINTS = 256, 256          # NRF_VOXEL_WIDE_* of the header (tests/test_voxel_host.py holds them to it)
DEFAULT_TRUNC_STEPS = 3.0
RULES = {"nonzero": L.NRF_VOX_NONZERO, "positive": L.NRF_VOX_POSITIVE, "odd": L.NRF_VOX_ODD}
_INSIDE = {L.NRF_VOX_NONZERO: lambda w: w != 0, L.NRF_VOX_POSITIVE: lambda w: w > 0, L.NRF_VOX_ODD: lambda w: (w & 1) != 0}          # step 10 of the header
_TRANSFER = ("Colors", "Normals", "Relevancy")


def _rule(who, rule):
    if rule not in RULES:
        raise L.NrfError(f"{who}: rule must be one of {sorted(RULES)}, got {rule!r}")
    return RULES[rule]


def _steps(box, dims):
    """The lattice steps as the kernels form them: (bmax - bmin) / (float)(n - 1), fp32 per operation"""
    return (box[3:] - box[:3]) / (np.asarray(dims) - 1).astype(np.float32)


def _lattice(who, mesh, bbox, resolution, trunc):
    """(box [6] f32 on the host, (nx, ny, nz), trunc, whether the box is the caller's).  Resolution and box as DensityGrid's.  bbox=None: the bounds of the finite
    vertices (one host synchronisation) padded by trunc plus one lattice step, so nothing is clipped and the surface never touches the lattice's rim; trunc=None:
    DEFAULT_TRUNC_STEPS of the largest step."""
    dims = M._resolution(resolution)
    if min(dims) < 2:
        raise L.NrfError(f"{who}: resolution {resolution!r} needs at least 2 lattice points per axis")
    if bbox is not None:
        box = _host_box(bbox)
        t = DEFAULT_TRUNC_STEPS * float(_steps(box, dims).max()) if trunc is None else float(trunc)
        return box, dims, t, True
    lo, hi = (v.astype(np.float64) for v in M._finite_box(_dev_f32(mesh.Vertices).reshape(-1, 3)))
    n = np.asarray(dims, np.float64) - 1.0
    ext = np.maximum(hi - lo, 1e-6 * np.maximum(np.abs(hi).max(), 1.0))
    if trunc is None:
        # pad = (k + 1) steps on each side, step = (ext + 2 pad) / n: step = ext / (n - 2 (k + 1)); needs more than 2 (k + 1) intervals per axis
        free = n - 2.0 * (DEFAULT_TRUNC_STEPS + 1.0)
        if free.min() < 1.0:
            raise L.NrfError(f"{who}: resolution {resolution!r} leaves no room for the default truncation of {DEFAULT_TRUNC_STEPS:g} steps on each side; give trunc or bbox")
        t = DEFAULT_TRUNC_STEPS * float((ext / free).max())
    else:
        t = float(trunc)
    free = n - 2.0
    step = (ext + 2.0 * t) / free          # the pad is trunc plus one step of the padded lattice
    if free.min() < 1.0 or not np.isfinite(step).all():
        raise L.NrfError(f"{who}: resolution {resolution!r} is too small to pad the mesh's bounds; give bbox")
    pad = t * (1.0 + 1e-6) + step
    box = np.concatenate([lo - pad, hi + pad]).astype(np.float32)
    return box, dims, t, False


def _voxelize(who, mesh, box, dims, trunc, rule, winding, sdf, face):
    """One nrf_mesh_voxelize; winding / sdf / face say which outputs are made -> (winding, sdf, face, stats [4] int32 on the device)"""
    verts, faces = _mesh_arrays(mesh)
    dev = verts.device
    nx, ny, nz = dims
    shape = (nz, ny, nx)
    w = torch.empty(shape, device=dev, dtype=torch.int32) if winding else None
    s = torch.empty(shape, device=dev, dtype=torch.float32) if sdf else None
    f = torch.empty(shape, device=dev, dtype=torch.int32) if face else None
    stats = torch.zeros((4,), device=dev, dtype=torch.int32)          # the uint32 counts of one call are at most F < 2^31
    lib = L.lib()
    nv, nf = int(verts.shape[0]), int(faces.shape[0])
    nbytes = int(lib.nrf_mesh_voxelize_workspace_bytes(nv, nf, nx, ny, nz))
    if nbytes == 0:
        raise L.NrfError(f"{who}: a lattice of {nx} x {ny} x {nz} (each >= 2, fewer than 2^31 points) with {nv} vertices and {nf} faces is refused")
    if not (sdf or face):
        nbytes -= 8 * nx * ny * nz          # the key lattice is the last piece and only the distance pass reads it: a short workspace is accepted
    ws = _workspace(nbytes, dev)
    L.check(lib.nrf_mesh_voxelize(_ptr(verts), nv, _ptr(faces), nf, box.ctypes.data_as(C.c_void_p), nx, ny, nz, float(trunc), rule, _ptr(w), _ptr(s), _ptr(f),
                                  _ptr(stats), _ptr(ws), ws.numel(), _stream()))
    return w, s, f, stats


def _refuse_clipped(who, stats):
    n = int(stats[0])          # the one host synchronisation of a call with the caller's box
    if n:
        raise L.NrfError(f"{who}: {n} faces reach beyond the guard band of the lattice's columns (NRF_RASTER_GUARD steps from the box) and were left out: the winding "
                         "number is void.  Give a box around the mesh")


def WindingGrid(mesh, bbox=None, resolution=256):
    """nrf_mesh_voxelize, winding only: [nz, ny, nx] int32 on the lattice of DensityGrid over bbox (None: the mesh's padded bounds, see MeshToSDF): the number of
    +z-facing sheets above each lattice point minus the -z-facing ones.  1 inside an outward-oriented closed solid, 0 outside, -1 inside an inverted one, 2 inside two
    nested like-oriented shells, 0 in a cavity whose shell faces inward.  Exact for a closed mesh; an open mesh gives the count of its sheets above."""
    box, dims, _, own = _lattice("WindingGrid", mesh, bbox, resolution, None if bbox is None else 1.0)
    w, _, _, stats = _voxelize("WindingGrid", mesh, box, dims, 0.0, L.NRF_VOX_NONZERO, True, False, False)
    if own:
        _refuse_clipped("WindingGrid", stats)
    return w


@dataclass
class SDFVolume:
    """A mesh on the lattice of DensityGrid.  Outside is positive, the TSDF's convention."""
    sdf: torch.Tensor            # [nz, ny, nx] f32: -dist inside, +dist outside, |sdf| <= trunc
    winding: torch.Tensor        # [nz, ny, nx] int32
    face: torch.Tensor           # [nz, ny, nx] int32: the nearest face within trunc, -1 where none is
    bbox: np.ndarray             # [6] f32 on the host
    trunc: float
    stats: torch.Tensor          # [4] int32 on the device: faces clipped from the winding pass, with a bad index, with a non-finite vertex; 0
    rule: str = "nonzero"
    source: M.Mesh = None        # the mesh it was made from: Extract(attributes=True) reads its attributes

    def Field(self):
        """-sdf: inside positive, the convention of Isosurface.  An inside lattice point ON a face (an interior shell that the rule merged into the solid passes through
        it: distance 0) gets the smallest positive fp32 instead of 0, so that the rule, not the sign of a zero, says on which side of the level it lies."""
        tiny = torch.full((), float(np.finfo(np.float32).tiny), device=self.sdf.device)
        return torch.where(self.InsideMask() & (self.sdf == 0), tiny, -self.sdf)

    def InsideMask(self):
        """[nz, ny, nx] bool: the lattice points the rule calls inside"""
        return _INSIDE[RULES[self.rule]](self.winding)          # not sdf < 0: a lattice point ON the surface has sdf == -0

    def Inside(self, points):
        """[p] bool: the inside mask at the NEAREST lattice point of each of points [p, 3] (r = floorf(g + 0.5f), g = (pt - bmin) / step, as nrf_tsdf_observed rounds;
        clamped into the lattice; a non-finite point is outside).  Torch indexing, accurate only to the lattice's resolution: a point within half a step of the
        surface can be called either way.  An exact per-point winding query is not offered."""
        x = _dev_f32(points).reshape(-1, 3).to(self.sdf.device)
        nz, ny, nx = (int(v) for v in self.sdf.shape)
        b = torch.as_tensor(self.bbox, device=x.device)
        n = torch.tensor([nx, ny, nz], device=x.device)
        step = (b[3:] - b[:3]) / (n - 1).to(torch.float32)
        r = torch.floor((x - b[:3]) / step + 0.5)
        ok = torch.isfinite(x).all(dim=1)
        r = torch.where(ok[:, None], r, torch.zeros_like(r)).clamp(min=0).minimum((n - 1).to(torch.float32)).to(torch.int64)
        return self.InsideMask()[r[:, 2], r[:, 1], r[:, 0]] & ok

    def Extract(self, offset=0.0, keep_largest=None, min_component_faces=0, attributes=False):
        """Isosurface(Field(), bbox, -offset) -> FilterComponents if asked -> Mesh: the surface sdf == offset, |offset| < trunc.  Offset 0 is the closed remesh of the
        solid; a positive offset the dilated surface, a negative one the eroded.  Normals are the isosurface's lattice normals.  attributes=True: Colors, Normals and
        Relevancy of the source mesh, where it carries them, at the closest point ON it (ClosestOnMesh + InterpolateAttributes; normals re-normalised)."""
        offset = float(offset)
        if not abs(offset) < self.trunc:
            raise L.NrfError(f"SDFVolume.Extract: |offset| = {abs(offset):g} must stay below trunc = {self.trunc:g}: the distance is truncated there")
        verts, faces, normals = M.Isosurface(self.Field(), self.bbox, -offset)
        out = M.Mesh(verts, faces, normals)
        if keep_largest is not None or min_component_faces > 0:
            out = M.FilterComponents(out, keep_largest, min_component_faces)
        if attributes:
            from . import geometry as G
            if self.source is None:
                raise L.NrfError("SDFVolume.Extract: attributes=True needs the source mesh (SDFVolume.source)")
            names = [a for a in _TRANSFER if getattr(self.source, a) is not None]
            if names and out.Vertices.shape[0]:
                res = G.ClosestOnMesh(out.Vertices, self.source, points=False)
                new = {a: G.InterpolateAttributes(self.source, res, a) for a in names}
                if "Normals" in new:
                    new["Normals"] = M._safe_normalize(new["Normals"])
                out = dataclasses.replace(out, **new)
        return out


def MeshToSDF(mesh, bbox=None, resolution=256, trunc=None, rule="nonzero"):
    """nrf_mesh_voxelize -> SDFVolume.  resolution and bbox as DensityGrid's.  bbox=None: the mesh's bounds (one host synchronisation) padded by trunc plus one
    lattice step, so no face is clipped and the surface never touches the lattice's rim.  trunc=None: three of the largest lattice step.  rule: "nonzero" (nested
    like-oriented shells merge into one solid), "positive" (a reversed inner shell is a cavity, an inverted solid is empty) or "odd" (parity).  With a caller's box the
    count of faces clipped from the winding pass is read back (one host synchronisation) and a non-zero count raises, naming it."""
    r = _rule("MeshToSDF", rule)
    box, dims, t, own = _lattice("MeshToSDF", mesh, bbox, resolution, trunc)
    if not (np.isfinite(t) and t > 0.0):
        raise L.NrfError(f"MeshToSDF: trunc must be finite and > 0, got {trunc!r}")
    w, s, f, stats = _voxelize("MeshToSDF", mesh, box, dims, t, r, True, True, True)
    if own:
        _refuse_clipped("MeshToSDF", stats)
    return SDFVolume(s, w, f, box, float(np.float32(t)), stats, rule, mesh)


def RemeshUnion(mesh, resolution=256, rule="nonzero", **filters):
    """MeshToSDF(mesh, None, resolution, None, rule).Extract(**filters): a closed, uniformly sampled remesh of the solid the rule defines.  Under "nonzero" the
    interior shells of a density isosurface vanish into the solid around them without any camera; under "positive" a reversed inner shell stays as a cavity."""
    return MeshToSDF(mesh, None, resolution, None, rule).Extract(0.0, **filters)


def _inside(who, mesh, box, dims, rule):
    w = _voxelize(who, mesh, box, dims, 0.0, L.NRF_VOX_NONZERO, True, False, False)
    return _INSIDE[rule](w[0]), w[3]


def VoxelVolume(mesh, bbox=None, resolution=256, rule="nonzero"):
    """The volume of the solid as a float64 device scalar: the number of inside lattice points times the volume of a lattice cell (stepx * stepy * stepz).  Accurate
    to the lattice's resolution: the error is of the order of the surface area times one step."""
    r = _rule("VoxelVolume", rule)
    box, dims, _, own = _lattice("VoxelVolume", mesh, bbox, resolution, None if bbox is None else 1.0)
    inside, stats = _inside("VoxelVolume", mesh, box, dims, r)
    if own:
        _refuse_clipped("VoxelVolume", stats)
    cell = float(np.prod(_steps(box, dims).astype(np.float64)))
    return inside.sum().to(torch.float64) * cell


def VolumeIoU(mesh_a, mesh_b, bbox=None, resolution=256, rule="nonzero"):
    """Volumetric intersection over union of two meshes on ONE lattice -> (iou, n_intersection, n_union): iou a float64 device scalar (NaN where both solids are
    empty), the two counts int64 device scalars, exact.  bbox=None: the padded bounds of both meshes together (one host synchronisation); with a box the call
    synchronises nothing, and faces clipped from the winding pass are the caller's to avoid (MeshToSDF(...).stats[0] counts them)."""
    r = _rule("VolumeIoU", rule)
    if bbox is None:
        va, vb = (_dev_f32(m.Vertices).reshape(-1, 3) for m in (mesh_a, mesh_b))
        both = M.Mesh(torch.cat([va, vb.to(va.device)], dim=0), mesh_a.Faces, None)
        box, dims, _, _ = _lattice("VolumeIoU", both, None, resolution, None)
    else:
        box, dims, _, _ = _lattice("VolumeIoU", mesh_a, bbox, resolution, 1.0)
    ia, _ = _inside("VolumeIoU", mesh_a, box, dims, r)
    ib, _ = _inside("VolumeIoU", mesh_b, box, dims, r)
    n_i, n_u = (ia & ib).sum(), (ia | ib).sum()
    return n_i.to(torch.float64) / n_u.to(torch.float64), n_i, n_u
