"""Time the mesh voxeliser on one MI355X, on the meshes the library itself makes from the bench hash scene (make_hash_scene()): the TSDF mesh of --fuse-views orbit
views at --mesh-res, the density isosurface at the 0.7 quantile of the density (the noise-like worst case of DESIGN 8b) at --mesh-res, its visible part
(FilterVisible over a ring of --ring views) and the simplified versions of the TSDF mesh and of the visible part.  Per mesh and lattice (--res, over the scene's box):
  * nrf_mesh_voxelize, winding alone, then winding + distance + face at a truncation of 3 lattice steps: ms, faces per second;
  * a census in torch ops (fused kernels: not bit-exact, good for a census): the summed projected area of the faces in columns (the expected number of integer adds),
    the summed size of the dilated lattice boxes (the point-to-triangle tests, an upper bound of the 64-bit atomic mins) and the share of faces on each wide list;
    from them the atomics' added bytes per second, to set against the chip-wide atomic rate;
  * the same d2 from nrf_closest_on_mesh(max_dist = trunc) over all lattice points (--closest-res; meshes up to --closest-max-faces faces): the only route before
    this entry.  Its time, the time of building its FaceGrid, and whether face and d2 agree bit for bit with the voxeliser's wherever either finds one;
  * RemeshUnion at --union-res of the meshes named by --union: faces and components before and after, beside the visible part's face count.
Warm-up first, then device events and the median of the repeats.  One JSON line on stdout; every row also goes to stderr as soon as it is measured.
    python tools/voxel_bench.py [--meshes tsdf tsdf_simplified iso visible visible_simplified] [--mesh-res 512] [--res 256 512] [--closest-res 256 512]
                                [--union iso] [--union-res 512] [--repeats 5] [--warmup 1] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ATOMIC_GB_S = 1300.0          # the chip-wide rate of global atomic adds, in added bytes (measured for fp32 adds; the integer add and the 64-bit min are set against it)
FACE_CHUNK = 1 << 24
QUERY_CHUNK = 1 << 24
TRUNC_STEPS = 3.0


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), ms


def census(mesh, box, dims, trunc, wide_columns, wide_points):
    """The header's steps 1-3 and 7 up to the boxes in torch ops -> dict(columns: summed projected area in columns, box_points: summed lattice boxes, wide shares)"""
    dev = mesh.Vertices.device
    b = torch.as_tensor(box, device=dev)
    n = torch.tensor(dims, device=dev)
    step = (b[3:] - b[:3]) / (n - 1).to(torch.float32)
    g = (mesh.Vertices - b[:3]) / step
    XY = torch.round(g[:, :2] * 256.0).to(torch.int64)
    top = (n - 1).to(torch.float32)
    out = dict(columns=0.0, box_points=0, wide_column_faces=0, wide_point_faces=0)
    for i in range(0, mesh.Faces.shape[0], FACE_CHUNK):
        f = mesh.Faces[i:i + FACE_CHUNK].to(torch.int64)
        x, y = XY[f][..., 0], XY[f][..., 1]
        A = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
        out["columns"] += float(A.abs().to(torch.float64).sum()) / (2.0 * 256.0 * 256.0)
        i0, i1 = ((x.amin(-1) + 255) >> 8).clamp_min(0), (x.amax(-1) >> 8).clamp_max(dims[0] - 1)
        j0, j1 = ((y.amin(-1) + 255) >> 8).clamp_min(0), (y.amax(-1) >> 8).clamp_max(dims[1] - 1)
        out["wide_column_faces"] += int(((A != 0) & ((i1 - i0 + 1).clamp_min(0) * (j1 - j0 + 1).clamp_min(0) > wide_columns)).sum())
        tri = mesh.Vertices[f]
        fl = (torch.floor((tri.amin(1) - trunc - b[:3]) / step) - 1.0)
        fh = (torch.ceil((tri.amax(1) + trunc - b[:3]) / step) + 1.0)
        some = ((fh >= 0) & (fl <= top)).all(-1)
        pts = ((torch.minimum(fh, top) - fl.clamp_min(0) + 1.0).clamp_min(0).to(torch.int64).prod(-1)) * some
        out["box_points"] += int(pts.sum())
        out["wide_point_faces"] += int((pts > wide_points).sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", nargs="+", default=["tsdf", "tsdf_simplified", "iso", "visible", "visible_simplified"])
    ap.add_argument("--mesh-res", type=int, default=512)
    ap.add_argument("--fuse-views", type=int, default=32)
    ap.add_argument("--hw", type=int, default=800)
    ap.add_argument("--ring", type=int, default=32)
    ap.add_argument("--simplify-faces", type=int, default=200000)
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--closest-res", type=int, nargs="*", default=[256, 512])
    ap.add_argument("--closest-max-faces", type=int, default=20000000)
    ap.add_argument("--union", nargs="*", default=["iso"])
    ap.add_argument("--union-res", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from nerfpp_amd import _lib as L, geometry as G, mesh as M, raster as R, scene as S, tsdf as T, voxel as V
    torch.cuda.set_device(0)
    sc = S.make_hash_scene()
    r = sc["renderer"]
    rp = S.lego_render_params(sc["bbox"])
    K = S.lego_K(a.hw, a.hw)
    box = M._bbox(r, None)
    out = dict(repeats=a.repeats, warmup=a.warmup, mesh_res=a.mesh_res, bbox=box.tolist(), trunc_steps=TRUNC_STEPS, atomic_gb_per_s=ATOMIC_GB_S,
               wide=(V.WIDE_COLUMNS, V.WIDE_POINTS), lib=os.path.relpath(os.environ["NRF_LIB_PATH"]) if os.environ.get("NRF_LIB_PATH") else "default")

    def emit(name, row):
        out[name] = row
        print(json.dumps({name: row}), file=sys.stderr, flush=True)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(json.dumps(out) + "\n")

    made = {}

    def make(name):
        if name in made:
            return made[name]
        if name == "tsdf":
            m = T.ExtractMeshTSDF(r, T.OrbitViews(a.fuse_views, a.hw, a.hw, K, 4.0), rp, resolution=a.mesh_res)
        elif name == "iso":
            sigma = M.DensityGrid(r, None, a.mesh_res)
            iso = float(torch.quantile(sigma.reshape(-1)[::97].float(), 0.7))
            del sigma
            m = M.ExtractMesh(r, iso, resolution=a.mesh_res, colors=False)
        elif name == "visible":
            m = R.FilterVisible(make("iso"), T.OrbitViews(a.ring, a.hw, a.hw, K, 4.0))
        else:
            m = M.SimplifyToFaces(make(name[:-len("_simplified")]), a.simplify_faces)[0]
        made[name] = m
        torch.cuda.empty_cache()
        return m

    for name in a.meshes:
        m = make(name)
        nv, nf = int(m.Vertices.shape[0]), int(m.Faces.shape[0])
        row = dict(verts=nv, faces=nf)
        for res in a.res:
            dims = (res, res, res)
            trunc = TRUNC_STEPS * float(V._steps(box, dims).max())
            at = dict(trunc=trunc)
            at.update(census(m, box, dims, trunc, V.WIDE_COLUMNS, V.WIDE_POINTS))
            at["winding_ms"], at["winding_all_ms"] = timed(lambda: V._voxelize("bench", m, box, dims, 0.0, L.NRF_VOX_NONZERO, True, False, False), a.warmup, a.repeats)
            at["full_ms"], at["full_all_ms"] = timed(lambda: V._voxelize("bench", m, box, dims, trunc, L.NRF_VOX_NONZERO, True, True, True), a.warmup, a.repeats)
            at["winding_faces_per_s"], at["full_faces_per_s"] = nf / at["winding_ms"] * 1e3, nf / at["full_ms"] * 1e3
            at["winding_atomic_gb_per_s"] = 4.0 * at["columns"] / at["winding_ms"] * 1e-6
            at["full_atomic_gb_per_s_upper"] = (4.0 * at["columns"] + 8.0 * at["box_points"]) / at["full_ms"] * 1e-6
            w, s, f, stats = V._voxelize("bench", m, box, dims, trunc, L.NRF_VOX_NONZERO, True, True, True)
            at["stats"] = stats.cpu().tolist()
            at["inside_points"], at["found_points"] = int((w != 0).sum()), int((f >= 0).sum())
            del w
            if res in a.closest_res and nf <= a.closest_max_faces:
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                grid = G.FaceGrid(m, bbox=box)
                e1.record()
                e1.synchronize()
                at["face_grid_build_ms"] = e0.elapsed_time(e1)
                n_pts = res ** 3
                d2 = torch.empty((n_pts,), device=s.device, dtype=torch.float32)
                face = torch.empty((n_pts,), device=s.device, dtype=torch.int32)

                def gather():
                    for q0 in range(0, n_pts, QUERY_CHUNK):
                        idx = torch.arange(q0, min(q0 + QUERY_CHUNK, n_pts), device=s.device)
                        res_ = G.ClosestOnMesh(M._lattice_points_at(box, res, res, res, idx), grid, max_dist=trunc, uv=False, points=False)
                        d2[q0:q0 + idx.numel()], face[q0:q0 + idx.numel()] = res_.Dist2, res_.Face
                at["closest_ms"], at["closest_all_ms"] = timed(gather, 0, 1)
                at["closest_over_full"] = at["closest_ms"] / at["full_ms"]
                dist = torch.where(face >= 0, torch.sqrt(d2), torch.full_like(d2, trunc)).clamp_max(trunc)
                at["faces_agree"] = bool((face == f.reshape(-1)).all())
                at["d2_agree"] = bool((dist.view(torch.int32) == s.abs().reshape(-1).view(torch.int32)).all())
                del grid, d2, face, dist
            del s, f
            torch.cuda.empty_cache()
            row[f"res{res}"] = at
        if name in a.union:
            comps = M.MeshComponents(m)[1]
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            u = V.RemeshUnion(m, resolution=a.union_res)
            e1.record()
            e1.synchronize()
            row["union"] = dict(resolution=a.union_res, ms=e0.elapsed_time(e1), faces_before=nf, faces_after=int(u.Faces.shape[0]), components_before=comps,
                                components_after=M.MeshComponents(u)[1], closed=bool(M.MeshTopology(u)["closed"]))
            del u
        emit(name, row)
        del m
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
