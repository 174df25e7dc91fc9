"""Time mesh simplification on one MI355X, on the two meshes the library itself makes from the bench hash scene (make_hash_scene()) and DESIGN 8k / 8l compare: the
TSDF mesh of --fuse-views orbit views at --res, and the density isosurface at the 0.7 quantile of the density at --res thinned by FilterVisible over a ring of --ring
views (coloured afterwards, as ExtractMesh colours a mesh); with --raw also the whole isosurface before that filter (timings and face counts only).
Per mesh and per cell size of --factors times the extraction step (bmax - bmin) / (res - 1):
  * nrf_mesh_simplify_count (its synchronisation included) and nrf_mesh_simplify_emit with every output, each against a floor of bytes moved at the streaming rate
    DESIGN 8j measured (3.2 TB/s): count reads 12 B per vertex and 12 B per face and writes and reads 4 B per cell; emit reads the vertices and the per-face triples again
    (12 B each) and the cells (4 B), and writes 12 B per output vertex and per output face;
  * the grid, the workspace bytes, the vertices and faces left, d_stats;
  * SurfaceDistance of the result against the input (--points samples of each), and EvaluateMesh over --eval-views views before and after;
  * the same clustering composed from torch ops on the same GPU: cells by floor, torch.unique over the sorted cell triples, index_add for the net orientation and for
    the means, scatter_reduce for the lowest face of each parity (the same faces survive; the means are fp32 sums, not the library's bits).
A call above 50 ms is repeated 3 times, not --repeats.  --profile-loop N: build the TSDF mesh only and run count + emit N times at the middle factor, for a kernel
trace by an outside profiler (nothing is timed).  Warm-up first, then device events and the median of the repeats.  One JSON line on stdout.
    python tools/simplify_bench.py [--res 512] [--factors 2 4 8] [--points 1000000] [--eval-views 4] [--raw] [--repeats 9] [--warmup 2] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.geometry_bench import floor_ms, timed, timed_auto, STREAM_GB_S          # noqa: E402


def torch_clustering(verts, faces, box, dims):
    """The clustering from torch ops -> (positions [V', 3], faces [F', 3] int64 output ids, kept input faces [F'])"""
    dev = verts.device
    lo = torch.as_tensor(box[:3], device=dev)
    n = torch.as_tensor(np.asarray(dims, np.float32), device=dev)
    inv = n / (torch.as_tensor(box[3:], device=dev) - lo)
    c = torch.floor((verts - lo) * inv).clamp_min(0).minimum(n - 1).to(torch.int64)
    cell = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    tri = cell[faces.to(torch.int64)]
    cand = torch.nonzero((tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])).reshape(-1)
    used = torch.zeros((verts.shape[0],), dtype=torch.bool, device=dev)
    used[faces.to(torch.int64).reshape(-1)] = True
    t = tri[cand]
    s = torch.sort(t, dim=1).values
    even = ((t == s).all(1)) | ((t == s.roll(-1, 1)).all(1)) | ((t == s.roll(-2, 1)).all(1))
    _, group = torch.unique(s, dim=0, return_inverse=True)
    k = int(group.max()) + 1 if group.numel() else 0
    net = torch.zeros((k,), dtype=torch.int64, device=dev).index_add_(0, group, torch.where(even, 1, -1))
    big = torch.iinfo(torch.int64).max
    low_even = torch.full((k,), big, dtype=torch.int64, device=dev).scatter_reduce_(0, group[even], cand[even], "amin")
    low_odd = torch.full((k,), big, dtype=torch.int64, device=dev).scatter_reduce_(0, group[~even], cand[~even], "amin")
    winner = torch.where(net > 0, low_even, torch.where(net < 0, low_odd, torch.full_like(net, big)))
    kept = torch.sort(winner[winner != big]).values
    out_cells, out_faces = torch.unique(tri[kept], return_inverse=True)
    member = torch.nonzero(used).reshape(-1)
    at = torch.searchsorted(out_cells, cell[member]).clamp_max(max(out_cells.numel() - 1, 0))
    hit = out_cells[at] == cell[member] if out_cells.numel() else torch.zeros_like(at, dtype=torch.bool)
    member, at = member[hit], at[hit]
    pos = torch.zeros((out_cells.numel(), 3), device=dev).index_add_(0, at, verts[member])
    cnt = torch.zeros((out_cells.numel(),), device=dev).index_add_(0, at, torch.ones_like(at, dtype=torch.float32))
    return pos / cnt[:, None], out_faces, kept


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--factors", type=float, nargs="+", default=[2.0, 4.0, 8.0])
    ap.add_argument("--fuse-views", type=int, default=32)
    ap.add_argument("--ring", type=int, default=32)
    ap.add_argument("--hw", type=int, default=800)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--eval-views", type=int, default=4)
    ap.add_argument("--raw", action="store_true", help="also the whole isosurface before FilterVisible (timings and counts only)")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--profile-loop", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from nerfpp_amd import _lib as L, geometry as G, mesh as M, raster as R, scene as S, tsdf as T
    from nerfpp_amd.modules import _ptr, _stream
    torch.cuda.set_device(0)
    sc = S.make_hash_scene()
    r = sc["renderer"]
    rp = S.lego_render_params(sc["bbox"])
    K = S.lego_K(a.hw, a.hw)
    box = np.asarray(sc["bbox"], np.float32).reshape(6)
    step = float((box[3:] - box[:3]).max()) / (a.res - 1)
    lib = L.lib()
    t0 = time.time()
    tsdf_mesh = T.ExtractMeshTSDF(r, T.OrbitViews(a.fuse_views, a.hw, a.hw, K, 4.0), rp, resolution=a.res)

    def measure(name, m, quality):
        s = M._Simplifier(m)
        dev = s.verts.device
        rows = {}
        for factor in a.factors:
            cell = factor * step
            gbox, dims = M._simplify_grid(s.verts, cell, None, None)
            cells = dims[0] * dims[1] * dims[2]
            nv, nf = s.count(gbox, dims)
            stats = s.stats.cpu().tolist()
            ws_bytes = int(lib.nrf_mesh_simplify_workspace_bytes(s.nv, s.nf, *dims))
            outs = [torch.empty((nv, 3), device=dev), torch.empty((nf, 3), device=dev, dtype=torch.int32), torch.empty((nv,), device=dev, dtype=torch.int32),
                    torch.empty((nf,), device=dev, dtype=torch.int32), torch.empty((s.nv,), device=dev, dtype=torch.int32)]

            def emit():
                L.check(lib.nrf_mesh_simplify_emit(_ptr(s.verts), s.nv, _ptr(s.faces), s.nf, gbox.ctypes.data_as(C.c_void_p), *dims, 0, nv, nf, *[_ptr(o) for o in outs],
                                                   _ptr(s.ws), s.ws.numel(), _stream()))
            count_ms = timed_auto(lambda: s.count(gbox, dims), a.warmup, a.repeats)
            emit_ms = timed_auto(emit, a.warmup, a.repeats)
            cf = floor_ms(12 * s.nv + 12 * s.nf + 8 * cells)
            ef = floor_ms(12 * s.nv + 12 * s.nf + 4 * cells + 12 * nv + 12 * nf)
            row = dict(cell=cell, dims=list(dims), cells=cells, workspace_bytes=ws_bytes, out_verts=nv, out_faces=nf, stats=stats, count_ms=count_ms, count_floor_ms=cf,
                       count_over_floor=count_ms / cf, emit_ms=emit_ms, emit_floor_ms=ef, emit_over_floor=emit_ms / ef)
            if quality:
                small = M.SimplifyMesh(m, cell_size=cell)
                sd = G.SurfaceDistance(small, m, taus=(0.5 * cell, cell), n_points=a.points, bbox=box)
                row["surface_distance"] = {k: getattr(sd, k).cpu().tolist() for k in ("Accuracy", "Completeness", "Chamfer", "Hausdorff", "Precision", "Recall", "FScore")}
                row["surface_distance"]["taus"] = [0.5 * cell, cell]
                if m.Colors is not None and a.eval_views > 0:
                    ev = R.EvaluateMesh(small, r, T.OrbitViews(a.eval_views, a.hw, a.hw, K, 4.0), rp)
                    row["evaluate_mesh"] = {k: float(ev["mean_" + k]) for k in ("psnr", "ssim", "depth_error", "iou")}
                del small
                if not a.no_torch:
                    fin = torch.isfinite(s.verts).all(1).all()
                    pos, tf, kept = torch_clustering(s.verts, s.faces, gbox, dims)
                    row["torch_ops"] = dict(ms=timed_auto(lambda: torch_clustering(s.verts, s.faces, gbox, dims), 1, 3), out_verts=int(pos.shape[0]), out_faces=int(tf.shape[0]),
                                            same_faces=bool(fin) and bool(torch.equal(kept.to(torch.int32), outs[3])) and bool(torch.equal(tf.to(torch.int32), outs[1])),
                                            max_position_difference=float((pos - outs[0]).abs().max()) if pos.shape == outs[0].shape and nv else None)
                    del pos, tf, kept
            rows[f"x{factor:g}"] = row
            print(json.dumps({name: {f"x{factor:g}": row}}), file=sys.stderr, flush=True)
            del outs
            torch.cuda.empty_cache()
        return rows

    if a.profile_loop:
        s = M._Simplifier(tsdf_mesh)
        gbox, dims = M._simplify_grid(s.verts, a.factors[len(a.factors) // 2] * step, None, None)
        for _ in range(a.profile_loop):
            s.count(gbox, dims)
            s.emit(0)
        torch.cuda.synchronize()
        print(json.dumps(dict(profile_loop=a.profile_loop, dims=list(dims), verts=s.nv, faces=s.nf, out=list(s.out))))
        return
    sigma = M.DensityGrid(r, None, a.res)
    iso = float(torch.quantile(sigma.reshape(-1)[::97].float(), 0.7))
    del sigma
    full = M.ExtractMesh(r, iso, resolution=a.res, colors=False)
    n_full = [int(full.Vertices.shape[0]), int(full.Faces.shape[0])]
    iso_mesh = R.FilterVisible(full, T.OrbitViews(a.ring, a.hw, a.hw, K, 4.0))
    build_s = time.time() - t0
    out = dict(repeats=a.repeats, warmup=a.warmup, res=a.res, step=step, stream_gb_per_s=STREAM_GB_S, mesh_build_s=build_s, bbox=box.tolist(), points=a.points,
               meshes=dict(tsdf=[int(tsdf_mesh.Vertices.shape[0]), int(tsdf_mesh.Faces.shape[0])], iso_visible=[int(iso_mesh.Vertices.shape[0]), int(iso_mesh.Faces.shape[0])],
                           iso_full=n_full))
    if a.raw:
        torch.cuda.empty_cache()
        out["iso_full"] = measure("iso_full", full, False)
    del full
    torch.cuda.empty_cache()
    rgb = torch.empty_like(iso_mesh.Vertices)          # ExtractMesh's colours, for the vertices FilterVisible kept
    for i in range(0, rgb.shape[0], M.COLOR_CHUNK):
        raw = r.RunNetwork(iso_mesh.Vertices[i:i + M.COLOR_CHUNK][:, None, :], (-iso_mesh.Normals[i:i + M.COLOR_CHUNK]).contiguous(), L.NRF_PREC_F32)
        rgb[i:i + M.COLOR_CHUNK] = torch.sigmoid(raw[:, 0, :3])
    iso_mesh.Colors = rgb
    for name, m in (("tsdf", tsdf_mesh), ("iso_visible", iso_mesh)):
        if m.Colors is not None and a.eval_views > 0:
            ev = R.EvaluateMesh(m, r, T.OrbitViews(a.eval_views, a.hw, a.hw, K, 4.0), rp)
            out[name + "_input_evaluate_mesh"] = {k: float(ev["mean_" + k]) for k in ("psnr", "ssim", "depth_error", "iou")}
        out[name] = measure(name, m, True)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
