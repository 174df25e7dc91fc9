"""Time the geometry entries on one MI355X, on the two meshes the library itself makes from the bench hash scene (make_hash_scene()) and DESIGN 8k compares: the TSDF
mesh of --fuse-views orbit views at --res, and the density isosurface at the 0.7 quantile of the density at --res thinned by FilterVisible over a ring of --ring views.
Per sample size of --points:
  * surface sampling of both meshes: nrf_mesh_sample_count (its synchronisation included) and nrf_mesh_sample_emit, each against its byte floor;
  * nrf_nearest_points from the TSDF samples to the isosurface samples on the default grid (GridDims at --occupancy, the first value the default): the grid build (a
    call with ONE query), the whole call, the query as the difference of the two, and the share of the queries the brute-force fallback served, from d_stats;
  * the same call at every other --occupancy, and -- with the emit of the isosurface's samples -- through every --ring-lib (tuning builds of geometry.hip: another
    NRF_NN_MAX_RINGS, or -DNRF_SAMPLE_EMIT_BY_FACE for one lane per face); a call above 50 ms is repeated 3 times, not --repeats;
  * nrf_distance_stats, and SurfaceDistance of the two point sets (both directions, two statistics);
  * the same nearest neighbours from torch ops: torch.cdist of --cdist-queries queries against all targets in chunks of --cdist-chunk, SCALED by nq / cdist-queries
    (the whole problem does not fit: nq x nt floats), agreement of the indices checked on those queries;
  * scipy's cKDTree on the host (build and query with 16 workers) where scipy is importable and the size is at most --kdtree-max.
Byte floors at the streaming rate DESIGN 8j measured (3.2 TB/s): count 12 B of indices + 36 B of corners + 8 B written per face; emit 12 + 4 + 8 B written and 12 + 36 B
gathered per point; build 2 x 12 B read + 16 B written per target + 16 B per cell (memset, count scan in and out, cursors); query 12 B read + 8 B written per query +
16 B per target + 4 B per cell; statistics 4 B per entry.  Warm-up first, then device events and the median of the repeats.  One JSON line on stdout.
    python tools/geometry_bench.py [--points 1000000 10000000] [--res 512] [--occupancy 8 2 4 16 32] [--ring-lib PATH ...] [--repeats 9] [--warmup 2] [--out FILE]
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

STREAM_GB_S = 3200.0


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
    return float(np.median(ms))


def timed_auto(fn, warmup, repeats):
    """timed(), but a call that takes more than 50 ms is repeated 3 times after the one run that found that out"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return timed(fn, 0, 3) if a.elapsed_time(b) > 50.0 else timed(fn, warmup, repeats)


def floor_ms(nbytes):
    return nbytes / STREAM_GB_S * 1e-6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[1000000, 10000000])
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--fuse-views", type=int, default=32)
    ap.add_argument("--ring", type=int, default=32)
    ap.add_argument("--hw", type=int, default=800)
    ap.add_argument("--occupancy", type=float, nargs="+", default=[8.0, 2.0, 4.0, 16.0, 32.0])
    ap.add_argument("--ring-lib", nargs="*", default=[], help="libnerfpp_hip.so of tuning builds (make OUT=... EXTRA=-DNRF_NN_MAX_RINGS=n)")
    ap.add_argument("--cdist-queries", type=int, default=4096)
    ap.add_argument("--cdist-chunk", type=int, default=1 << 18)
    ap.add_argument("--kdtree-max", type=int, default=1000000)
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
    t0 = time.time()
    tsdf_mesh = T.ExtractMeshTSDF(r, T.OrbitViews(a.fuse_views, a.hw, a.hw, K, 4.0), rp, resolution=a.res)
    sigma = M.DensityGrid(r, None, a.res)
    iso = float(torch.quantile(sigma.reshape(-1)[::97].float(), 0.7))
    del sigma
    full = M.ExtractMesh(r, iso, resolution=a.res, colors=False)
    n_full = int(full.Faces.shape[0])
    iso_mesh = R.FilterVisible(full, T.OrbitViews(a.ring, a.hw, a.hw, K, 4.0))
    del full
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    out = dict(repeats=a.repeats, warmup=a.warmup, res=a.res, stream_gb_per_s=STREAM_GB_S, mesh_build_s=time.time() - t0, bbox=box.tolist(),
               meshes=dict(tsdf=[int(tsdf_mesh.Vertices.shape[0]), int(tsdf_mesh.Faces.shape[0])], iso_visible=[int(iso_mesh.Vertices.shape[0]), int(iso_mesh.Faces.shape[0])],
                           iso_full_faces=n_full), max_rings=G.NN_MAX_RINGS)
    lib = L.lib()
    dev = tsdf_mesh.Vertices.device

    def ring_lib(path):
        other = C.CDLL(path)
        for name in ("nrf_nearest_points", "nrf_nearest_points_workspace_bytes", "nrf_mesh_sample_emit"):
            ret, args = L.SIGNATURES[name]
            getattr(other, name).restype = L._KINDS[ret]
            getattr(other, name).argtypes = [L._KINDS[k] for k in args]
        return other

    def nearest(q, t, dims, stats=None, use=lib):
        nq, nt = int(q.shape[0]), int(t.shape[0])
        d2 = torch.empty((nq,), device=dev, dtype=torch.float32)
        idx = torch.empty((nq,), device=dev, dtype=torch.int32)
        ws = torch.empty((int(use.nrf_nearest_points_workspace_bytes(nq, nt, *dims)),), device=dev, dtype=torch.uint8)

        def call():
            L.check(use.nrf_nearest_points(_ptr(q), nq, _ptr(t), nt, box.ctypes.data_as(C.c_void_p), *dims, float("inf"), _ptr(d2), _ptr(idx), _ptr(stats), _ptr(ws), ws.numel(),
                                           _stream()))
        return call, d2, idx

    for n in a.points:
        row = {}
        samples = {}
        for name, m in (("tsdf", tsdf_mesh), ("iso_visible", iso_mesh)):
            verts, faces = G._mesh_arrays(m)
            nv, nf = int(verts.shape[0]), int(faces.shape[0])
            ws = G._workspace(lib.nrf_mesh_sample_workspace_bytes(nv, nf), dev)
            _, area = G._count(verts, faces, 0.0, 0, None, ws)
            density = n / area
            got, _ = G._count(verts, faces, density, 0, None, ws)
            pts = torch.empty((got, 3), device=dev, dtype=torch.float32)
            face = torch.empty((got,), device=dev, dtype=torch.int32)
            uv = torch.empty((got, 2), device=dev, dtype=torch.float32)
            count_ms = timed(lambda: G._count(verts, faces, density, 0, None, ws), a.warmup, a.repeats)
            emit_ms = timed(lambda: L.check(lib.nrf_mesh_sample_emit(_ptr(verts), nv, _ptr(faces), nf, 0, got, _ptr(pts), _ptr(face), _ptr(uv), _ptr(ws), ws.numel(), _stream())),
                            a.warmup, a.repeats)
            stats = G.SampleSurface(m, density=density, seed=0).Stats.cpu().tolist()
            cf, ef = floor_ms(56 * nf), floor_ms(72 * got)
            row["sample_" + name] = dict(area=area, points=got, stats=stats, count_ms=count_ms, count_floor_ms=cf, count_over_floor=count_ms / cf, emit_ms=emit_ms,
                                         emit_floor_ms=ef, emit_over_floor=emit_ms / ef)
            samples[name] = pts
            del ws, face, uv
        q, t = samples["tsdf"], samples["iso_visible"]
        nq, nt = int(q.shape[0]), int(t.shape[0])
        d2 = idx = None
        libs = [("default", lib)] + [(os.path.basename(os.path.dirname(os.path.abspath(path))), ring_lib(path)) for path in a.ring_lib]
        for occ in a.occupancy:
            dims = G.GridDims(box, nt, occ)
            cells = dims[0] * dims[1] * dims[2]
            occupied = int((torch.unique(_cells_of(t, box, dims)).numel()))
            for lib_name, use in libs:
                st = torch.zeros((3,), device=dev, dtype=torch.int32)
                whole, d2o, idxo = nearest(q, t, dims, use=use)
                counted, _, _ = nearest(q, t, dims, st, use=use)
                counted()
                whole_ms = timed_auto(whole, a.warmup, a.repeats)
                if d2 is None:
                    d2, idx = d2o, idxo
                entry = dict(dims=list(dims), cells=cells, occupied_cells=occupied, targets_per_occupied_cell=nt / max(occupied, 1), whole_ms=whole_ms,
                             fallback_queries=int(st[2]), fallback_share=int(st[2]) / max(nq, 1), same_bits=bool(torch.equal(d2o, d2) and torch.equal(idxo, idx)))
                if lib_name == "default":
                    build, _, _ = nearest(q[:1], t, dims)
                    build_ms = timed_auto(build, a.warmup, a.repeats)
                    bf, qf = floor_ms(40 * nt + 16 * cells), floor_ms(20 * nq + 16 * nt + 4 * cells)
                    entry.update(build_ms=build_ms, build_floor_ms=bf, build_over_floor=build_ms / bf, query_ms=whole_ms - build_ms, query_floor_ms=qf,
                                 query_over_floor=(whole_ms - build_ms) / qf, queries_per_s=nq / max(whole_ms - build_ms, 1e-9) * 1e3)
                row[f"nearest_occ{occ:g}_{lib_name}"] = entry
                print(json.dumps({n: {f"nearest_occ{occ:g}_{lib_name}": entry}}), file=sys.stderr, flush=True)
        # two samplings of ONE surface (another seed): the case of a mesh close to its ground truth, where a fine grid pays
        q_same = G.SampleSurface(iso_mesh, density=n / row["sample_iso_visible"]["area"], seed=1).Points
        for occ in a.occupancy:
            dims = G.GridDims(box, nt, occ)
            st = torch.zeros((3,), device=dev, dtype=torch.int32)
            counted, _, _ = nearest(q_same, t, dims, st)
            counted()
            whole, _, _ = nearest(q_same, t, dims)
            entry = dict(dims=list(dims), queries=int(q_same.shape[0]), whole_ms=timed_auto(whole, a.warmup, a.repeats), fallback_queries=int(st[2]))
            row[f"nearest_same_surface_occ{occ:g}"] = entry
            print(json.dumps({n: {f"nearest_same_surface_occ{occ:g}": entry}}), file=sys.stderr, flush=True)
        del q_same
        # the emit of the isosurface's samples through every library (a build with -DNRF_SAMPLE_EMIT_BY_FACE serves one lane per face)
        verts, faces = G._mesh_arrays(iso_mesh)
        nv, nf = int(verts.shape[0]), int(faces.shape[0])
        ews = G._workspace(lib.nrf_mesh_sample_workspace_bytes(nv, nf), dev)
        got, _ = G._count(verts, faces, n / row["sample_iso_visible"]["area"], 0, None, ews)
        pts, pts_alt = torch.empty((got, 3), device=dev), torch.empty((got, 3), device=dev)
        emit = lambda use, o: L.check(use.nrf_mesh_sample_emit(_ptr(verts), nv, _ptr(faces), nf, 0, got, _ptr(o), None, None, _ptr(ews), ews.numel(), _stream()))
        emit(lib, pts)
        for lib_name, use in libs:
            emit_ms = timed(lambda: emit(use, pts_alt), a.warmup, a.repeats)
            row["emit_points_only_" + lib_name] = dict(ms=emit_ms, same_bits=bool(torch.equal(pts.view(torch.int32), pts_alt.view(torch.int32))))
        del ews, pts, pts_alt
        print(json.dumps({n: "nearest done"}), file=sys.stderr, flush=True)
        sws = G._workspace(lib.nrf_distance_stats_workspace_bytes(nq), dev)
        sout = torch.empty((7,), device=dev, dtype=torch.float64)
        taus = np.array([0.005, 0.01, 0.02], np.float32)
        stats_ms = timed(lambda: L.check(lib.nrf_distance_stats(_ptr(d2), nq, taus.ctypes.data_as(C.c_void_p), 3, _ptr(sout), _ptr(sws), sws.numel(), _stream())), a.warmup, a.repeats)
        row["stats"] = dict(ms=stats_ms, floor_ms=floor_ms(4 * nq), over_floor=stats_ms / floor_ms(4 * nq), values=sout.cpu().tolist())
        row["surface_distance_ms"] = timed_auto(lambda: G.SurfaceDistance(q, t, taus=tuple(taus.tolist()), bbox=box), 1, max(3, a.repeats // 3))
        sd = G.SurfaceDistance(q, t, taus=tuple(taus.tolist()), bbox=box)
        row["surface_distance"] = {k: getattr(sd, k).cpu().tolist() for k in ("Accuracy", "Completeness", "Chamfer", "ChamferSq", "Hausdorff", "Precision", "Recall", "FScore")}
        # torch ops: cdist over chunks of the targets, a running minimum
        qs = q[:a.cdist_queries].contiguous()

        def by_cdist():
            best = torch.full((qs.shape[0],), float("inf"), device=dev)
            arg = torch.zeros((qs.shape[0],), device=dev, dtype=torch.int64)
            for c0 in range(0, nt, a.cdist_chunk):
                d, j = torch.cdist(qs, t[c0:c0 + a.cdist_chunk]).min(dim=1)
                better = d < best
                best = torch.where(better, d, best)
                arg = torch.where(better, j + c0, arg)
            return best, arg
        cd_ms = timed(by_cdist, 1, 3)
        _, arg = by_cdist()
        row["torch_cdist"] = dict(queries=int(qs.shape[0]), chunk=a.cdist_chunk, ms=cd_ms, scaled_to_all_queries_ms=cd_ms * nq / max(int(qs.shape[0]), 1), scaled=True,
                                  index_agreement=float((arg.to(torch.int32) == idx[:qs.shape[0]]).float().mean()))
        try:
            from scipy.spatial import cKDTree
            if max(nq, nt) <= a.kdtree_max * 1.1:
                tc, qc = t.cpu().numpy(), q.cpu().numpy()
                t1 = time.time()
                tree = cKDTree(tc)
                t2 = time.time()
                _, j = tree.query(qc, workers=16)
                t3 = time.time()
                row["scipy_ckdtree"] = dict(build_s=t2 - t1, query_s=t3 - t2, workers=16, index_agreement=float((j == idx.cpu().numpy()).mean()))
            else:
                row["scipy_ckdtree"] = "not measured at this size"
        except ImportError:
            row["scipy_ckdtree"] = "scipy is not importable"
        out[str(n)] = row
        print(json.dumps({n: row}), file=sys.stderr, flush=True)
        del samples, q, t, d2, idx
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


def _cells_of(points, box, dims):
    """The linear cell of every point in torch ops (a census, not the kernel's bits)"""
    lo = torch.as_tensor(box[:3], device=points.device)
    inv = torch.as_tensor(np.asarray(dims, np.float32) / (box[3:] - box[:3]), device=points.device)
    c = torch.floor((points - lo) * inv).clamp_min(0).minimum(torch.as_tensor(np.asarray(dims, np.float32) - 1, device=points.device)).to(torch.int64)
    return (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]


if __name__ == "__main__":
    main()
