"""Time the point-cloud tools on one MI355X, in one process on the same inputs: surface samples of the bench scene's two meshes (the TSDF mesh of --fuse-views
orbit views and the visible density isosurface at --res, as tools/bvh_bench.py builds them).  Every yardstick is a path the library had before the point tools:
  * build: PointBVH(points) beside MeshBVH on the equivalent faces (i, i, i) -- the same kernels, a face array more -- and beside nothing for the grid (it is built
    inside every nrf_nearest_points call); the bytes of the buffer and the workspace;
  * nearest: k = 1 of --points samples of one mesh against as many of the other, NearestPoints over the grid (box given: no synchronisation) against
    NearestPoints over the PointBVH, plain and coherent; the same with --far-points queries pushed 10 and 1000 box diagonals away (the grid's brute-force fallback);
  * knn: k = 8 / 16 / 32 of --knn-points samples against a chunked torch.cdist + topk at that size (distances only compared as values: cdist forms d another way);
  * normals / scores: EstimateNormals(k = 16) and StatisticalOutliers(k = 16) at the first --points size, split into their kNN and the rest;
  * icp: one iteration's query and sums against a cloud, point mode through the grid beside plane mode through the PointBVH and given normals.
Outputs of the two sides of a row are compared as bytes.  Warm-up first, then device events and the median of the repeats; a call above 50 ms is repeated 3 times;
the first call is reported apart.  One JSON line on stdout.
    python tools/points_bench.py [--points 1000000 10000000] [--res 512] [--out profiles/points/points_bench.json]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed_auto(fn, warmup, repeats):
    """(first call ms, median ms of the later calls): a call above 50 ms is repeated 3 times, not `repeats`, and needs no further warm-up"""
    first = event_ms(fn)
    if first <= 50.0:
        for _ in range(warmup):
            fn()
    return first, float(np.median([event_ms(fn) for _ in range(3 if first > 50.0 else repeats)]))


def same_bytes(a, b):
    return bool(torch.equal(a.contiguous().view(torch.uint8).reshape(-1), b.contiguous().view(torch.uint8).reshape(-1)))          # KNearest's [n, 1] beside NearestPoints' [n]


def cdist_topk(q, t, k, chunk):
    d, i = [], []
    for s in range(0, q.shape[0], chunk):
        dd, ii = torch.cdist(q[s:s + chunk], t).topk(k, dim=1, largest=False)
        d.append(dd)
        i.append(ii)
    return torch.cat(d), torch.cat(i)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[1000000, 10000000])
    ap.add_argument("--knn-points", type=int, default=100000)
    ap.add_argument("--far-points", type=int, default=20000)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--fuse-views", type=int, default=32)
    ap.add_argument("--ring", type=int, default=32)
    ap.add_argument("--hw", type=int, default=800)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from nerfpp_amd import align as A, geometry as G, mesh as M, points as P, raster as R, scene as S, tsdf as T
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
    iso_mesh = R.FilterVisible(full, T.OrbitViews(a.ring, a.hw, a.hw, K, 4.0))
    del full
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    dev = tsdf_mesh.Vertices.device
    lib = G.L.lib()
    out = dict(repeats=a.repeats, warmup=a.warmup, res=a.res, mesh_build_s=time.time() - t0, bbox=box.tolist(), build={}, nearest={}, far={}, knn={}, normals={}, icp={})

    def keep(section, name, row):
        out[section][name] = row
        print(json.dumps({f"{section}:{name}": row}), file=sys.stderr, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(json.dumps(out) + "\n")

    def nearest_row(q, t, bvh):
        st = torch.zeros((3,), device=dev, dtype=torch.int32)
        want = G.NearestPoints(q, t, bbox=box, stats=st)
        got = G.NearestPoints(q, bvh)
        coh = P.KNearest(q, bvh, 1, coherent=True)
        same = same_bytes(want[0], got[0]) and same_bytes(want[1], got[1]) and same_bytes(want[0], coh.Dist2) and same_bytes(want[1], coh.Index)
        g_first, g_ms = timed_auto(lambda: G.NearestPoints(q, t, bbox=box), a.warmup, a.repeats)
        b_first, b_ms = timed_auto(lambda: G.NearestPoints(q, bvh), a.warmup, a.repeats)
        _, c_ms = timed_auto(lambda: P.KNearest(q, bvh, 1, coherent=True), a.warmup, a.repeats)
        return dict(queries=int(q.shape[0]), targets=int(t.shape[0]), grid_first_ms=g_first, grid_ms=g_ms, grid_fallback_queries=int(st[2]), bvh_first_ms=b_first, bvh_ms=b_ms,
                    bvh_coherent_ms=c_ms, bvh_over_grid=b_ms / max(g_ms, 1e-9), same_bits=same, winner="bvh" if min(b_ms, c_ms) < g_ms else "grid")

    for n in a.points:
        samples = {name: G.SampleSurface(m, n_points=n, seed=0).Points for name, m in (("tsdf", tsdf_mesh), ("iso_visible", iso_mesh))}
        bvhs = {}
        for name, pts in samples.items():
            m = int(pts.shape[0])
            p_first, p_ms = timed_auto(lambda: P.PointBVH(pts), a.warmup, a.repeats)
            faces = torch.arange(m, device=dev, dtype=torch.int32)[:, None].repeat(1, 3).contiguous()
            as_mesh = M.Mesh(pts, faces, torch.zeros_like(pts))
            m_first, m_ms = timed_auto(lambda: G.MeshBVH(as_mesh), a.warmup, a.repeats)
            bvhs[name] = P.PointBVH(pts)
            same = same_bytes(bvhs[name].Buffer[8:], G.MeshBVH(as_mesh).Buffer[8:])
            del faces, as_mesh
            keep("build", f"{n}:{name}", dict(points=m, point_first_ms=p_first, point_ms=p_ms, mesh_iii_first_ms=m_first, mesh_iii_ms=m_ms, point_over_mesh=p_ms / max(m_ms, 1e-9),
                                              bvh_bytes=int(bvhs[name].Buffer.numel()), bytes_per_point=bvhs[name].Buffer.numel() / max(m, 1),
                                              workspace_bytes=int(lib.nrf_point_bvh_workspace_bytes(m)), grid_workspace_bytes_for_a_query=int(lib.nrf_nearest_points_workspace_bytes(
                                                  m, m, *G.GridDims(box, m))), same_bytes_past_the_magic=same))
        for qname, tname in (("tsdf", "iso_visible"), ("iso_visible", "tsdf")):
            keep("nearest", f"{n}:{qname}->{tname}", nearest_row(samples[qname], samples[tname], bvhs[tname]))
        if n == a.points[0]:
            centre = torch.as_tensor((box[:3] + box[3:]) / 2, device=dev)
            for times in (10.0, 1000.0):
                far = (centre + (samples["tsdf"][:a.far_points] - centre) * (2.0 * times)).contiguous()
                keep("far", f"{a.far_points}:tsdf x {times:g} diagonals->iso_visible", nearest_row(far, samples["iso_visible"], bvhs["iso_visible"]))
            # k > 1 beside cdist + topk at a size where that finishes
            q, t = samples["tsdf"][:a.knn_points].contiguous(), samples["iso_visible"][:a.knn_points].contiguous()
            small = P.PointBVH(t)
            for k in (8, 16, 32):
                got = P.KNearest(q, small, k)
                wd, wi = cdist_topk(q, t, k, 4096)
                agree = float((got.Index.to(torch.int64) == wi).float().mean())          # cdist forms the distance through a matrix product: ties and last bits differ
                _, c_ms = timed_auto(lambda: cdist_topk(q, t, k, 4096), a.warmup, a.repeats)
                b_first, b_ms = timed_auto(lambda: P.KNearest(q, small, k), a.warmup, a.repeats)
                _, full_ms = timed_auto(lambda: P.KNearest(samples["tsdf"], bvhs["iso_visible"], k), a.warmup, a.repeats)
                keep("knn", f"k={k}", dict(queries=int(q.shape[0]), targets=int(t.shape[0]), cdist_topk_ms=c_ms, bvh_first_ms=b_first, bvh_ms=b_ms, bvh_over_cdist=b_ms / max(c_ms, 1e-9),
                                           index_agreement_with_cdist=agree, max_abs_distance_difference=float((got.Dist2.sqrt() - wd).abs().max()),
                                           bvh_ms_at_full_size=full_ms, full_size=[int(samples["tsdf"].shape[0]), int(samples["iso_visible"].shape[0])]))
            # normals and outlier scores of one cloud
            pts, bvh = samples["tsdf"], bvhs["tsdf"]
            m = int(pts.shape[0])
            nn = P.KNearest(pts, bvh, 16, exclude_self=True)
            normals, eigen = torch.empty_like(pts), torch.empty_like(pts)
            _, knn_ms = timed_auto(lambda: P.KNearest(pts, bvh, 16, exclude_self=True), a.warmup, a.repeats)
            _, coh_ms = timed_auto(lambda: P.KNearest(pts, bvh, 16, exclude_self=True, coherent=True), a.warmup, a.repeats)
            _, nrm_ms = timed_auto(lambda: G.L.check(lib.nrf_points_normals(pts.data_ptr(), m, nn.Index.data_ptr(), 16, None, 0, normals.data_ptr(), eigen.data_ptr(), None, None)),
                                   a.warmup, a.repeats)
            _, est_ms = timed_auto(lambda: P.EstimateNormals(pts, k=16, bvh=bvh), a.warmup, a.repeats)
            _, out_ms = timed_auto(lambda: P.StatisticalOutliers(pts, k=16, bvh=bvh), a.warmup, a.repeats)
            _, score_ms = timed_auto(lambda: P.ValueStats(P.MeanNeighborDistance(nn.Dist2)), a.warmup, a.repeats)
            res = P.EstimateNormals(pts, k=16, bvh=bvh)
            keep_mask, _ = P.StatisticalOutliers(pts, k=16, bvh=bvh)
            keep("normals", f"{n}:tsdf", dict(points=m, knn16_self_ms=knn_ms, knn16_self_coherent_ms=coh_ms, normals_kernel_ms=nrm_ms, estimate_normals_ms=est_ms, scores_and_stats_ms=score_ms,
                                              statistical_outliers_ms=out_ms, valid=int(res.Valid.sum()), kept=int(keep_mask.sum()),
                                              two_runs_same_bits=same_bytes(res.Normals, P.EstimateNormals(pts, k=16, bvh=bvh).Normals)))
            # one ICP iteration against a cloud: point mode through the grid, plane mode through the PointBVH
            half = math.radians(10.0) / 2.0
            axis = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
            away = A.Transform(quaternion=[math.cos(half)] + list(math.sin(half) * axis), scale=1.1, translation=(0.05, -0.03, 0.02), device=dev).Inverse()
            src = away.Apply(samples["tsdf"])
            cloud = samples["tsdf"]
            _, point_ms = timed_auto(lambda: A.RegisterICP(src, cloud, iterations=1, method="point", scale=True), a.warmup, a.repeats)
            _, plane_ms = timed_auto(lambda: A.RegisterICP(src, cloud, iterations=1, method="plane", scale=True, target_normals=res.Normals), a.warmup, a.repeats)
            _, plane5_ms = timed_auto(lambda: A.RegisterICP(src, cloud, iterations=5, method="plane", scale=True, target_normals=res.Normals), a.warmup, a.repeats)
            _, point5_ms = timed_auto(lambda: A.RegisterICP(src, cloud, iterations=5, method="point", scale=True), a.warmup, a.repeats)
            keep("icp", f"{n}:tsdf moved->tsdf cloud", dict(points=m, point_one_iteration_with_box_sync_ms=point_ms, plane_one_iteration_with_build_ms=plane_ms,
                                                           point_five_iterations_ms=point5_ms, plane_five_iterations_ms=plane5_ms,
                                                           point_per_iteration_ms=(point5_ms - point_ms) / 4.0, plane_per_iteration_ms=(plane5_ms - plane_ms) / 4.0))
            del small, nn, normals, eigen, res
        del samples, bvhs
        torch.cuda.empty_cache()
    out["same_bits_everywhere"] = all(row["same_bits"] for sec in ("nearest", "far") for row in out[sec].values()) and \
        all(row["same_bytes_past_the_magic"] for row in out["build"].values())
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
