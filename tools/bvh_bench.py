"""Time the mesh BVH against the face grid on one MI355X, in one process on the same inputs: the meshes and pairs of tools/closest_bench.py, raycast_bench.py and
align_bench.py (the TSDF mesh of --fuse-views orbit views at --res, the visible density isosurface, both simplified at --factor times the extraction step).
  * build: FaceGrid(mesh) (count with its synchronisation + build) against MeshBVH(mesh) (no synchronisation), the bytes of both buffers;
  * closest: --points surface samples of one dense mesh against the other, both directions, on dense and simplified targets: ClosestOnMesh over the grid, over the
    BVH, and over the BVH with coherent=True (the Morton sort of the queries included, and apart); the grid's fallback queries; the outputs compared bit for bit;
  * far: --far-points of the same samples pushed 10 and 1000 box diagonals away (the grid's ring walk gives up: its brute-force fallback), a twentieth of them on
    the dense target, where every fallback query is a workgroup over 11 M faces;
  * rays: the --hw x --hw rays of one camera of the ring and --rays random pixels of four others, RayCastMesh and Occluded, grid / BVH / BVH coherent; and the same
    rays with origins moved 1000 diagonals back along the ray (the grid's far-origin fallback), on the simplified targets;
  * icp: one iteration's query, ClosestOnMesh(points=True, uv=False) of samples moved by a 10-degree pose, grid against BVH (the rest of an iteration does not depend
    on the structure).
Warm-up first, then device events and the median of the repeats; a call above 50 ms is repeated 3 times; the first call is reported apart.  One JSON line on stdout.
    python tools/bvh_bench.py [--points 1000000 10000000] [--res 512] [--rays 1000000] [--out profiles/bvh/bvh_bench.json]
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
    return a is b or bool(torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[1000000, 10000000])
    ap.add_argument("--rays", type=int, default=1000000)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--factor", type=float, default=4.0)
    ap.add_argument("--fuse-views", type=int, default=32)
    ap.add_argument("--ring", type=int, default=32)
    ap.add_argument("--hw", type=int, default=800)
    ap.add_argument("--far-points", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from nerfpp_amd import align as A, geometry as G, mesh as M, raster as R, scene as S, tsdf as T
    from nerfpp_amd.renderer import GetRays
    torch.cuda.set_device(0)
    sc = S.make_hash_scene()
    r = sc["renderer"]
    rp = S.lego_render_params(sc["bbox"])
    K = S.lego_K(a.hw, a.hw)
    box = np.asarray(sc["bbox"], np.float32).reshape(6)
    diag = float(np.linalg.norm(box[3:] - box[:3]))
    step = float((box[3:] - box[:3]).max()) / (a.res - 1)
    t0 = time.time()
    tsdf_mesh = T.ExtractMeshTSDF(r, T.OrbitViews(a.fuse_views, a.hw, a.hw, K, 4.0), rp, resolution=a.res)
    sigma = M.DensityGrid(r, None, a.res)
    iso = float(torch.quantile(sigma.reshape(-1)[::97].float(), 0.7))
    del sigma
    full = M.ExtractMesh(r, iso, resolution=a.res, colors=False)
    views = T.OrbitViews(a.ring, a.hw, a.hw, K, 4.0)
    iso_mesh = R.FilterVisible(full, views)
    del full
    cell = a.factor * step
    meshes = dict(tsdf=tsdf_mesh, iso_visible=iso_mesh, tsdf_small=M.SimplifyMesh(tsdf_mesh, cell_size=cell), iso_visible_small=M.SimplifyMesh(iso_mesh, cell_size=cell))
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    dev = tsdf_mesh.Vertices.device
    out = dict(repeats=a.repeats, warmup=a.warmup, res=a.res, cell=cell, mesh_build_s=time.time() - t0, bbox=box.tolist(), max_depth=G.BVH_MAX_DEPTH,
               meshes={k: [int(m.Vertices.shape[0]), int(m.Faces.shape[0])] for k, m in meshes.items()}, build={}, closest={}, far={}, rays={}, far_rays={}, icp={})

    def keep(section, name, row):
        out[section][name] = row
        print(json.dumps({f"{section}:{name}": row}), file=sys.stderr, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(json.dumps(out) + "\n")

    grids, bvhs = {}, {}
    for name, m in meshes.items():
        g_first, g_ms = timed_auto(lambda: G.FaceGrid(m, bbox=box), a.warmup, a.repeats)
        b_first, b_ms = timed_auto(lambda: G.MeshBVH(m), a.warmup, a.repeats)
        grids[name], bvhs[name] = G.FaceGrid(m, bbox=box), G.MeshBVH(m)
        keep("build", name, dict(faces=int(m.Faces.shape[0]), grid_first_ms=g_first, grid_ms=g_ms, grid_bytes=int(grids[name].Buffer.numel()), grid_dims=list(grids[name].Dims),
                                 grid_large=grids[name].NLarge, bvh_first_ms=b_first, bvh_ms=b_ms, bvh_bytes=int(bvhs[name].Buffer.numel()),
                                 bvh_workspace_bytes=int(G.L.lib().nrf_mesh_bvh_workspace_bytes(int(m.Faces.shape[0]))), bvh_over_grid=b_ms / max(g_ms, 1e-9)))

    def closest_row(q, tname, **kw):
        g, b = grids[tname], bvhs[tname]
        nq = int(q.shape[0])
        st = torch.zeros((4,), device=dev, dtype=torch.int32)
        want = G.ClosestOnMesh(q, g, stats=st, **kw)
        got, coh = G.ClosestOnMesh(q, b, **kw), G.ClosestOnMesh(q, b, coherent=True, **kw)
        same = all(same_bytes(getattr(want, k), getattr(x, k)) for x in (got, coh) for k in ("Dist2", "Face", "UV", "Points") if getattr(want, k) is not None)
        g_first, g_ms = timed_auto(lambda: G.ClosestOnMesh(q, g, **kw), a.warmup, a.repeats)
        b_first, b_ms = timed_auto(lambda: G.ClosestOnMesh(q, b, **kw), a.warmup, a.repeats)
        _, c_ms = timed_auto(lambda: G.ClosestOnMesh(q, b, coherent=True, **kw), a.warmup, a.repeats)
        _, order_ms = timed_auto(lambda: b.Order(q), a.warmup, a.repeats)
        fin = torch.isfinite(want.Dist2)
        return dict(queries=nq, faces=int(meshes[tname].Faces.shape[0]), grid_first_ms=g_first, grid_ms=g_ms, grid_fallback_queries=int(st[3]), bvh_first_ms=b_first, bvh_ms=b_ms,
                    bvh_coherent_ms=c_ms, of_which_order_ms=order_ms, bvh_over_grid=b_ms / max(g_ms, 1e-9), coherent_over_bvh=c_ms / max(b_ms, 1e-9), same_bits=same,
                    mean_distance=float(want.Dist2[fin].sqrt().mean()) if bool(fin.any()) else None, winner="bvh" if min(b_ms, c_ms) < g_ms else "grid")

    pairs = [("tsdf", "iso_visible"), ("iso_visible", "tsdf"), ("tsdf", "iso_visible_small"), ("iso_visible", "tsdf_small")]
    for n in a.points:
        samples = {name: G.SampleSurface(meshes[name], n_points=n, seed=0).Points for name in ("tsdf", "iso_visible")}
        for qname, tname in pairs:
            keep("closest", f"{n}:{qname}->{tname}", closest_row(samples[qname], tname))
        if n == a.points[0]:
            centre = torch.as_tensor((box[:3] + box[3:]) / 2, device=dev)
            for qname, tname, count in (("tsdf", "iso_visible_small", a.far_points), ("iso_visible", "tsdf_small", a.far_points), ("iso_visible", "tsdf", a.far_points // 20)):
                for times in (10.0, 1000.0):          # far queries: the grid's rings end and its brute-force fallback, a workgroup over all faces per query, takes over
                    q = samples[qname][:count]
                    far = (centre + (q - centre) * (2.0 * times)).contiguous()          # up to `times` box diagonals from the centre
                    keep("far", f"{count}:{qname} x {times:g} diagonals->{tname}", closest_row(far, tname))
            # one ICP iteration's query: samples moved by a 10-degree pose, the closest point wanted, no uv
            half = math.radians(10.0) / 2.0
            axis = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
            away = A.Transform(quaternion=[math.cos(half)] + list(math.sin(half) * axis), scale=1.1, translation=(0.05, -0.03, 0.02), device=dev).Inverse()
            for tname in ("tsdf", "tsdf_small"):
                keep("icp", f"{n}:tsdf moved->{tname}", closest_row(away.Apply(samples["tsdf"]), tname, uv=False))
        del samples
        torch.cuda.empty_cache()

    n_view = a.hw * a.hw
    o, d, _ = GetRays(a.hw, a.hw, np.asarray(K, np.float32).reshape(9), views[1].Pose)
    view_rays = torch.zeros((n_view, 8), device=dev)
    view_rays[:, 0:3], view_rays[:, 3:6], view_rays[:, 7] = o.reshape(-1, 3), d.reshape(-1, 3), float("inf")
    per_view = -(-a.rays // 4)
    parts = []
    gen = torch.Generator(device="cpu").manual_seed(0)
    for v in views[2:6]:          # random pixels of four cameras of the ring: a training batch's rays
        oo, dd, _ = GetRays(a.hw, a.hw, np.asarray(K, np.float32).reshape(9), v.Pose)
        pick = torch.randint(0, n_view, (per_view,), generator=gen).to(dev)
        part = torch.zeros((per_view, 8), device=dev)
        part[:, 0:3], part[:, 3:6], part[:, 7] = oo.reshape(-1, 3)[pick], dd.reshape(-1, 3)[pick], float("inf")
        parts.append(part)
    batch_rays = torch.cat(parts)[:a.rays].contiguous()
    del parts

    def rays_row(rays, tname):
        g, b = grids[tname], bvhs[tname]
        n = int(rays.shape[0])
        st = torch.zeros((4,), device=dev, dtype=torch.int32)
        want = G.RayCastMesh(rays, g, stats=st)
        got, coh = G.RayCastMesh(rays, b), G.RayCastMesh(rays, b, coherent=True)
        same = all(same_bytes(getattr(want, k), getattr(x, k)) for x in (got, coh) for k in ("T", "Face", "UV", "Points"))
        same = same and same_bytes(G.Occluded(rays, g), G.Occluded(rays, b))
        g_first, g_ms = timed_auto(lambda: G.RayCastMesh(rays, g), a.warmup, a.repeats)
        b_first, b_ms = timed_auto(lambda: G.RayCastMesh(rays, b), a.warmup, a.repeats)
        _, c_ms = timed_auto(lambda: G.RayCastMesh(rays, b, coherent=True), a.warmup, a.repeats)
        _, g_any = timed_auto(lambda: G.Occluded(rays, g), a.warmup, a.repeats)
        _, b_any = timed_auto(lambda: G.Occluded(rays, b), a.warmup, a.repeats)
        return dict(rays=n, faces=int(meshes[tname].Faces.shape[0]), hits=int((want.Face >= 0).sum()), grid_first_ms=g_first, grid_ms=g_ms, grid_fallback_rays=int(st[3]),
                    bvh_first_ms=b_first, bvh_ms=b_ms, bvh_coherent_ms=c_ms, grid_any_ms=g_any, bvh_any_ms=b_any, bvh_over_grid=b_ms / max(g_ms, 1e-9),
                    coherent_over_bvh=c_ms / max(b_ms, 1e-9), any_bvh_over_grid=b_any / max(g_any, 1e-9), same_bits=same, winner="bvh" if min(b_ms, c_ms) < g_ms else "grid")

    for tname in meshes:
        keep("rays", f"view {a.hw}x{a.hw}->{tname}", rays_row(view_rays, tname))
        keep("rays", f"batch {a.rays}->{tname}", rays_row(batch_rays, tname))
    for tname in ("tsdf_small", "iso_visible_small"):          # origins 1000 diagonals back along the ray: the grid's far-origin rule sends them to its fallback
        far = view_rays[::64].clone()
        far[:, 0:3] = far[:, 0:3] - far[:, 3:6] / far[:, 3:6].norm(dim=1, keepdim=True) * (1000.0 * diag)
        keep("far_rays", f"{int(far.shape[0])} origins 1000 diagonals back->{tname}", rays_row(far.contiguous(), tname))
    out["same_bits_everywhere"] = all(row["same_bits"] for sec in ("closest", "far", "rays", "far_rays", "icp") for row in out[sec].values())
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
