"""Time registration on one MI355X, on the meshes DESIGN 8m / 8p measure: the TSDF mesh of --fuse-views orbit views at --res (about 11 M faces) and the same mesh
simplified at --factor times the extraction step.  The source of every run is the target's own surface, sampled at each count of --points and carried into another
frame (10 degrees about (1, 2, 3), scale 1 / 1.1, a shift of 0.05), so that the run has a pose to find.  Per (target mesh, sample count):
  * the FaceGrid of the target (built once, outside every timing below);
  * one iteration from the start pose, split into its four calls: nrf_align_apply, nrf_closest_on_mesh (the query), nrf_align_sums and nrf_align_solve, in both
    modes; "new_kernels_ms" is apply + sums + solve;
  * the whole run: RegisterICP(--iterations, method plane and point, scale=True) with tolerance=None (no synchronisation inside), its pose error at the end;
  * the comparison: the same point-to-point iteration composed from ClosestOnMesh + torch float64 ops (the pose applied as a matrix product, means, the 3x3
    covariance, torch.linalg.svd, the Umeyama scale, the composed pose), query apart from the rest.
Warm-up first, then device events and the median of the repeats; a call above 50 ms is repeated 3 times.  One JSON line on stdout.
    python tools/align_bench.py [--points 100000 1000000] [--res 512] [--factor 4] [--iterations 10] [--repeats 9] [--warmup 2] [--out profiles/align/align_bench.json]
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


def torch_point_step(y, p, keep, pose):
    """One Umeyama update from torch float64 ops: pose [4, 4] <- the similarity that fits y[keep] onto p[keep], composed with pose"""
    yk, pk = y[keep].double(), p[keep].double()
    yb, pb = yk.mean(0), pk.mean(0)
    yc, pc = yk - yb, pk - pb
    U, D, Vt = torch.linalg.svd(pc.T @ yc)
    sg = torch.ones(3, dtype=torch.float64, device=y.device)
    sg[2] = torch.sign(torch.linalg.det(U) * torch.linalg.det(Vt))
    R = U @ torch.diag(sg) @ Vt
    s = (D * sg).sum() / (yc * yc).sum()
    step = torch.eye(4, dtype=torch.float64, device=y.device)
    step[:3, :3] = s * R
    step[:3, 3] = pb - s * (R @ yb)
    return step @ pose


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--factor", type=float, default=4.0)
    ap.add_argument("--fuse-views", type=int, default=32)
    ap.add_argument("--hw", type=int, default=800)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from nerfpp_amd import align as A, geometry as G, mesh as M, scene as S, tsdf as T
    torch.cuda.set_device(0)
    sc = S.make_hash_scene()
    rp = S.lego_render_params(sc["bbox"])
    box = np.asarray(sc["bbox"], np.float32).reshape(6)
    step = float((box[3:] - box[:3]).max()) / (a.res - 1)
    t0 = time.time()
    dense = T.ExtractMeshTSDF(sc["renderer"], T.OrbitViews(a.fuse_views, a.hw, a.hw, S.lego_K(a.hw, a.hw), 4.0), rp, resolution=a.res)
    meshes = dict(tsdf=dense, tsdf_small=M.SimplifyMesh(dense, cell_size=a.factor * step))
    torch.cuda.synchronize()
    dev = dense.Vertices.device
    half = math.radians(10.0) / 2.0
    axis = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    truth = A.Transform(quaternion=[math.cos(half)] + list(math.sin(half) * axis), scale=1.1, translation=(0.05, -0.03, 0.02), device=dev)
    away = truth.Inverse()
    out = dict(repeats=a.repeats, warmup=a.warmup, res=a.res, iterations=a.iterations, mesh_build_s=time.time() - t0,
               meshes={k: [int(m.Vertices.shape[0]), int(m.Faces.shape[0])] for k, m in meshes.items()}, runs={})
    for name, m in meshes.items():
        grid = G.FaceGrid(m, bbox=box)
        for n in a.points:
            src = away.Apply(G.SampleSurface(m, n_points=n, seed=0).Points)
            nq = int(src.shape[0])
            row = dict(samples=nq, faces=int(m.Faces.shape[0]))
            start = A.Transform(device=dev)
            y = torch.empty_like(src)
            first, row["apply_ms"] = timed_auto(lambda: start.Apply(src, out=y), a.warmup, a.repeats)
            res = G.ClosestOnMesh(y, grid, uv=False)
            first, row["query_ms"] = timed_auto(lambda: G.ClosestOnMesh(y, grid, uv=False), a.warmup, a.repeats)
            for method, mode in (("plane", A.ALIGN_PLANE), ("point", A.ALIGN_POINT)):
                ws = A._workspace(nq, mode, dev)
                state, hist = A.Transform(device=dev).State, torch.zeros((1, 8), device=dev, dtype=torch.float64)
                lib = A.L.lib()

                def sums():
                    A._sums_solve(y, res.Points, res.Face, mode, True, grid, state, hist, 0, ws)
                both = timed_auto(sums, a.warmup, a.repeats)[1]
                solve = timed_auto(lambda: A.L.check(lib.nrf_align_solve(nq, mode, 1, 0, 1, state.data_ptr(), hist.data_ptr(), ws.data_ptr(), ws.numel(), A._stream())),
                                   a.warmup, a.repeats)[1]
                row[method] = dict(sums_ms=both - solve, solve_ms=solve, new_kernels_ms=row["apply_ms"] + both,
                                   iteration_ms=row["apply_ms"] + row["query_ms"] + both, query_share=row["query_ms"] / (row["apply_ms"] + row["query_ms"] + both))
                keep = {}

                def whole():
                    keep["r"] = A.RegisterICP(src, grid, iterations=a.iterations, method=method, scale=True)
                first, ms = timed_auto(whole, 1, a.repeats)
                st = keep["r"].Transform.State.cpu().numpy()
                err = (keep["r"].Transform.Matrix - truth.Matrix).abs().max()
                row[method].update(run_first_ms=first, run_ms=ms, run_ms_per_iteration=ms / a.iterations, pose_matrix_error=float(err), scale=float(st[4]),
                                   flags=keep["r"].History[:, 2].tolist())
            pose = torch.eye(4, dtype=torch.float64, device=dev)
            keep_pairs = res.Face >= 0
            t_rest = timed_auto(lambda: torch_point_step((src.double() @ pose[:3, :3].T + pose[:3, 3]).float(), res.Points, keep_pairs, pose), a.warmup, a.repeats)[1]
            row["torch_point_iteration"] = dict(rest_ms=t_rest, query_ms=row["query_ms"], iteration_ms=t_rest + row["query_ms"],
                                                rest_over_new_kernels=t_rest / max(row["point"]["new_kernels_ms"], 1e-9))
            out["runs"][f"{name}:{n}"] = row
            print(json.dumps({f"{name}:{n}": row}), file=sys.stderr, flush=True)
            del src, y, res
        del grid
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
