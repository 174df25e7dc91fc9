"""Time the closest-point-on-a-mesh entries on one MI355X, on the meshes DESIGN 8m measures: the TSDF mesh of --fuse-views orbit views at --res, the density
isosurface at the 0.7 quantile of the density at --res thinned by FilterVisible over a ring of --ring views, and both simplified at --factor times the extraction step.
Per target mesh:
  * FaceGrid on the default dims (GridDims(box, F)): nrf_face_grid_count (its synchronisation included) + nrf_face_grid_build, the first call apart from the median of
    the repeated ones; n_refs / F, n_large, the bytes of the grid buffer;
Per (query mesh, target mesh) pair and per sample count of --points:
  * nrf_closest_on_mesh of the query mesh's surface samples against the target's faces: first call, median of the repeats, queries per second, the share of the
    queries the brute-force fallback served (d_stats);
  * yardstick 1, the same definition composed from torch ops by brute force: --torch-queries of those samples against ALL faces in chunks of --torch-chunk faces, a
    running minimum of the same key, SCALED by nq / torch-queries (the whole problem does not fit a run), and the share of those queries whose d2 has the same bits;
  * yardstick 2, nrf_nearest_points of the same samples against the target's VERTICES on its default grid: existing code, what the grid walk alone costs.
And BakeTexture(simplified mesh, source=the dense mesh it came from) at --tile, with the vertex-snapped TransferAttributes of the same vertices beside it.
Warm-up first, then device events and the median of the repeats; a call above 50 ms is repeated 3 times.  One JSON line on stdout.
    python tools/closest_bench.py [--points 1000000 10000000] [--res 512] [--factor 4] [--repeats 9] [--warmup 2] [--out profiles/closest/closest_bench.json]
"""
import argparse
import json
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


def torch_closest(q, a, b, c, chunk):
    """The header's definition from torch ops: q [n, 3] against all faces (a, b, c [F, 3]) in chunks -> (d2 [n], face [n]); one torch op per source operation"""
    n = q.shape[0]
    none = (0x7F800000 << 32) | 0xFFFFFFFF
    best = torch.full((n,), none, device=q.device, dtype=torch.int64)
    dot = lambda x, y: (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]
    qq = q[:, None, :]
    for c0 in range(0, a.shape[0], chunk):
        A, B, Cc = a[None, c0:c0 + chunk], b[None, c0:c0 + chunk], c[None, c0:c0 + chunk]
        ab, ac, ap, bp, cp = B - A, Cc - A, qq - A, qq - B, qq - Cc
        d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        w_bc = e43 / (e43 + e56)
        denom = 1.0 / ((va + vb) + vc)
        P = (A + ab * (vb * denom)[..., None]) + ac * (vc * denom)[..., None]
        for cond, cand in (((va <= 0) & (e43 >= 0) & (e56 >= 0), B + w_bc[..., None] * (Cc - B)), ((vb <= 0) & (d2 >= 0) & (d6 <= 0), A + (d2 / (d2 - d6))[..., None] * ac),
                           ((d6 >= 0) & (d5 <= d6), Cc.expand_as(P)), ((vc <= 0) & (d1 >= 0) & (d3 <= 0), A + (d1 / (d1 - d3))[..., None] * ab),
                           ((d3 >= 0) & (d4 <= d3), B.expand_as(P)), ((d1 <= 0) & (d2 <= 0), A.expand_as(P))):          # the last that holds is the first in the header's order
            P = torch.where(cond[..., None], cand, P)
        lo, hi = torch.minimum(torch.minimum(A, B), Cc), torch.maximum(torch.maximum(A, B), Cc)
        P = torch.where(P < lo, lo, torch.where(P > hi, hi, P))
        dx, dy, dz = qq[..., 0] - P[..., 0], qq[..., 1] - P[..., 1], qq[..., 2] - P[..., 2]
        dd = (dx * dx + dy * dy) + dz * dz
        key = (dd.view(torch.int32).to(torch.int64) << 32) | torch.arange(c0, c0 + A.shape[1], device=q.device, dtype=torch.int64)[None]
        key = torch.where(dd == dd, key, torch.full_like(key, none))          # a NaN never wins; d2 >= 0, so the int64 order is the key's
        best = torch.minimum(best, key.min(dim=1).values)
    return (best >> 32).to(torch.int32).view(torch.float32), (best & 0xFFFFFFFF).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[1000000, 10000000])
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--factor", type=float, default=4.0)
    ap.add_argument("--fuse-views", type=int, default=32)
    ap.add_argument("--ring", type=int, default=32)
    ap.add_argument("--hw", type=int, default=800)
    ap.add_argument("--tile", type=int, default=8)
    ap.add_argument("--torch-queries", type=int, default=512)
    ap.add_argument("--torch-chunk", type=int, default=1 << 15)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from nerfpp_amd import _lib as L, geometry as G, mesh as M, raster as R, scene as S, texture as X, tsdf as T
    torch.cuda.set_device(0)
    sc = S.make_hash_scene()
    r = sc["renderer"]
    rp = S.lego_render_params(sc["bbox"])
    K = S.lego_K(a.hw, a.hw)
    box = np.asarray(sc["bbox"], np.float32).reshape(6)
    step = float((box[3:] - box[:3]).max()) / (a.res - 1)
    t0 = time.time()
    tsdf_mesh = T.ExtractMeshTSDF(r, T.OrbitViews(a.fuse_views, a.hw, a.hw, K, 4.0), rp, resolution=a.res)
    sigma = M.DensityGrid(r, None, a.res)
    iso = float(torch.quantile(sigma.reshape(-1)[::97].float(), 0.7))
    del sigma
    full = M.ExtractMesh(r, iso, resolution=a.res, colors=False)
    iso_mesh = R.FilterVisible(full, T.OrbitViews(a.ring, a.hw, a.hw, K, 4.0))
    del full
    rgb = torch.empty_like(iso_mesh.Vertices)          # ExtractMesh's colours, for the vertices FilterVisible kept
    for i in range(0, rgb.shape[0], M.COLOR_CHUNK):
        raw = r.RunNetwork(iso_mesh.Vertices[i:i + M.COLOR_CHUNK][:, None, :], (-iso_mesh.Normals[i:i + M.COLOR_CHUNK]).contiguous(), L.NRF_PREC_F32)
        rgb[i:i + M.COLOR_CHUNK] = torch.sigmoid(raw[:, 0, :3])
    iso_mesh.Colors = rgb
    cell = a.factor * step
    meshes = dict(tsdf=tsdf_mesh, iso_visible=iso_mesh, tsdf_small=M.SimplifyMesh(tsdf_mesh, cell_size=cell), iso_visible_small=M.SimplifyMesh(iso_mesh, cell_size=cell))
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    dev = tsdf_mesh.Vertices.device
    out = dict(repeats=a.repeats, warmup=a.warmup, res=a.res, cell=cell, mesh_build_s=time.time() - t0, bbox=box.tolist(), max_face_cells=G.FG_MAX_FACE_CELLS,
               max_rings=G.NN_MAX_RINGS, meshes={k: [int(m.Vertices.shape[0]), int(m.Faces.shape[0])] for k, m in meshes.items()}, grids={}, queries={}, bake={})

    grids = {}
    for name, m in meshes.items():
        first, ms = timed_auto(lambda: G.FaceGrid(m, bbox=box), a.warmup, a.repeats)
        g = grids[name] = G.FaceGrid(m, bbox=box)
        nf = int(m.Faces.shape[0])
        out["grids"][name] = dict(dims=list(g.Dims), cells=int(np.prod(g.Dims)), faces=nf, n_refs=g.NRefs, refs_per_face=g.NRefs / max(nf, 1), n_large=g.NLarge,
                                  grid_bytes=int(g.Buffer.numel()), count_build_first_ms=first, count_build_ms=ms)
        print(json.dumps({name: out["grids"][name]}), file=sys.stderr, flush=True)

    torch_ms = {}
    pairs = [("tsdf", "iso_visible"), ("iso_visible", "tsdf"), ("tsdf", "iso_visible_small"), ("iso_visible", "tsdf_small")]
    for n in a.points:
        samples = {name: G.SampleSurface(meshes[name], n_points=n, seed=0).Points for name in ("tsdf", "iso_visible")}
        for qname, tname in pairs:
            q, g, tm = samples[qname], grids[tname], meshes[tname]
            nq = int(q.shape[0])
            st = torch.zeros((4,), device=dev, dtype=torch.int32)
            res = G.ClosestOnMesh(q, g, stats=st)
            first, ms = timed_auto(lambda: G.ClosestOnMesh(q, g), a.warmup, a.repeats)
            row = dict(queries=nq, faces=int(tm.Faces.shape[0]), first_ms=first, ms=ms, queries_per_s=nq / max(ms, 1e-9) * 1e3, fallback_queries=int(st[3]),
                       fallback_share=int(st[3]) / max(nq, 1), mean_distance=float(res.Dist2[torch.isfinite(res.Dist2)].sqrt().mean()))
            tv, tf = G._mesh_arrays(tm)
            f64 = tf.to(torch.int64)
            ok = ((f64 >= 0) & (f64 < tv.shape[0])).all(1)
            ok &= torch.isfinite(tv[f64.clamp(0, tv.shape[0] - 1)]).all(2).all(1)
            keep = torch.nonzero(ok)[:, 0]
            ta, tb, tc = (tv[f64[keep, k]].contiguous() for k in range(3))
            qs = q[:a.torch_queries].contiguous()
            if (qname, tname) not in torch_ms:          # per query the cost does not depend on how many there are: measured once per pair
                keep_d2 = {}

                def by_torch():
                    keep_d2["d2"] = torch_closest(qs, ta, tb, tc, a.torch_chunk)[0]
                torch_ms[(qname, tname)] = timed_auto(by_torch, 1, 3) + (float((keep_d2["d2"].view(torch.int32) == res.Dist2[:qs.shape[0]].view(torch.int32)).float().mean()),)
                del keep_d2
            t_first, t_ms, same = torch_ms[(qname, tname)]
            scaled = t_ms * nq / max(int(qs.shape[0]), 1)
            row["torch_ops"] = dict(queries=int(qs.shape[0]), chunk=a.torch_chunk, first_ms=t_first, ms=t_ms, scaled_to_all_queries_ms=scaled, scaled=True, same_d2_bits=same,
                                    times_slower_than_the_kernel=scaled / max(ms, 1e-9))
            np_first, np_ms = timed_auto(lambda: G.NearestPoints(q, tm.Vertices, bbox=box), a.warmup, a.repeats)
            row["nearest_points_to_vertices"] = dict(targets=int(tm.Vertices.shape[0]), first_ms=np_first, ms=np_ms, closest_over_nearest=ms / max(np_ms, 1e-9))
            row["no_slower_than_torch"] = bool(ms <= scaled)
            out["queries"][f"{n}:{qname}->{tname}"] = row
            print(json.dumps({f"{n}:{qname}->{tname}": row}), file=sys.stderr, flush=True)
            del res, ta, tb, tc
        del samples
        torch.cuda.empty_cache()

    for small, dense in (("tsdf_small", "tsdf"), ("iso_visible_small", "iso_visible")):
        if meshes[dense].Colors is None:
            out["bake"][small] = "the dense mesh has no colours"
            continue
        first, ms = timed_auto(lambda: X.BakeTexture(meshes[small], grids[dense], tile=a.tile), 1, 3)
        with_grid = timed_auto(lambda: X.BakeTexture(meshes[small], meshes[dense], tile=a.tile), 0, 3)[1]
        atlas = X.BakeTexture(meshes[small], grids[dense], tile=a.tile)
        snap = timed_auto(lambda: G.TransferAttributes(meshes[dense], meshes[small], names=("Colors",), bbox=box), 1, 3)[1]
        surf = timed_auto(lambda: G.TransferAttributes(grids[dense], meshes[small], names=("Colors",), source="surface"), 1, 3)[1]
        out["bake"][small] = dict(tile=a.tile, atlas=list(atlas.Image.shape), texels=int(atlas.Image.shape[0] * atlas.Image.shape[1]), first_ms=first, ms=ms,
                                  ms_with_the_grid_built_inside=with_grid, transfer_vertex_ms=snap, transfer_surface_ms=surf)
        print(json.dumps({small: out["bake"][small]}), file=sys.stderr, flush=True)
        del atlas
    out["no_slower_than_torch_everywhere"] = all(v["no_slower_than_torch"] for v in out["queries"].values())
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
