"""Time mesh adjacency, smoothing and vertex normals on one MI355X, on the meshes tools/simplify_bench.py builds from the bench hash scene (make_hash_scene()): the
TSDF mesh of --fuse-views orbit views at --res, the density isosurface at the 0.7 quantile of the density at --res thinned by FilterVisible over a ring of --ring
views, and SimplifyMesh of each at every cell size of --factors times the extraction step.  Per mesh:
  * nrf_mesh_adjacency_count (its synchronisation included) and nrf_mesh_adjacency_emit, the workspace bytes and d_stats;
  * one nrf_mesh_smooth step (iterations = 1, mu = 0) at C = 3 under every boundary mode and at C = 1 and 4, each against the bytes model V*C*4 read and written plus
    n_neighbours * (4 + 4*C) gathered (and 16 B of row starts per vertex) at the streaming rate DESIGN 8j measured (3.2 TB/s);
  * nrf_mesh_vertex_normals under both weightings against V*(16 + 12) + n_incident * (4 + 12 + 36) bytes;
  * the same operations composed from torch ops on the same GPU in the same process: the step as index_add_ of the gathered neighbours over the directed edge list
    (float atomics), a division by the degree and the update; the normals as three index_add_ of the face cross products and a normalisation; the neighbour list
    itself as torch.unique over the 6F directed edge keys.  The largest difference between the two results is reported (the torch sums are not ordered).
Warm-up first, then device events and the median of the repeats.  A call above 50 ms is repeated 3 times, not --repeats; a call below 5 ms is timed as --batch
calls back to back between one pair of events (a window of one 0.2 ms call measures the events as much as the kernel), the same way for both sides.  The repeats
leave the arrays in the Infinity Cache where they fit (256 MiB): a time below the bytes model at the HBM streaming rate says so.  One JSON line on stdout.
    python tools/smooth_bench.py [--res 512] [--factors 4] [--repeats 9] [--warmup 2] [--batch 20] [--out FILE]
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

BATCH = 20


def timed_call(fn, warmup, repeats):
    """ms per call: timed_auto, and for a call below 5 ms BATCH calls per pair of events"""
    ms = timed_auto(fn, warmup, repeats)
    if ms >= 5.0:
        return ms

    def batch():
        for _ in range(BATCH):
            fn()
    return timed(batch, 1, repeats) / BATCH


def torch_edges(faces, n_verts):
    """(own, nbr) of every directed edge once, ascending: what d_nbr_start / d_nbr hold, from torch.unique over 6F keys (valid faces assumed)"""
    f = faces.to(torch.int64)
    a = torch.cat([f[:, 0], f[:, 0], f[:, 1], f[:, 1], f[:, 2], f[:, 2]])
    b = torch.cat([f[:, 1], f[:, 2], f[:, 0], f[:, 2], f[:, 0], f[:, 1]])
    key = torch.unique(a * n_verts + b)
    return key // n_verts, key % n_verts


def torch_step(x, own, nbr, degree, factor):
    s = torch.zeros_like(x).index_add_(0, own, x[nbr])
    m = s / degree[:, None]
    return torch.where(degree[:, None] > 0, x + factor * (m - x), x)


def torch_normals(verts, faces):
    f = faces.to(torch.int64)
    a, b, c = verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]]
    n = torch.linalg.cross(b - a, c - a)
    s = torch.zeros_like(verts)
    for k in range(3):
        s.index_add_(0, f[:, k], n)
    length = torch.linalg.vector_norm(s, dim=1, keepdim=True)
    return torch.where(length > 0, s / length, torch.zeros_like(s))


def main():
    global BATCH
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--factors", type=float, nargs="+", default=[4.0])
    ap.add_argument("--fuse-views", type=int, default=32)
    ap.add_argument("--ring", type=int, default=32)
    ap.add_argument("--hw", type=int, default=800)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=BATCH)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    BATCH = max(1, a.batch)
    from nerfpp_amd import _lib as L, mesh as M, raster as R, scene as S, tsdf as T
    from nerfpp_amd.modules import _ptr, _stream
    torch.cuda.set_device(0)
    sc = S.make_hash_scene()
    r = sc["renderer"]
    rp = S.lego_render_params(sc["bbox"])
    K = S.lego_K(a.hw, a.hw)
    box = np.asarray(sc["bbox"], np.float32).reshape(6)
    step = float((box[3:] - box[:3]).max()) / (a.res - 1)
    lib = L.lib()

    def measure(name, m):
        verts = m.Vertices.contiguous()
        faces = m.Faces.to(torch.int32).contiguous()
        dev = verts.device
        nv, nf = int(verts.shape[0]), int(faces.shape[0])
        ws = torch.empty((max(1, int(lib.nrf_mesh_adjacency_workspace_bytes(nv, nf))),), device=dev, dtype=torch.uint8)
        ni, nn = C.c_int64(0), C.c_int64(0)

        def count():
            L.check(lib.nrf_mesh_adjacency_count(_ptr(faces), nv, nf, C.addressof(ni), C.addressof(nn), _ptr(ws), ws.numel(), _stream()))
        count_ms = timed_auto(count, a.warmup, a.repeats)
        adj = M.BuildAdjacency(m)
        outs = [torch.empty_like(t) for t in (adj.FaceStart, adj.FaceList, adj.NbrStart, adj.Nbr, adj.NbrFaces, adj.Flags, adj.Stats)]

        def emit():
            L.check(lib.nrf_mesh_adjacency_emit(_ptr(faces), nv, nf, ni.value, nn.value, *[_ptr(o) for o in outs], _ptr(ws), ws.numel(), _stream()))
        emit_ms = timed_auto(emit, a.warmup, a.repeats)
        del ws, outs
        torch.cuda.empty_cache()
        n_nbr, n_inc = int(adj.Nbr.numel()), int(adj.FaceList.numel())
        row = dict(verts=nv, faces=nf, n_incident=n_inc, n_neighbours=n_nbr, stats=adj.stats, topology=M.MeshTopology(adj), adjacency_count_ms=count_ms,
                   adjacency_emit_ms=emit_ms, adjacency_workspace_bytes=int(lib.nrf_mesh_adjacency_workspace_bytes(nv, nf)), step={})
        gen = torch.Generator(device=dev).manual_seed(1)
        for c, modes in ((3, ("free", "fixed", "curve")), (1, ("free",)), (4, ("free",))):
            x = verts if c == 3 else torch.randn((nv, c), device=dev, generator=gen)
            out, tmp = torch.empty_like(x), torch.empty_like(x)
            model = floor_ms(nv * c * 8 + nv * 16 + n_nbr * (4 + 4 * c))
            for mode in modes:
                def one():
                    L.check(lib.nrf_mesh_smooth(_ptr(x), _ptr(out), _ptr(tmp), nv, c, 1, 0.5, 0.0, M._BOUNDARIES[mode], _ptr(adj.NbrStart), _ptr(adj.Nbr), _ptr(adj.NbrFaces),
                                                _ptr(adj.Flags), n_nbr, _stream()))
                ms = timed_call(one, a.warmup, a.repeats)
                row["step"][f"C{c}_{mode}"] = dict(ms=ms, model_ms=model, over_model=ms / model if model else None)
        normals = torch.empty_like(verts)
        nmodel = floor_ms(nv * 28 + n_inc * 52)
        for weighting in ("area", "unit"):
            def nrm():
                L.check(lib.nrf_mesh_vertex_normals(_ptr(verts), nv, _ptr(faces), nf, _ptr(adj.FaceStart), _ptr(adj.FaceList), n_inc, M._WEIGHTINGS[weighting], _ptr(normals),
                                                    _stream()))
            ms = timed_call(nrm, a.warmup, a.repeats)
            row["normals_" + weighting] = dict(ms=ms, model_ms=nmodel, over_model=ms / nmodel if nmodel else None)
        if not a.no_torch and nf:
            valid = row["stats"]["bad_index"] == 0 and row["stats"]["repeated_corner"] == 0
            t = dict(valid_faces_only=valid)
            t["edges_ms"] = timed_auto(lambda: torch_edges(faces, nv), 1, 3)
            own, nbr = torch_edges(faces, nv)
            t["same_neighbours"] = bool(valid and nbr.numel() == n_nbr and torch.equal(nbr.to(torch.int32), adj.Nbr))
            degree = torch.bincount(own, minlength=nv).to(torch.float32)
            for c in (3, 1, 4):
                x = verts if c == 3 else torch.randn((nv, c), device=dev, generator=gen)
                t[f"step_C{c}_ms"] = timed_call(lambda: torch_step(x, own, nbr, degree, 0.5), a.warmup, a.repeats)
                if c == 3:
                    got = M._smooth("smooth_bench", x, adj, 1, 0.5, 0.0, M.SMOOTH_FREE)
                    t["step_max_difference"] = float((torch_step(x, own, nbr, degree, 0.5) - got).abs().max()) if t["same_neighbours"] else None
            t["normals_ms"] = timed_call(lambda: torch_normals(verts, faces), a.warmup, a.repeats)
            got = M.VertexNormals(m, "area", adjacency=adj)
            t["normals_max_difference"] = float((torch_normals(verts, faces) - got).abs().max()) if valid else None
            t["hip_step_not_slower"] = all(row["step"][f"C{c}_free"]["ms"] <= t[f"step_C{c}_ms"] for c in (3, 1, 4))
            t["hip_normals_not_slower"] = row["normals_area"]["ms"] <= t["normals_ms"]
            row["torch_ops"] = t
            del own, nbr, degree
        print(json.dumps({name: row}), file=sys.stderr, flush=True)
        del adj
        torch.cuda.empty_cache()
        return row

    t0 = time.time()
    tsdf_mesh = T.ExtractMeshTSDF(r, T.OrbitViews(a.fuse_views, a.hw, a.hw, K, 4.0), rp, resolution=a.res)
    sigma = M.DensityGrid(r, None, a.res)
    iso = float(torch.quantile(sigma.reshape(-1)[::97].float(), 0.7))
    del sigma
    full = M.ExtractMesh(r, iso, resolution=a.res, colors=False)
    iso_mesh = R.FilterVisible(full, T.OrbitViews(a.ring, a.hw, a.hw, K, 4.0))
    del full
    torch.cuda.empty_cache()
    out = dict(repeats=a.repeats, warmup=a.warmup, batch=BATCH, res=a.res, step=step, stream_gb_per_s=STREAM_GB_S, mesh_build_s=time.time() - t0)
    for name, m in (("tsdf", tsdf_mesh), ("iso_visible", iso_mesh)):
        out[name] = measure(name, m)
        for factor in a.factors:
            small = M.SimplifyMesh(m, cell_size=factor * step)
            out[f"{name}_x{factor:g}"] = measure(f"{name}_x{factor:g}", small)
            del small
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
