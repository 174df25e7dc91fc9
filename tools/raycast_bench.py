"""Time the ray-casting entries on one MI355X, on the meshes DESIGN 8m / 8p measure (tools/closest_bench.py builds the same): the TSDF mesh of --fuse-views orbit
views at --res, the density isosurface at the 0.7 quantile thinned by FilterVisible, and both simplified at --factor times the extraction step.  Per mesh:
  * an --hw x --hw camera's rays through RayCastView's path (GetRays + nrf_ray_cast_mesh, closest mode): first call, median of the repeats, rays per second, the
    share the brute-force fallback served; any mode over the same rays; and the yardstick, RenderMesh of the same pinhole view (the ratio is reported, no threshold);
  * --rays random rays of a training batch's kind (random pixels of a ring of cameras), closest and any mode;
  * the acceptance yardstick: the same definition composed from torch ops by brute force, --torch-rays of those rays against ALL faces in [rays, faces] tiles of
    --torch-chunk faces with a running key minimum, SCALED by n / torch-rays (the whole problem does not fit a run), with the share of rays whose T and Face have
    the same bits.
Per simplified mesh:
  * AmbientOcclusion at its vertices (k = --k) fused, against its own composition HemisphereDirections -> packed rays -> Occluded, bit for bit;
  * BakeAmbientOcclusion at --tile.
Warm-up first, then device events and the median of the repeats with the first call apart; a call above 50 ms is repeated 3 times.  Every row is printed to stderr as
it is measured and the JSON written so far is kept, so a run that is cut short leaves what it had.
    python tools/raycast_bench.py [--res 512] [--rays 1000000] [--hw 800] [--k 64] [--out profiles/raycast/raycast_bench.json]
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


def torch_cast(rays, a, b, c, chunk):
    """The header's definition from torch ops: rays [n, 8] against all faces (a, b, c [F, 3]) in tiles -> (t [n], face [n]); one torch op per source operation"""
    n = rays.shape[0]
    none = (0x7F800000 << 32) | 0xFFFFFFFF
    best = torch.full((n,), none, device=rays.device, dtype=torch.int64)
    dot = lambda x, y: (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]
    cross = lambda x, y: torch.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1], x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2],
                                      x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], -1)
    o, d = rays[:, None, 0:3], rays[:, None, 3:6]
    lo, hi = rays[:, None, 6].clamp(min=0.0), rays[:, None, 7]
    o_inf = o.abs().amax(-1)
    for c0 in range(0, a.shape[0], chunk):
        A, B, Cc = a[None, c0:c0 + chunk], b[None, c0:c0 + chunk], c[None, c0:c0 + chunk]
        ab, ac, tv = B - A, Cc - A, o - A
        p = cross(d.expand(n, A.shape[1], 3), ac.expand(n, A.shape[1], 3))
        det = dot(ab, p)
        inv = 1.0 / det
        v = dot(tv, p) * inv
        q = cross(tv, ab.expand(n, A.shape[1], 3))
        w = dot(d, q) * inv
        t = dot(ac, q) * inv + 0.0
        ok = (det != 0) & (v >= 0) & (w >= 0) & (v + w <= 1.0) & (t >= lo) & (t <= hi) & (t < float("inf"))
        P = (A + ab * v[..., None]) + ac * w[..., None]
        flo, fhi = torch.minimum(torch.minimum(A, B), Cc), torch.maximum(torch.maximum(A, B), Cc)
        P = torch.where(P < flo, flo, torch.where(P > fhi, fhi, P))
        tf = torch.where(torch.isfinite(t), t, torch.zeros_like(t))
        Pu = o + tf[..., None] * d
        m = torch.maximum(o_inf, Pu.abs().amax(-1))
        e = (Pu - P).abs().amax(-1)
        ok &= e <= (2.0 ** -12) * m          # a NaN fails
        key = (t.view(torch.int32).to(torch.int64) << 32) | torch.arange(c0, c0 + A.shape[1], device=rays.device, dtype=torch.int64)[None]
        best = torch.minimum(best, torch.where(ok, key, torch.full_like(key, none)).min(dim=1).values)
    return (best >> 32).to(torch.int32).view(torch.float32), (best & 0xFFFFFFFF).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--factor", type=float, default=4.0)
    ap.add_argument("--fuse-views", type=int, default=32)
    ap.add_argument("--ring", type=int, default=32)
    ap.add_argument("--hw", type=int, default=800)
    ap.add_argument("--rays", type=int, default=1000000)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--tile", type=int, default=8)
    ap.add_argument("--torch-rays", type=int, default=256)
    ap.add_argument("--torch-chunk", type=int, default=1 << 15)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from nerfpp_amd import geometry as G, mesh as M, raster as R, scene as S, texture as X, tsdf as T
    from nerfpp_amd.renderer import GetRays
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
    views = T.OrbitViews(a.ring, a.hw, a.hw, K, 4.0)
    iso_mesh = R.FilterVisible(full, views)
    del full
    cell = a.factor * step
    meshes = dict(tsdf=tsdf_mesh, iso_visible=iso_mesh, tsdf_small=M.SimplifyMesh(tsdf_mesh, cell_size=cell), iso_visible_small=M.SimplifyMesh(iso_mesh, cell_size=cell))
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    dev = tsdf_mesh.Vertices.device
    out = dict(repeats=a.repeats, warmup=a.warmup, res=a.res, cell=cell, mesh_build_s=time.time() - t0, bbox=box.tolist(), max_steps=G.RC_MAX_STEPS, tau_log2=G.RC_TAU_LOG2,
               meshes={k: [int(m.Vertices.shape[0]), int(m.Faces.shape[0])] for k, m in meshes.items()}, grids={}, view={}, batch={}, ao={}, bake={})

    def keep(section, name, row):
        out[section][name] = row
        print(json.dumps({f"{section}:{name}": row}), file=sys.stderr, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(json.dumps(out) + "\n")

    grids = {}
    for name, m in meshes.items():
        g = grids[name] = G.FaceGrid(m)          # the box of the vertices: the premise of the walk holds
        keep("grids", name, dict(dims=list(g.Dims), faces=int(m.Faces.shape[0]), n_refs=g.NRefs, n_large=g.NLarge, grid_bytes=int(g.Buffer.numel())))

    pose = views[1].Pose
    n_view = a.hw * a.hw
    o, d, _ = GetRays(a.hw, a.hw, np.asarray(K, np.float32).reshape(9), pose)
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

    def cast_rows(section, name, rays, g, m):
        n = int(rays.shape[0])
        st = torch.zeros((4,), device=dev, dtype=torch.int32)
        res = G.RayCastMesh(rays, g, stats=st)
        first, ms = timed_auto(lambda: G.RayCastMesh(rays, g), a.warmup, a.repeats)
        _, any_ms = timed_auto(lambda: G.Occluded(rays, g), a.warmup, a.repeats)
        _, lean_ms = timed_auto(lambda: G.RayCastMesh(rays, g, uv=False, points=False), a.warmup, a.repeats)
        row = dict(rays=n, faces=int(m.Faces.shape[0]), first_ms=first, ms=ms, ms_without_uv_and_points=lean_ms, any_mode_ms=any_ms, rays_per_s=n / max(ms, 1e-9) * 1e3,
                   hits=int((res.Face >= 0).sum()), fallback_rays=int(st[3]), fallback_share=int(st[3]) / max(n, 1), invalid_rays=int(st[0]))
        tv, tf = G._mesh_arrays(m)
        f64 = tf.to(torch.int64)
        ok = ((f64 >= 0) & (f64 < tv.shape[0])).all(1)
        ok &= torch.isfinite(tv[f64.clamp(0, tv.shape[0] - 1)]).all(2).all(1)
        sel = torch.nonzero(ok)[:, 0]
        if int(sel.shape[0]) != int(tf.shape[0]):
            row["torch_ops"] = "the mesh has invalid faces: the composition's face indices would not be the mesh's"
        else:
            ta, tb, tc = (tv[f64[:, k]].contiguous() for k in range(3))
            pick = torch.linspace(0, n - 1, a.torch_rays, device=dev).to(torch.int64)          # spread over the whole set
            rs = rays[pick].contiguous()
            got = {}

            def by_torch():
                got["t"], got["face"] = torch_cast(rs, ta, tb, tc, a.torch_chunk)
            t_first, t_ms = timed_auto(by_torch, 1, 3)
            same_t = float((got["t"].view(torch.int32) == res.T[pick].view(torch.int32)).float().mean())
            same_f = float((got["face"] == res.Face[pick]).float().mean())
            scaled = t_ms * n / max(int(rs.shape[0]), 1)
            row["torch_ops"] = dict(rays=int(rs.shape[0]), chunk=a.torch_chunk, first_ms=t_first, ms=t_ms, scaled_to_all_rays_ms=scaled, scaled=True, same_t_bits=same_t,
                                    same_face=same_f, times_slower_than_the_kernel=scaled / max(ms, 1e-9))
            row["no_slower_than_torch"] = bool(ms <= scaled)
            row["torch_agrees_bit_for_bit"] = bool(same_t == 1.0 and same_f == 1.0)
            del ta, tb, tc, got
        keep(section, name, row)
        return row

    for name, m in meshes.items():
        row = cast_rows("view", name, view_rays, grids[name], m)
        whole_first, whole = timed_auto(lambda: R.RayCastView(grids[name], pose, a.hw, a.hw, K), a.warmup, a.repeats)
        _, ras = timed_auto(lambda: R.RenderMesh(m, pose, a.hw, a.hw, K, attrs=()), a.warmup, a.repeats)
        rc, rm = R.RayCastView(grids[name], pose, a.hw, a.hw, K), R.RenderMesh(m, pose, a.hw, a.hw, K, attrs=())
        row.update(ray_cast_view_ms=whole, render_mesh_ms=ras, ray_cast_over_render_mesh=whole / max(ras, 1e-9),
                   same_face_share=float((rc.FaceMap == rm.FaceMap).float().mean()), hit_pixels=[int((rc.FaceMap >= 0).sum()), int((rm.FaceMap >= 0).sum())])
        keep("view", name, row)
        del rc, rm
        cast_rows("batch", name, batch_rays, grids[name], m)
        torch.cuda.empty_cache()

    for name in ("tsdf_small", "iso_visible_small"):
        m, g = meshes[name], grids[name]
        nrm = m.Normals if m.Normals is not None else M.VertexNormals(m)
        at = (m.Vertices, nrm)
        n = int(m.Vertices.shape[0])
        diag = G._box_diagonal(g.Box)
        off, md = G.AO_OFFSET * diag, G.AO_MAX_DIST * diag
        st = torch.zeros((4,), device=dev, dtype=torch.int32)
        ao = G.AmbientOcclusion(m, k=a.k, grid=g, at=at, stats=st)
        first, ms = timed_auto(lambda: G.AmbientOcclusion(m, k=a.k, grid=g, at=at), a.warmup, a.repeats)

        def composed():
            dirs = G.HemisphereDirections(nrm, a.k)
            nh = torch.nn.functional.normalize(nrm, dim=1)          # timing only; the bit-for-bit composition is the GPU test's
            rays = torch.zeros((n, a.k, 8), device=dev)
            rays[..., 0:3], rays[..., 3:6], rays[..., 7] = (m.Vertices + off * nh)[:, None, :], dirs, md
            return G.Occluded(rays.reshape(-1, 8), g)
        c_first, c_ms = timed_auto(composed, 1, 3)
        occ = composed().reshape(n, a.k).sum(1)
        two = (a.k - occ).to(torch.float32) / float(a.k)
        keep("ao", name, dict(points=n, k=a.k, rays=n * a.k, offset=off, max_dist=md, first_ms=first, ms=ms, rays_per_s=n * a.k / max(ms, 1e-9) * 1e3, mean_ao=float(ao.mean()),
                              fallback_rays=int(st[3]), fallback_share=int(st[3]) / max(n * a.k, 1), invalid_rays=int(st[0]), composed_first_ms=c_first, composed_ms=c_ms,
                              fused_no_slower_than_composed=bool(ms <= c_ms), composed_agrees_share=float((two == ao).float().mean())))
        b_first, b_ms = timed_auto(lambda: X.BakeAmbientOcclusion(m, tile=a.tile, k=a.k, grid=g), 0, 3)
        bst = torch.zeros((4,), device=dev, dtype=torch.int32)
        atlas = X.BakeAmbientOcclusion(m, tile=a.tile, k=a.k, grid=g, stats=bst)
        texels = int(atlas.Image.shape[0] * atlas.Image.shape[1])
        # invalid rays: the k rays of every texel without an owner (it has no normal); they are never walked
        keep("bake", name, dict(tile=a.tile, k=a.k, atlas=list(atlas.Image.shape), texels=texels, rays=texels * a.k, first_ms=b_first, ms=b_ms,
                                fallback_rays=int(bst[3]), fallback_share=int(bst[3]) / max(texels * a.k, 1), invalid_rays=int(bst[0]),
                                mean_ao_of_owned=float(atlas.Image[atlas.Image > 0].mean()) if bool((atlas.Image > 0).any()) else 0.0))
        del atlas
    rows = list(out["view"].values()) + list(out["batch"].values())
    out["no_slower_than_torch_everywhere"] = all(v.get("no_slower_than_torch", False) for v in rows)
    out["torch_agrees_everywhere"] = all(v.get("torch_agrees_bit_for_bit", False) for v in rows)
    out["fused_ao_no_slower_everywhere"] = all(v["fused_no_slower_than_composed"] for v in out["ao"].values())
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
