"""Time the mesh rasteriser on one MI355X, on the meshes the library itself makes from the bench hash scene (make_hash_scene()): the TSDF mesh of --fuse-views orbit
views at --tsdf-res, and the density isosurfaces at the 0.7 quantile of the density (the noise-like worst case of DESIGN 8b) at each --iso-res.  Per mesh:
  * nrf_raster_mesh through RenderMesh at --hw x --hw: one view, and a ring of --ring views one call each; cull none / back; no attribute and eight (colours, normals
    and a 2-column relevancy); ms per view and faces per second;
  * the traffic floor of the design as built -- 28 B per vertex (12 read, 16 written by the pre-pass), 12 B per face of indices, 48 B per face of corner gathers, 8 B
    per pixel of z-buffer -- at the streaming rate DESIGN 8j measured (3.2 TB/s), and the measured time over it;
  * the share of faces that take the wide kernel (the header's rule restated in torch ops), the pixels hit (a lower bound of the atomics that lowered a key) and the
    summed screen area of the drawn faces in pixels (the expected number of covered face-pixel pairs: an upper bound of the atomics, the plain-load filter removes some);
  * FilterVisible over the ring: faces before and after (--filter-visible);
  * EvaluateMesh over --eval-views views for a mesh that has colours.
The field render of the same view (RenderView) is timed for context.  Warm-up first, then device events and the median of the repeats.  One JSON line on stdout.
    python tools/raster_bench.py [--meshes tsdf iso256 iso512] [--hw 800] [--ring 32] [--repeats 9] [--warmup 2] [--filter-visible iso512] [--eval-views 4] [--wide-pixels N] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STREAM_GB_S = 3200.0          # what nrf_tsdf_integrate reaches on this part (3.1-3.3 TB/s)
FACE_CHUNK = 1 << 25


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


def face_census(mesh, pose, hw, K, wide_pixels):
    """The header's steps 1-5 up to the bounding box in torch ops (fused kernels: not bit-exact, good for a census) -> (wide faces, drawn faces, their summed area in pixels)"""
    dev = mesh.Vertices.device
    c2w = torch.as_tensor(np.asarray(pose, np.float32)[:3, :4], device=dev)
    k = np.asarray(K, np.float32).reshape(3, 3)
    cam = (mesh.Vertices - c2w[:, 3]) @ c2w[:, :3]
    zd = -cam[:, 2]
    u = float(k[0, 0]) * (cam[:, 0] / zd) + float(k[0, 2])
    v = float(k[1, 2]) - float(k[1, 1]) * (cam[:, 1] / zd)
    ok = (zd > 1e-3) & (u.abs() <= 16384) & (v.abs() <= 16384)
    X = torch.where(ok, torch.round(u * 256.0), torch.zeros_like(u)).to(torch.int64)
    Y = torch.where(ok, torch.round(v * 256.0), torch.zeros_like(v)).to(torch.int64)
    del cam, zd, u, v
    wide = drawn = 0
    area = 0.0
    for i in range(0, mesh.Faces.shape[0], FACE_CHUNK):
        f = mesh.Faces[i:i + FACE_CHUNK].to(torch.int64)
        x, y, good = X[f], Y[f], ok[f].all(-1)
        A = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
        good &= A != 0
        i0, i1 = ((x.amin(-1) + 255) >> 8).clamp_min(0), (x.amax(-1) >> 8).clamp_max(hw - 1)
        j0, j1 = ((y.amin(-1) + 255) >> 8).clamp_min(0), (y.amax(-1) >> 8).clamp_max(hw - 1)
        box = (i1 - i0 + 1).clamp_min(0) * (j1 - j0 + 1).clamp_min(0)
        wide += int((good & (box > wide_pixels)).sum())
        drawn += int(good.sum())
        area += float((A.abs().to(torch.float64) * good).sum()) / (2.0 * 256.0 * 256.0)
    return wide, drawn, area


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", nargs="+", default=["tsdf", "iso256", "iso512"])
    ap.add_argument("--tsdf-res", type=int, default=512)
    ap.add_argument("--fuse-views", type=int, default=32)
    ap.add_argument("--hw", type=int, default=800)
    ap.add_argument("--ring", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--filter-visible", nargs="*", default=["iso512"])
    ap.add_argument("--eval-views", type=int, default=4)
    ap.add_argument("--wide-pixels", type=int, default=None, help="the NRF_RASTER_WIDE_PIXELS of a tuning library loaded through NRF_LIB_PATH (census only)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from nerfpp_amd import mesh as M, raster as R, scene as S, tsdf as T
    from nerfpp_amd.renderer import RenderView
    torch.cuda.set_device(0)
    sc = S.make_hash_scene()
    r = sc["renderer"]
    rp = S.lego_render_params(sc["bbox"])
    K = S.lego_K(a.hw, a.hw)
    ring = T.OrbitViews(a.ring, a.hw, a.hw, K, 4.0)
    wide_pixels = R.WIDE_PIXELS if a.wide_pixels is None else a.wide_pixels
    out = dict(repeats=a.repeats, warmup=a.warmup, hw=a.hw, ring=a.ring, stream_gb_per_s=STREAM_GB_S, wide_pixels=wide_pixels,
               lib=os.path.relpath(os.environ["NRF_LIB_PATH"]) if os.environ.get("NRF_LIB_PATH") else "default")
    out["field_render_ms"], _ = timed(lambda: RenderView(r, ring[0].Pose, a.hw, a.hw, K, rp), 1, 3)
    for name in a.meshes:
        if name == "tsdf":
            m = T.ExtractMeshTSDF(r, T.OrbitViews(a.fuse_views, a.hw, a.hw, K, 4.0), rp, resolution=a.tsdf_res)
        else:
            res = int(name[3:])
            sigma = M.DensityGrid(r, None, res)
            iso = float(torch.quantile(sigma.reshape(-1)[::97].float(), 0.7))
            del sigma
            m = M.ExtractMesh(r, iso, resolution=res, colors=res <= 256)
        torch.cuda.empty_cache()
        nv, nf, px = int(m.Vertices.shape[0]), int(m.Faces.shape[0]), a.hw * a.hw
        row = dict(verts=nv, faces=nf, has_colors=m.Colors is not None)
        row["floor_bytes"] = 28 * nv + 60 * nf + 8 * px
        row["floor_ms"] = row["floor_bytes"] / STREAM_GB_S * 1e-6
        wide, drawn, area = face_census(m, ring[0].Pose, a.hw, K, wide_pixels)
        row.update(wide_faces=wide, wide_share=wide / max(nf, 1), census_drawn=drawn, sum_face_area_px=area)
        eight = M.Mesh(m.Vertices, m.Faces, m.Normals, m.Colors if m.Colors is not None else m.Normals.abs(), m.Normals[:, :2].contiguous())
        for cull in ("none", "back"):
            for label, mesh_, attrs in (("attr0", m, ()), ("attr8", eight, ("Colors", "Normals", "Relevancy"))):
                key = f"{cull}_{label}"
                ms, every = timed(lambda: R.RenderMesh(mesh_, ring[0].Pose, a.hw, a.hw, K, cull=cull, attrs=attrs), a.warmup, a.repeats)
                row[key + "_ms"], row[key + "_all_ms"] = ms, every
                row[key + "_faces_per_s"] = nf / ms * 1e3
                row[key + "_over_floor"] = ms / row["floor_ms"]

                def around():
                    for v in ring:
                        R.RenderMesh(mesh_, v.Pose, a.hw, a.hw, K, cull=cull, attrs=attrs)
                ms, _ = timed(around, 1, max(3, a.repeats // 3))
                row[key + "_ring_ms_per_view"] = ms / len(ring)
            one = R.RenderMesh(m, ring[0].Pose, a.hw, a.hw, K, cull=cull, attrs=())
            row[cull + "_stats"] = one.Stats.cpu().tolist()
            row[cull + "_pixels_hit"] = int((one.FaceMap >= 0).sum())
        del eight
        if name in a.filter_visible:
            seen = R.VisibleFaces(m, ring)
            row["visible_faces"] = int(seen.sum())
            row["visible_faces_back_culled"] = int(R.VisibleFaces(m, ring, cull="back").sum())
            del seen
        if m.Colors is not None and a.eval_views > 0:
            ev = R.EvaluateMesh(m, r, T.OrbitViews(a.eval_views, a.hw, a.hw, K, 4.0), rp)
            row["evaluate_mesh"] = {k: v.tolist() for k, v in ev.items()}
        out[name] = row
        print(json.dumps({name: row}), file=sys.stderr, flush=True)
        del m
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
