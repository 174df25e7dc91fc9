"""Time depth fusion on one MI355X, on what the library itself produces from the bench hash scene (make_hash_scene()): --views orbit views of --hw x --hw rendered once
with RenderView (DepthMap, AccMap, RGBMap stay on the device), then, at each --res and for each view count:
  * nrf_tsdf_integrate over all views in one call (16 views per launch) and one view per call, with colour: time per call and per view, and the volume bytes the
    launches move (40 B per lattice point per launch; 8 B without colour) over that time, against the 6.3 TB/s a streaming kernel can reach on this part;
  * the same definition composed from torch ops (project, gather, where), one view at a time -- what a user would otherwise write -- on --torch-views views;
  * TSDFVolume.Extract (Isosurface + observed filter + colours; its stream synchronisations included, wall clock);
  * the face counts of ExtractMeshTSDF's mesh and of ExtractMesh at the 0.7 quantile of the density (the noise-like worst case of DESIGN 8b) at the same resolution.
Warm-up first, then hipEvent timing and the median of the repeats; the volume is reset before every timed call.  One JSON line on stdout; --out also writes it to a file.
    python tools/tsdf_bench.py [--res 512 256] [--views 8 32] [--hw 800] [--repeats 5] [--warmup 2] [--torch-views 2] [--no-density-mesh] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_ACHIEVABLE_GB_S = 6300.0
LAUNCH_VIEWS = 16


def timed(fn, before, warmup, repeats):
    for _ in range(warmup):
        before()
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), ms


def torch_integrate(vol, depth, K, pose, acc, rgb):
    """nrf_tsdf_integrate's definition for one view in torch ops, in place on vol's tensors (same branches; the rounding of fused torch kernels is not pinned)."""
    from nerfpp_amd import mesh as M
    dev = vol.tsdf.device
    h, w = depth.shape
    P = M._lattice_points(vol.bbox, vol.nx, vol.ny, vol.nz, dev)
    c2w = torch.as_tensor(np.asarray(pose, np.float32)[:3, :4], device=dev)
    k = np.asarray(K, np.float32).reshape(3, 3)
    q = P - c2w[:, 3]
    cam = q @ c2w[:, :3]
    zd = -cam[:, 2]
    u = float(k[0, 0]) * (cam[:, 0] / zd) + float(k[0, 2])
    v = float(k[1, 2]) - float(k[1, 1]) * (cam[:, 1] / zd)
    fu, fv = torch.floor(u + 0.5), torch.floor(v + 0.5)
    inimg = (zd > 0) & (fu >= 0) & (fu < w) & (fv >= 0) & (fv < h)
    pix = torch.where(inimg, fv * w + fu, torch.zeros_like(fu)).to(torch.int64)
    d, a = depth.reshape(-1)[pix], acc.reshape(-1)[pix]
    solid = inimg & (a >= vol.acc_min)
    carved = inimg & (a < vol.acc_min) & vol.carve
    d = torch.where(solid, d / a, d)
    sdf = d - zd
    surface = solid & torch.isfinite(d) & (d > 0) & ~(sdf < -vol.trunc)
    s = torch.where(carved, torch.ones_like(sdf), torch.clamp(sdf / vol.trunc, max=1.0))
    upd = surface | carved
    D, W = vol.tsdf.reshape(-1), vol.weight.reshape(-1)
    Wn = W + 1.0
    D.copy_(torch.where(upd, (D * W + s) / Wn, D))
    W.copy_(torch.where(upd, torch.clamp(Wn, max=vol.max_weight), W))
    cm = surface & (sdf.abs() <= vol.trunc)
    col = vol.color.reshape(4, -1)
    cn = col[3] + 1.0
    px = rgb.reshape(-1, 3)[pix]
    for ch in range(3):
        col[ch].copy_(torch.where(cm, (col[ch] * col[3] + px[:, ch]) / cn, col[ch]))
    col[3].copy_(torch.where(cm, torch.clamp(cn, max=vol.max_weight), col[3]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[512, 256])
    ap.add_argument("--views", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--hw", type=int, default=800)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-views", type=int, default=2)
    ap.add_argument("--no-density-mesh", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from nerfpp_amd import mesh as M, scene as S, tsdf as T
    from nerfpp_amd.renderer import RenderView
    torch.cuda.set_device(0)
    sc = S.make_hash_scene()
    r = sc["renderer"]
    rp = S.lego_render_params(sc["bbox"])
    out = dict(repeats=a.repeats, warmup=a.warmup, hw=a.hw, hbm_achievable_gb_per_s=HBM_ACHIEVABLE_GB_S)
    for nv in a.views:
        views = T.OrbitViews(nv, a.hw, a.hw, S.lego_K(a.hw, a.hw), 4.0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        recs = []
        for v in views:
            o = RenderView(r, v.Pose, v.W, v.H, v.K, rp).Outputs
            recs.append((o.DepthMap.reshape(a.hw, a.hw), v.K, v.Pose, o.AccMap.reshape(a.hw, a.hw), o.RGBMap.reshape(a.hw, a.hw, 3)))
        torch.cuda.synchronize()
        out[f"render_{nv}_views_s"] = time.perf_counter() - t0
        hit = float(torch.stack([(x[3] >= 0.5).float().mean() for x in recs]).mean())
        for res in a.res:
            row = dict(views=nv, res=res, pixels_with_acc_ge_half=hit)
            vol = T.TSDFVolume(sc["bbox"], res)
            launches = -(-nv // LAUNCH_VIEWS)
            row["batched_ms"], row["batched_all_ms"] = timed(lambda: vol.IntegrateViews(recs), vol.Reset, a.warmup, a.repeats)
            row["batched_volume_bytes"] = 40 * res ** 3 * launches
            row["image_bytes"] = nv * a.hw * a.hw * 20
            row["batched_gb_per_s"] = row["batched_volume_bytes"] / row["batched_ms"] * 1e-6
            row["batched_share_of_hbm"] = row["batched_gb_per_s"] / HBM_ACHIEVABLE_GB_S
            row["batched_ms_per_view"] = row["batched_ms"] / nv

            def each():
                for x in recs:
                    vol.Integrate(*x[:3], acc=x[3], rgb=x[4])
            row["per_call_ms"], row["per_call_all_ms"] = timed(each, vol.Reset, a.warmup, a.repeats)
            row["per_call_volume_bytes"] = 40 * res ** 3 * nv
            row["per_call_gb_per_s"] = row["per_call_volume_bytes"] / row["per_call_ms"] * 1e-6
            row["per_call_ms_per_view"] = row["per_call_ms"] / nv
            plain = T.TSDFVolume(sc["bbox"], res, colors=False)
            row["batched_no_colour_ms"], _ = timed(lambda: plain.IntegrateViews(recs), plain.Reset, a.warmup, a.repeats)
            row["batched_no_colour_gb_per_s"] = 8 * res ** 3 * launches / row["batched_no_colour_ms"] * 1e-6
            del plain
            if a.torch_views > 0:
                sub = recs[:a.torch_views]

                def composed():
                    for x in sub:
                        torch_integrate(vol, x[0], x[1], x[2], x[3], x[4])
                ms, _ = timed(composed, vol.Reset, 1, max(2, a.repeats // 2))
                row["torch_ops_ms_per_view"] = ms / len(sub)
                # the composition is the same definition: after the same views the two volumes agree up to the rounding of torch's fused kernels
                vol.Reset(); composed(); t_ref = vol.tsdf.clone(); w_ref = vol.weight.clone()
                vol.Reset(); vol.IntegrateViews(sub)
                row["torch_ops_max_abs_tsdf_diff"] = float((t_ref - vol.tsdf).abs().max())
                row["torch_ops_weight_mismatches"] = int((w_ref != vol.weight).sum())
                del t_ref, w_ref
            vol.Reset()
            vol.IntegrateViews(recs)
            row["observed_fraction"] = float((vol.weight > 0).float().mean())
            for _ in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m = vol.Extract()
                torch.cuda.synchronize()
                row["extract_s"] = time.perf_counter() - t0
            row["tsdf_faces"], row["tsdf_verts"] = int(m.Faces.shape[0]), int(m.Vertices.shape[0])
            largest = M.FilterComponents(m, keep_largest=1) if m.Faces.shape[0] else m
            row["tsdf_faces_largest_component"] = int(largest.Faces.shape[0])
            del m, largest, vol
            torch.cuda.empty_cache()
            if not a.no_density_mesh and nv == a.views[-1]:
                sigma = M.DensityGrid(r, None, res)
                iso = float(torch.quantile(sigma.reshape(-1)[::97].float(), 0.7))
                del sigma
                dm = M.ExtractMesh(r, iso, resolution=res, colors=False)
                row["density_iso"], row["density_faces"] = iso, int(dm.Faces.shape[0])
                del dm
                torch.cuda.empty_cache()
            out[f"{res}_{nv}"] = row
            print(json.dumps({f"{res}_{nv}": row}), file=sys.stderr, flush=True)
        del recs
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
