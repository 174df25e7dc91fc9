"""Time texture baking and textured rendering on one MI355X, on the meshes DESIGN 8m simplifies: the bench hash scene's (make_hash_scene()) TSDF mesh of
--fuse-views orbit views at --res and its visible density isosurface, each simplified at cells of --factors extraction steps.  Per simplified mesh and tile of --tiles:
  * the atlas (width, height, texels, the share of them that has an owner);
  * nrf_atlas_texels over the whole atlas with every output, against a floor of bytes moved at the streaming rate DESIGN 8j measured (3.2 TB/s): 72 B written per
    texel (face 4, barycentrics 12, position 12, ray 44), 12 B read per face and 24 B per vertex (position and normal);
  * BakeTexture from the network in mode="point" and in mode="render" (--bake-samples coarse + as many fine samples on rays of one cell above and below the surface);
  * nrf_texture_shade alone at --hw x --hw on a RenderMesh result, bilinear and nearest, against 28 B streamed per pixel (face 4, barycentrics 12, colour 12; the
    gathers of a hit pixel -- 12 B of indices, 36 B of vertices, up to 48 B of texels -- are listed beside it), and RenderMeshTextured whole;
  * the same texels and the same shading composed from torch ops on the same GPU (index arithmetic and gathers; fused arithmetic, so close, not bit-equal);
  * EvaluateMesh over --eval-views views with the vertex colours and with the baked atlas, both modes.
A call above 50 ms is repeated 3 times, one above 2 s is timed once (a bake: its first run).  Warm-up first, then device events and the median of the repeats.  One JSON line on stdout.
    python tools/texture_bench.py [--res 512] [--factors 2 4 8] [--tiles 4 8 16] [--meshes tsdf iso_visible] [--eval-views 4] [--no-torch] [--repeats 9] [--out FILE]
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

from tools.geometry_bench import floor_ms, timed, STREAM_GB_S          # noqa: E402


def timed_auto(fn, warmup, repeats):
    """timed(), but a call above 50 ms is repeated 3 times and one above 2 s is the one run that found that out"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()          # first launches load code objects
    a.record()
    fn()
    b.record()
    b.synchronize()
    first = a.elapsed_time(b)
    return first if first > 2000.0 else timed(fn, 0, 3) if first > 50.0 else timed(fn, warmup, repeats)


def timed_bake(fn):
    """(ms, the result of fn): the first run where it takes more than 2 s (set-up is nothing beside it), else the median of 3 more"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res = fn()
    b.record()
    b.synchronize()
    first = a.elapsed_time(b)
    return (first if first > 2000.0 else timed(fn, 0, 3)), res


def torch_texels(verts, faces, normals, tile, offset, layout):
    """nrf_atlas_texels from torch ops -> (face [h, w] int64, pos [h, w, 3], rays [h, w, 11], the length of the interpolated vertex normal [h, w])"""
    w, h, cols, _ = layout
    dev = verts.device
    nf = faces.shape[0]
    Y, X = torch.arange(h, device=dev)[:, None], torch.arange(w, device=dev)[None, :]
    i, j = (X % tile).expand(h, w), (Y % tile).expand(h, w)
    upper = i + j > tile - 2
    f = 2 * ((X // tile) + cols * (Y // tile)) + upper
    i, j = torch.where(upper, tile - 1 - i, i), torch.where(upper, tile - 1 - j, j)
    fc = faces[f.clamp_max(nf - 1)].to(torch.int64)
    p0 = verts[fc[..., 0]]
    e1, e2 = verts[fc[..., 1]] - p0, verts[fc[..., 2]] - p0
    c = torch.linalg.cross(e1, e2)
    ln = torch.linalg.vector_norm(c, dim=-1)
    own = (f < nf) & (ln > 0)
    b1, b2 = i.to(torch.float32) / (tile - 3), j.to(torch.float32) / (tile - 3)
    b0 = (1.0 - b1) - b2
    pos = p0 + (b1[..., None] * e1 + b2[..., None] * e2)
    m = (b0[..., None] * normals[fc[..., 0]] + b1[..., None] * normals[fc[..., 1]]) + b2[..., None] * normals[fc[..., 2]]
    lm = torch.linalg.vector_norm(m, dim=-1)
    n = torch.where((lm > 0)[..., None], m / lm[..., None], c / ln[..., None])
    z = torch.zeros_like(ln)[..., None]
    rays = torch.cat([pos + offset * n, -n, z, z + 2.0 * offset, -n], -1)
    keep = own[..., None]
    return torch.where(own, f, -1), torch.where(keep, pos, z), torch.where(keep, rays, z), lm


def torch_shade(verts, faces, face_map, bary_map, c2w, image, tile, cols):
    """nrf_texture_shade (bilinear) from torch ops -> [h, w, C]"""
    dev = verts.device
    m = torch.as_tensor(np.asarray(c2w, np.float32)[:3, :4], device=dev)
    zd = -((verts - m[:, 3]) @ m[:, 2])
    hit = face_map >= 0
    f = face_map.clamp_min(0).to(torch.int64)
    p = bary_map / zd[faces[f].to(torch.int64)]
    beta = p / p.sum(-1, keepdim=True)
    n = tile - 3
    x, y = (beta[..., 1] * n).nan_to_num(0.0).clamp(0, n), (beta[..., 2] * n).nan_to_num(0.0).clamp(0, n)
    ix, iy = torch.floor(x), torch.floor(y)
    fx, fy = x - ix, y - iy
    cell, odd = f >> 1, (f & 1) == 1
    x0, y0 = (cell % cols) * tile, (cell // cols) * tile
    out = torch.zeros(face_map.shape + (image.shape[2],), device=dev)
    for di, dj, wgt in ((0, 0, (1 - fx) * (1 - fy)), (1, 0, fx * (1 - fy)), (0, 1, (1 - fx) * fy), (1, 1, fx * fy)):
        i, j = ix.to(torch.int64) + di, iy.to(torch.int64) + dj
        read = hit & (i + j <= n + 1)
        tx, ty = torch.where(odd, x0 + tile - 1 - i, x0 + i), torch.where(odd, y0 + tile - 1 - j, y0 + j)
        val = image[torch.where(read, ty, 0), torch.where(read, tx, 0)]
        out = out + torch.where(read[..., None], wgt[..., None] * val, torch.zeros_like(val))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--factors", type=float, nargs="+", default=[2.0, 4.0, 8.0])
    ap.add_argument("--tiles", type=int, nargs="+", default=[4, 8, 16])
    ap.add_argument("--meshes", nargs="+", default=["tsdf", "iso_visible"])
    ap.add_argument("--fuse-views", type=int, default=32)
    ap.add_argument("--ring", type=int, default=32)
    ap.add_argument("--hw", type=int, default=800)
    ap.add_argument("--bake-samples", type=int, default=16)
    ap.add_argument("--eval-views", type=int, default=4)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from nerfpp_amd import _lib as L, mesh as M, raster as R, scene as S, texture as X, tsdf as T
    from nerfpp_amd.dataset import _k9, _m12
    from nerfpp_amd.modules import _ptr, _stream
    torch.cuda.set_device(0)
    sc = S.make_hash_scene()
    r = sc["renderer"]
    rp = S.lego_render_params(sc["bbox"])
    rp_bake = S.lego_render_params(sc["bbox"], n_samples=a.bake_samples, n_importance=a.bake_samples)
    K = S.lego_K(a.hw, a.hw)
    box = np.asarray(sc["bbox"], np.float32).reshape(6)
    step = float((box[3:] - box[:3]).max()) / (a.res - 1)
    views = T.OrbitViews(a.eval_views, a.hw, a.hw, K, 4.0)
    pose = T.OrbitViews(a.ring, a.hw, a.hw, K, 4.0)[0].Pose
    lib = L.lib()
    t0 = time.time()
    inputs = {}
    if "tsdf" in a.meshes:
        inputs["tsdf"] = T.ExtractMeshTSDF(r, T.OrbitViews(a.fuse_views, a.hw, a.hw, K, 4.0), rp, resolution=a.res)
    if "iso_visible" in a.meshes:
        sigma = M.DensityGrid(r, None, a.res)
        iso = float(torch.quantile(sigma.reshape(-1)[::97].float(), 0.7))
        del sigma
        m = R.FilterVisible(M.ExtractMesh(r, iso, resolution=a.res, colors=False), T.OrbitViews(a.ring, a.hw, a.hw, K, 4.0))
        rgb = torch.empty_like(m.Vertices)          # ExtractMesh's colours, for the vertices FilterVisible kept
        for i in range(0, rgb.shape[0], M.COLOR_CHUNK):
            raw = r.RunNetwork(m.Vertices[i:i + M.COLOR_CHUNK][:, None, :], (-m.Normals[i:i + M.COLOR_CHUNK]).contiguous(), L.NRF_PREC_F32)
            rgb[i:i + M.COLOR_CHUNK] = torch.sigmoid(raw[:, 0, :3])
        m.Colors = rgb
        inputs["iso_visible"] = m
    torch.cuda.empty_cache()
    out = dict(repeats=a.repeats, warmup=a.warmup, res=a.res, step=step, hw=a.hw, stream_gb_per_s=STREAM_GB_S, mesh_build_s=time.time() - t0, bake_samples=a.bake_samples,
               meshes={k: [int(m.Vertices.shape[0]), int(m.Faces.shape[0])] for k, m in inputs.items()})
    k9, m12 = _k9(K), _m12(pose)
    score = lambda ev: {k: float(ev["mean_" + k]) for k in ("psnr", "ssim", "depth_error", "iou")}
    for name, full in inputs.items():
        rows = {}
        for factor in a.factors:
            cell = factor * step
            small = M.SimplifyMesh(full, cell_size=cell)
            verts, faces = X._mesh_arrays(small)
            normals = small.Normals.contiguous()
            nv, nf = int(verts.shape[0]), int(faces.shape[0])
            row = dict(cell=cell, verts=nv, faces=nf)
            if a.eval_views > 0:
                row["evaluate_vertex_colours"] = score(R.EvaluateMesh(small, r, views, rp))
            ras = R.RenderMesh(small, pose, a.hw, a.hw, K, attrs=())
            hit = int((ras.FaceMap >= 0).sum())
            row["pixels_hit"] = hit
            row["render_mesh_colours_ms"] = timed_auto(lambda: R.RenderMesh(small, pose, a.hw, a.hw, K, attrs=("Colors",)), a.warmup, a.repeats)
            for tile in a.tiles:
                layout = X.AtlasLayout(nf, tile)
                w, h = layout[0], layout[1]
                n_tex = w * h
                t = dict(width=w, height=h, texels=n_tex)
                face = torch.empty((h, w), device=verts.device, dtype=torch.int32)
                bary, pos, rays = torch.empty((h, w, 3), device=verts.device), torch.empty((h, w, 3), device=verts.device), torch.empty((h, w, 11), device=verts.device)

                def texels():
                    L.check(lib.nrf_atlas_texels(_ptr(verts), nv, _ptr(faces), nf, _ptr(normals), tile, cell, 0, h, _ptr(face), _ptr(bary), _ptr(pos), _ptr(rays), _stream()))
                t["texels_ms"] = timed_auto(texels, a.warmup, a.repeats)
                t["owned_share"] = float((face >= 0).sum()) / n_tex
                t["texels_floor_ms"] = floor_ms(72 * n_tex + 12 * nf + 24 * nv)
                t["texels_over_floor"] = t["texels_ms"] / t["texels_floor_ms"]
                t["texels_gb_per_s"] = (72 * n_tex + 12 * nf + 24 * nv) / t["texels_ms"] * 1e-6
                if not a.no_torch:
                    tf, tp, tr, lm = torch_texels(verts, faces, normals, tile, cell, layout)
                    # where the interpolated vertex normal nearly cancels its direction is ill-conditioned: such texels are counted, not folded into the maximum
                    far = (tr - rays).abs().amax(-1) > 1e-5
                    t["torch_texels"] = dict(ms=timed_auto(lambda: torch_texels(verts, faces, normals, tile, cell, layout), 1, 3), same_faces=bool(torch.equal(tf.to(torch.int32), face)),
                                             max_position_difference=float((tp - pos).abs().max()), max_ray_difference=float((tr - rays).abs().max()),
                                             rays_beyond_1e5=int(far.sum()), longest_normal_there=float(torch.where(far, lm, torch.zeros_like(lm)).max()),
                                             max_ray_difference_elsewhere=float(torch.where(far[..., None], torch.zeros_like(tr), tr - rays).abs().max()))
                    del tf, tp, tr, lm, far
                del face, bary, pos, rays
                torch.cuda.empty_cache()
                atlases = {}
                t["bake_point_ms"], atlases["point"] = timed_bake(lambda: X.BakeTexture(small, r, tile=tile, mode="point"))
                t["bake_render_ms"], atlases["render"] = timed_bake(lambda: X.BakeTexture(small, r, tile=tile, mode="render", rparams=rp_bake, offset=cell))
                t["render_acc_mean_owned"] = float(atlases["render"].Acc.sum()) / max(t["owned_share"] * n_tex, 1.0)
                image = atlases["point"].Image
                shaded = torch.empty((a.hw, a.hw, 3), device=verts.device)
                for flt_name, flt in (("bilinear", X.BILINEAR), ("nearest", X.NEAREST)):
                    def shade():
                        L.check(lib.nrf_texture_shade(_ptr(verts), nv, _ptr(faces), nf, _ptr(ras.FaceMap), _ptr(ras.BaryMap), a.hw, a.hw, k9.ctypes.data_as(C.c_void_p),
                                                      m12.ctypes.data_as(C.c_void_p), _ptr(image), tile, 3, flt, _ptr(shaded), _stream()))
                    t[f"shade_{flt_name}_ms"] = timed_auto(shade, a.warmup, a.repeats)
                t["shade_floor_ms"] = floor_ms(28 * a.hw * a.hw)
                t["shade_gather_bytes"] = 96 * hit
                t["shade_bilinear_over_floor"] = t["shade_bilinear_ms"] / t["shade_floor_ms"]
                t["render_mesh_textured_ms"] = timed_auto(lambda: X.RenderMeshTextured(small, atlases["point"], pose, a.hw, a.hw, K), a.warmup, a.repeats)
                if not a.no_torch:
                    L.check(lib.nrf_texture_shade(_ptr(verts), nv, _ptr(faces), nf, _ptr(ras.FaceMap), _ptr(ras.BaryMap), a.hw, a.hw, k9.ctypes.data_as(C.c_void_p),
                                                  m12.ctypes.data_as(C.c_void_p), _ptr(image), tile, 3, X.BILINEAR, _ptr(shaded), _stream()))
                    ts = torch_shade(verts, faces, ras.FaceMap, ras.BaryMap, pose, image, tile, layout[2])
                    t["torch_shade"] = dict(ms=timed_auto(lambda: torch_shade(verts, faces, ras.FaceMap, ras.BaryMap, pose, image, tile, layout[2]), 1, 3),
                                            max_difference=float((ts - shaded).abs().max()))
                    del ts
                if a.eval_views > 0:
                    for mode, atlas in atlases.items():
                        t["evaluate_" + mode] = score(R.EvaluateMesh(small, r, views, rp, texture=atlas))
                del atlases, image, shaded
                torch.cuda.empty_cache()
                row[f"tile{tile}"] = t
                print(json.dumps({name: {f"x{factor:g}": {f"tile{tile}": t}}}), file=sys.stderr, flush=True)
            rows[f"x{factor:g}"] = row
            del small, ras
            torch.cuda.empty_cache()
        out[name] = rows
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
