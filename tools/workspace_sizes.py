"""Prints what every *_workspace_bytes entry of the loaded library reports, one `name bytes` line each: the grid of tests/test_workspace_gpu.py and the bench shapes
(800 x 800, 64 + 128, Chunk 65 536 on 1 and 2 lanes; the classic and LeRF frames; the three training steps).  Run it once per library (NRF_LIB_PATH selects a
build) and join the columns: profiles/workspace_layout/sizes.txt.  Needs the GPU: the handles own device memory."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from nerfpp_amd import _lib as L, renderer as R, scene as S
    lib = L.lib()
    rows = []

    def put(name, nbytes):
        rows.append((name, int(nbytes)))

    def params(s, ni, prec, coarse=0, **kw):
        rp = L.RenderParams(s, ni, 0, 1, prec, R.ATEN_SUM_VEC)
        rp.coarse_mode = coarse
        rp.has_bbox, rp.bbox = 1, (C.c_float * 6)(*np.asarray(S.LEGO_BBOX, np.float32).reshape(6).tolist())
        for k, v in kw.items():
            setattr(rp, k, v)
        return rp

    def view(w, rows_, chunk, use_viewdirs=1):
        v = L.View()
        v.h, v.w, v.row0, v.rows = rows_, w, 0, rows_
        v.K = (C.c_float * 9)(*S.lego_K(rows_, w).reshape(-1).tolist())
        v.c2w = (C.c_float * 12)(*np.asarray(S.pose_spherical(30.0, -30.0, 4.0), np.float32).reshape(-1).tolist())
        v.use_viewdirs, v.ndc, v.chunk = use_viewdirs, 0, chunk
        v.bbox = (C.c_float * 6)(*np.asarray(S.LEGO_BBOX, np.float32).reshape(-1).tolist())
        return v

    # ---- the test grid (tiny tables)
    small = dict(cu=S.make_hash_scene(mode="cu", log2_t=12), ngp=S.make_hash_scene(mode="ngp", log2_t=12), classic=S.make_classic_scene(),
                 sh3=S.make_hash_scene(mode="cu", log2_t=12, sh_degree=3))
    lerf = S.make_lerf_scene(log2_t=12)
    for kind, sc in small.items():
        r, m = sc["renderer"]._r, sc["mlp"]._m
        for n, s in ((5, 3), (70, 7)):
            put(f"run_network {kind} {n}x{s}", lib.nrf_run_network_workspace_bytes(r, n, s))
        for n in (5, 67):
            for s, ni in ((4, 0), (4, 3), (7, 1), (8, 24)):
                for prec in (0, 1, 2):
                    for coarse in (0, 1, 2):
                        put(f"render_rays {kind} n{n} {s}+{ni} prec{prec} coarse{coarse}", lib.nrf_render_rays_workspace_bytes(r, n, C.byref(params(s, ni, prec, coarse))))
        for prec in (0, 2):
            for s, ni in ((4, 3), (8, 24)):
                for kw in (dict(perturb=1.0), dict(has_cone=1, cone_angle=0.01), dict(precond_alpha=0.02)):
                    put(f"render_rays {kind} n67 {s}+{ni} prec{prec} {sorted(kw)[0]}", lib.nrf_render_rays_workspace_bytes(r, 67, C.byref(params(s, ni, prec, **kw))))
                for bits in (1, 2, 3):
                    put(f"render_rays_normals {kind} n67 {s}+{ni} prec{prec} bits{bits}", lib.nrf_render_rays_normals_workspace_bytes(r, 67, C.byref(params(s, ni, prec)), bits))
                for lanes in (1, 2):
                    L.check(lib.nrf_renderer_set_lanes(r, lanes))
                    for n, chunk in ((150, 64), (50, 64), (33000, 9000), (33000, 40000)):
                        put(f"batchify_rays {kind} n{n} chunk{chunk} {s}+{ni} prec{prec} lanes{lanes}", lib.nrf_batchify_rays_workspace_bytes(r, n, chunk, C.byref(params(s, ni, prec))))
                    put(f"render_rows {kind} 9x7 chunk16 {s}+{ni} prec{prec} lanes{lanes}", lib.nrf_render_rows_workspace_bytes(r, C.byref(view(9, 7, 16)), C.byref(params(s, ni, prec))))
                L.check(lib.nrf_renderer_set_lanes(r, 0))
        put(f"density_grid {kind} 5x4x3 slab7", lib.nrf_density_grid_workspace_bytes(r, 5, 4, 3, 7))
        put(f"density_grad {kind} p37", lib.nrf_density_grad_workspace_bytes(r, 37))
        put(f"mlp_backward {kind} p33", lib.nrf_mlp_backward_workspace_bytes(m, 33))
    put("mlp_backward_f16 p64", lib.nrf_mlp_backward_f16_workspace_bytes(small["cu"]["mlp"]._m, 64))
    put("normal_losses 257x64", lib.nrf_normal_losses_workspace_bytes(257, 64))
    put("ray_regularizers 64x64", lib.nrf_ray_regularizers_workspace_bytes(64, 64))
    lr, lm = lerf["renderer"]._r, lerf["lerf"]._m
    for ni in (32, 64):
        rp = L.RenderParams(32, ni, 0, 0, lerf["renderer"].precision, R.ATEN_SUM_VEC)
        for n in (3, 40):
            put(f"lerf_render_rays n{n} 32+{ni}", lib.nrf_lerf_render_rays_workspace_bytes(lr, n, C.byref(rp)))
            for lanes in (1, 2):
                L.check(lib.nrf_lerf_renderer_set_lanes(lr, lanes))
                put(f"lerf_batchify_rays n{n} chunk16 32+{ni} lanes{lanes}", lib.nrf_lerf_batchify_rays_workspace_bytes(lr, n, 16, C.byref(rp)))
                put(f"lerf_render_rows 8x5 chunk16 32+{ni} lanes{lanes}", lib.nrf_lerf_render_rows_workspace_bytes(lr, C.byref(view(8, 5, 16, 0)), C.byref(rp)))
            L.check(lib.nrf_lerf_renderer_set_lanes(lr, 1))
    put("lerf_head_backward 3x32", lib.nrf_lerf_head_backward_workspace_bytes(lm, 3, 32))
    put("lerf_backward_points 3x32", lib.nrf_lerf_backward_points_workspace_bytes(lr, 3, 32))
    for prec in (0, 2):
        put(f"lerf_head_relevancy p37 prec{prec}", lib.nrf_lerf_head_relevancy_workspace_bytes(lm, 37, 3, prec))
        put(f"lerf_point_relevancy p37 slab7 prec{prec}", lib.nrf_lerf_point_relevancy_workspace_bytes(lr, 37, prec, 7))
        put(f"lerf_relevancy_grid 5x4x3 slab7 prec{prec}", lib.nrf_lerf_relevancy_grid_workspace_bytes(lr, 5, 4, 3, prec, 7))
    del small, lerf

    # ---- the bench shapes
    hs, cs, ls = S.make_hash_scene(mode="cu"), S.make_classic_scene(), S.make_lerf_scene()
    rp = params(64, 128, L.NRF_PREC_F16_SPLIT)
    for name, sc in (("hash", hs), ("classic", cs)):
        r = sc["renderer"]._r
        for lanes in (1, 2):
            L.check(lib.nrf_renderer_set_lanes(r, lanes))
            put(f"bench {name} frame render_rows 800x800 64+128 chunk65536 f16x3 lanes{lanes}", lib.nrf_render_rows_workspace_bytes(r, C.byref(view(800, 800, 65536)), C.byref(rp)))
            put(f"bench {name} frame batchify_rays n640000 64+128 chunk65536 f16x3 lanes{lanes}", lib.nrf_batchify_rays_workspace_bytes(r, 640000, 65536, C.byref(rp)))
        L.check(lib.nrf_renderer_set_lanes(r, 0))
        put(f"bench {name} chunk render_rays n65536 64+128 f16x3", lib.nrf_render_rays_workspace_bytes(r, 65536, C.byref(rp)))
        put(f"bench {name} chunk render_rays n65536 64+128 f32 (re-render)", lib.nrf_render_rays_workspace_bytes(r, 65536, C.byref(params(64, 128, L.NRF_PREC_F32))))
    lrp = L.RenderParams(64, 128, 0, 0, ls["renderer"].precision, R.ATEN_SUM_VEC)
    put("bench lerf frame render_rows 800x800 64+128 chunk32768", lib.nrf_lerf_render_rows_workspace_bytes(ls["renderer"]._r, C.byref(view(800, 800, 32768, 0)), C.byref(lrp)))
    put("bench train hash: batchify_rays n16384 64+128 f16x3", lib.nrf_batchify_rays_workspace_bytes(hs["renderer"]._r, 16384, 16384, C.byref(rp)))
    put("bench train hash: mlp_backward_f16 p16384x192", lib.nrf_mlp_backward_f16_workspace_bytes(hs["mlp"]._m, 16384 * 192))
    put("bench train hash: mlp_backward p16384x192", lib.nrf_mlp_backward_workspace_bytes(hs["mlp"]._m, 16384 * 192))
    put("bench train hash: hash_backward_binned n16384 s192", lib.nrf_hash_backward_binned_workspace_bytes_for(hs["embedder"]._h, 16384, 192))
    put("bench train classic: batchify_rays n4096 64+128 f16x3", lib.nrf_batchify_rays_workspace_bytes(cs["renderer"]._r, 4096, 4096, C.byref(rp)))
    put("bench train classic: mlp_backward p4096x192", lib.nrf_mlp_backward_workspace_bytes(cs["mlp"]._m, 4096 * 192))
    put("bench train lerf: lerf_batchify_rays n16384 64+128 chunk32768", lib.nrf_lerf_batchify_rays_workspace_bytes(ls["renderer"]._r, 16384, 32768, C.byref(lrp)))
    put("bench train lerf: lerf_backward_points n16384 s192", lib.nrf_lerf_backward_points_workspace_bytes(ls["renderer"]._r, 16384, 192))
    # ---- the mesh tools: pure functions of the shapes (a test-sized mesh, odd counts, and the isosurface of the tools' benches)
    for nv, nf, side in ((0, 0, 2), (37, 61, 9), (5_000_000, 10_000_000, 256)):
        put(f"raster v{nv} f{nf} {side}x{side + 1}", lib.nrf_raster_workspace_bytes(nv, nf, side, side + 1))
        put(f"mesh_voxelize v{nv} f{nf} {side}x{side + 1}x{side + 2}", lib.nrf_mesh_voxelize_workspace_bytes(nv, nf, side, side + 1, side + 2))
        put(f"nearest_points q{nf} t{nv} {side}^3", lib.nrf_nearest_points_workspace_bytes(nf, nv, side, side, side))
        put(f"face_grid f{nf} {side}^3", lib.nrf_face_grid_workspace_bytes(nf, side, side, side))
        put(f"face_grid_bytes f{nf} {side}^3 refs{3 * nf} large{nf // 7}", lib.nrf_face_grid_bytes(nf, side, side, side, 3 * nf, nf // 7))
        put(f"closest_on_mesh q{nf}", lib.nrf_closest_on_mesh_workspace_bytes(nf))
        put(f"ray_cast n{nf}", lib.nrf_ray_cast_workspace_bytes(nf))
    for name, nbytes in rows:
        print(f"{name}\t{nbytes}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
