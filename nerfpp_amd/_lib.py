"""ctypes loader for libnerfpp_hip.so (the C ABI declared in include/nerfpp_hip.h).

The library is built in-tree by `__graft_entry__.build()` / `make -C nerfpp_amd/csrc`.  There is no CPU
fallback: if the shared object is missing, importing the compute API raises.
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NRF_LIB_PATH") or os.path.join(_HERE, "lib", "libnerfpp_hip.so")   # NRF_LIB_PATH: tuning builds only

NRF_OK = 0
NRF_HASH_NGP, NRF_HASH_CU = 0, 1
NRF_SH_LIBTORCH, NRF_SH_CUDA = 0, 1
NRF_PREC_F32, NRF_PREC_F16_MFMA, NRF_PREC_F16_SPLIT = 0, 1, 2
NRF_DIRS_NONE, NRF_DIRS_PE, NRF_DIRS_SH_LIBTORCH, NRF_DIRS_SH_CUDA = 0, 1, 2, 3
(NRF_RNG_T_RAND, NRF_RNG_R_COARSE, NRF_RNG_THETA_COARSE, NRF_RNG_NOISE_COARSE, NRF_RNG_U_PDF, NRF_RNG_PRECOND, NRF_RNG_R_FINE, NRF_RNG_THETA_FINE,
 NRF_RNG_NOISE_FINE) = range(1, 10)       # include/nrf_rng.h
NRF_RNG_SURFACE_COUNT, NRF_RNG_SURFACE_UV = 10, 11
NRF_RNG_HEMI_DIR = 12
NRF_RC_CLOSEST, NRF_RC_ANY = 0, 1          # nrf_ray_cast_mesh: mode
NRF_RC_CULL_NONE, NRF_RC_CULL_BACK, NRF_RC_CULL_FRONT = 0, 1, 2
NRF_VOX_NONZERO, NRF_VOX_POSITIVE, NRF_VOX_ODD = 0, 1, 2          # nrf_mesh_voxelize: rule
NRF_ALIGN_POINT, NRF_ALIGN_PLANE = 0, 1          # nrf_align_sums / nrf_align_solve: mode
NRF_PROF_NAMES = ("hash", "mlp", "composite", "sample", "other", "sigma", "mlp_colour")
NRF_COARSE_AUTO, NRF_COARSE_FULL, NRF_COARSE_SIGMA_F32 = 0, 1, 2
NRF_OVERFLOW_AUTO, NRF_OVERFLOW_RERENDER, NRF_OVERFLOW_ERROR, NRF_OVERFLOW_DEFERRED, NRF_OVERFLOW_IGNORE = 0, 1, 2, 3, 4
NRF_ERR_NONFINITE = 5
NRF_NORMALS_DENSITY, NRF_NORMALS_PREDICTED = 1, 2          # nrf_render_normals.bits


class HashDesc(C.Structure):
    _fields_ = [("mode", C.c_int), ("n_levels", C.c_int), ("n_features", C.c_int), ("log2_hashmap_size", C.c_int),
                ("base_resolution", C.c_int), ("finest_resolution", C.c_int), ("bbox", C.c_float * 6)]


class MlpSmallDesc(C.Structure):
    _fields_ = [("input_ch", C.c_int), ("input_ch_views", C.c_int), ("num_layers", C.c_int), ("hidden_dim", C.c_int),
                ("geo_feat_dim", C.c_int), ("num_layers_color", C.c_int), ("hidden_dim_color", C.c_int),
                ("use_pred_normal", C.c_int), ("num_layers_normals", C.c_int), ("hidden_dim_normals", C.c_int)]


class MlpNerfDesc(C.Structure):
    _fields_ = [("depth", C.c_int), ("width", C.c_int), ("input_ch", C.c_int), ("input_ch_views", C.c_int),
                ("output_ch", C.c_int), ("skip", C.c_int), ("use_viewdirs", C.c_int)]


class RendererDesc(C.Structure):
    _fields_ = [("hash", C.c_void_p), ("pe_freqs", C.c_int), ("dirs_encoder", C.c_int), ("dirs_param", C.c_int), ("mlp", C.c_void_p)]


class RenderParams(C.Structure):
    _fields_ = [("n_samples", C.c_int), ("n_importance", C.c_int), ("lindisp", C.c_int), ("white_bkgr", C.c_int),
                ("precision", C.c_int), ("sum_vec", C.c_int),
                ("perturb", C.c_float), ("has_cone", C.c_int), ("cone_angle", C.c_float), ("raw_noise_std", C.c_float), ("precond_alpha", C.c_float),
                ("has_bbox", C.c_int), ("bbox", C.c_float * 6), ("seed", C.c_uint64), ("ray_base", C.c_int64), ("coarse_mode", C.c_int), ("overflow_policy", C.c_int)]


class RenderOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("d_rgb", "d_disp", "d_acc", "d_depth", "d_weights", "d_raw",
                                          "d_z_coarse", "d_raw_coarse", "d_weights_coarse", "d_z_fine")]


class RenderNormals(C.Structure):          # nrf_render_normals: beside RenderParams / RenderOutputs in the *_normals entries
    _fields_ = [("bits", C.c_int), ("d_normals", C.c_void_p), ("d_pred_normals", C.c_void_p)]


class LerfRendererDesc(C.Structure):
    _fields_ = [("lang_embed", C.c_void_p), ("lerf", C.c_void_p)]


class LerfOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("d_embedding", "d_disp", "d_acc", "d_depth", "d_weights", "d_relevancy", "d_z_coarse", "d_weights_coarse", "d_z_fine")]


class View(C.Structure):          # nrf_view
    _fields_ = [("h", C.c_int), ("w", C.c_int), ("K", C.c_float * 9), ("c2w", C.c_float * 12), ("has_staticcam", C.c_int), ("c2w_staticcam", C.c_float * 12),
                ("row0", C.c_int), ("rows", C.c_int), ("use_viewdirs", C.c_int), ("ndc", C.c_int), ("chunk", C.c_int), ("bbox", C.c_float * 6)]


# The C ABI: one line per NRF_API function of include/nerfpp_hip.h, in the header's order, as name(argument kinds)->return kind.
# Kinds: i int, l int64_t, z size_t, f float, d double, u uint32_t, q uint64_t, p any pointer (data, handle, struct, out-parameter,
# pointer array, stream); returns also s const char * and v void, and no arrow means the int status.  lib() turns each line into
# argtypes / restype, so call sites pass plain Python values; tests/test_host_cpu.py holds every line to the header.
_KINDS = {"i": C.c_int, "l": C.c_int64, "z": C.c_size_t, "f": C.c_float, "d": C.c_double, "u": C.c_uint32, "q": C.c_uint64, "p": C.c_void_p,
          "s": C.c_char_p, "v": None}
_ABI = """
    nrf_version()
    nrf_last_error()->s
    nrf_status_string(i)->s
    nrf_get_rays(iippiipppp)
    nrf_ndc_rays(iiffpplppp)
    nrf_precrop_bounds(iiiifp)
    nrf_rand_pixels(qliiiilppp)
    nrf_rand_patches(qliiiilippp)
    nrf_ray_batch(pppplpppp)
    nrf_gather_pixels(piiipplpp)
    nrf_aabb(ppplfppp)
    nrf_pack_rays(ppplipp)
    nrf_pack_rays_viewsrc(pppplpp)
    nrf_view_rays(pppp)
    nrf_near_far_range(plippp)
    nrf_near_far_range_device(plipp)
    nrf_linspace(ffip)
    nrf_z_vals(pilpiipp)
    nrf_points(piplipp)
    nrf_pe_encode(plipp)
    nrf_sh_encode(pliipp)
    nrf_hash_create(pp)
    nrf_hash_destroy(p)->v
    nrf_hash_output_dims(p)
    nrf_hash_table_elems(p)->l
    nrf_hash_set_table(ppip)
    nrf_hash_set_primes(ppp)
    nrf_hash_set_dense_budget(plp)
    nrf_hash_get_dense_budget(p)->l
    nrf_hash_memory_bytes(ppp)
    nrf_hash_get_level_scales(pp)
    nrf_hash_set_level_scales(ppp)
    nrf_hash_encode(pplppp)
    nrf_hash_encode_lm_f16(pplppp)
    nrf_hash_encode_lm_f16_strided(pplplpp)
    nrf_mlp_small_param_count(p)->l
    nrf_mlp_nerf_param_count(p)->l
    nrf_mlp_lerf_param_count(p)->l
    nrf_mlp_lerf_create(ppipp)
    nrf_mlp_small_create(ppipp)
    nrf_mlp_nerf_create(ppipp)
    nrf_mlp_destroy(p)->v
    nrf_mlp_output_dims(p)
    nrf_mlp_forward(pplipp)
    nrf_raw2outputs(pppiliiipppppp)
    nrf_raw2weights(piippilippppp)
    nrf_raw2weights_gather(piipppilippppp)
    nrf_lerf_mfma_available(p)
    nrf_lerf_set_precision(pi)
    nrf_lerf_sigma(ppplpp)
    nrf_lerf_render_embedding(ppplipp)
    nrf_lerf_sigma_lm(ppplpp)
    nrf_lerf_render_embedding_lm(ppplipp)
    nrf_lerf_sigma_lm_strided(pplplpp)
    nrf_lerf_geo_bytes(l)->z
    nrf_lerf_sigma_geo_lm_strided(pplplpplp)
    nrf_lerf_sigma_exact_available(p)
    nrf_lerf_sigma_exact_lm_strided(pplplpplp)
    nrf_lerf_render_embedding_lm_geo(pplpplplipp)
    nrf_lerf_render_embedding_lm_gather(pplpplipp)
    nrf_render_clip_embedding(piiplipp)
    nrf_lerf_relevancy(plipipiipp)
    nrf_relevancy_image(plipp)
    nrf_colormap_jet_u8(plpp)
    nrf_colormap_jet_lut(p)
    nrf_pyramid_level_geometry(iiifip)
    nrf_pyramid_max_zoom_out(piip)
    nrf_pyramid_create(iifiipp)
    nrf_pyramid_destroy(p)
    nrf_pyramid_memory_bytes(p)->l
    nrf_pyramid_set_entries(plppip)
    nrf_pyramid_pixel_values(pifpplplp)
    nrf_pyramid_relevancy_preview_workspace_bytes(pii)->z
    nrf_pyramid_relevancy_preview(pifpipiipppzp)
    nrf_sample_pdf(pplipiippp)
    nrf_fine_depths(pplipiipp)
    nrf_fine_depths_merge(pplipiipppp)
    nrf_rng_fill(quqlipp)
    nrf_jitter_z(pplipp)
    nrf_tangent_scatter(ppiplifppppp)
    nrf_precondition(ppfplpp)
    nrf_raw2outputs_noise(pppiliiipfpppppp)
    nrf_sample_pdf_rand(pplipiippp)
    nrf_fine_depths_rand(pplipiipp)
    nrf_renderer_create(pp)
    nrf_renderer_destroy(p)->v
    nrf_renderer_last_features(pppppppp)
    nrf_renderer_nonfinite(ppp)
    nrf_run_network_workspace_bytes(pli)->z
    nrf_run_network(pppliippzp)
    nrf_density_grid_workspace_bytes(piiil)->z
    nrf_density_grid(ppiiiplpzp)
    nrf_isosurface_workspace_bytes(iii)->z
    nrf_isosurface_count(piiipfppppzp)
    nrf_isosurface_emit(piiipfpppllpzp)
    nrf_mesh_components_workspace_bytes(ll)->z
    nrf_mesh_components(pllpppzp)
    nrf_lattice_components_workspace_bytes(iii)->z
    nrf_lattice_components(piiiipppzp)
    nrf_tsdf_integrate(pppiiippifffip)
    nrf_tsdf_observed(piiipplpp)
    nrf_tsdf_sample_color(piiipplpp)
    nrf_raster_workspace_bytes(llii)->z
    nrf_raster_mesh(plplpiiippfippppppzp)
    nrf_mesh_sample_workspace_bytes(ll)->z
    nrf_mesh_sample_count(plplfqppppzp)
    nrf_mesh_sample_emit(plplqlppppzp)
    nrf_nearest_points_workspace_bytes(lliii)->z
    nrf_nearest_points(plplpiiifppppzp)
    nrf_distance_stats_workspace_bytes(l)->z
    nrf_distance_stats(plpippzp)
    nrf_mesh_simplify_workspace_bytes(lliii)->z
    nrf_mesh_simplify_count(plplpiiippppzp)
    nrf_mesh_simplify_emit(plplpiiiillppppppzp)
    nrf_ssim_window(p)
    nrf_ssim_workspace_bytes(iiii)->z
    nrf_ssim(ppiiiidpppzp)
    nrf_image_mse_workspace_bytes(il)->z
    nrf_image_mse(ppilppzp)
    nrf_ms_ssim_workspace_bytes(iiiii)->z
    nrf_ms_ssim(ppiiiidippzp)
    nrf_ssim_loss_workspace_bytes(iiii)->z
    nrf_ssim_loss(ppiiiiddppppzp)
    nrf_atlas_dims(lipp)
    nrf_atlas_texels(plplpifiippppp)
    nrf_texture_sample(pliipplipp)
    nrf_texture_shade(plplppiipppiiipp)
    nrf_mesh_adjacency_workspace_bytes(ll)->z
    nrf_mesh_adjacency_count(pllpppzp)
    nrf_mesh_adjacency_emit(pllllppppppppzp)
    nrf_mesh_smooth(pppliiffipppplp)
    nrf_mesh_vertex_normals(plplpplipp)
    nrf_density_grad_workspace_bytes(pl)->z
    nrf_density_grad(pplpppzp)
    nrf_face_grid_workspace_bytes(liii)->z
    nrf_face_grid_bytes(liiill)->z
    nrf_face_grid_count(plplpiiippppzp)
    nrf_face_grid_build(plplpiiillpzpzp)
    nrf_closest_on_mesh_workspace_bytes(l)->z
    nrf_closest_on_mesh(plplplpiiillpzfppppppzp)
    nrf_ray_cast_workspace_bytes(l)->z
    nrf_ray_cast_mesh(pliplplpiiillpziipppppppzp)
    nrf_hemisphere_dirs(pliqlppp)
    nrf_mesh_ambient_occlusion(ppliffqlplplpiiillpzpppzp)
    nrf_mesh_voxelize_workspace_bytes(lliii)->z
    nrf_mesh_voxelize(plplpiiifipppppzp)
    nrf_align_state_init(ppp)
    nrf_align_apply(plpipp)
    nrf_align_workspace_bytes(li)->z
    nrf_align_sums(pppliplplppzp)
    nrf_align_solve(liiiipppzp)
    nrf_sort_workspace_bytes(l)->z
    nrf_sort_pairs_u32(ppliipppzp)
    nrf_mesh_bvh_bytes(l)->z
    nrf_mesh_bvh_workspace_bytes(l)->z
    nrf_mesh_bvh_build(plplpzppzp)
    nrf_bvh_query_workspace_bytes(l)->z
    nrf_bvh_closest_on_mesh(plplplpzpfppppppzp)
    nrf_bvh_ray_cast_mesh(pliplplpzpiipppppppzp)
    nrf_bvh_point_codes(plipzlpp)
    nrf_point_bvh_bytes(l)->z
    nrf_point_bvh_workspace_bytes(l)->z
    nrf_point_bvh_build(plpzppzp)
    nrf_point_bvh_codes(plipzlpp)
    nrf_bvh_knn(plplpzpifipppppzp)
    nrf_points_normals(plpipipppp)
    nrf_knn_mean_distance(plipp)
    nrf_value_stats_workspace_bytes(l)->z
    nrf_value_stats(plppzp)
    nrf_align_sums_normals(pppplppzp)
    nrf_render_rays_workspace_bytes(plp)->z
    nrf_render_rays(ppilpppppzp)
    nrf_batchify_rays_workspace_bytes(plip)->z
    nrf_batchify_rays(ppilipppppzp)
    nrf_render_rows_workspace_bytes(ppp)->z
    nrf_render_rows(pppppppppzp)
    nrf_render_rays_normals_workspace_bytes(plpi)->z
    nrf_render_rays_normals(ppilppppppzp)
    nrf_batchify_rays_normals_workspace_bytes(plipi)->z
    nrf_batchify_rays_normals(ppilippppppzp)
    nrf_render_rows_normals_workspace_bytes(pppi)->z
    nrf_render_rows_normals(ppppppppppzp)
    nrf_huber_loss(pplppp)
    nrf_raw2outputs_backward(pppiliiippp)
    nrf_raw2outputs_backward_noise(pppiliiipfppp)
    nrf_mask_sigma_grad(plipp)
    nrf_mlp_backward_workspace_bytes(pl)->z
    nrf_mlp_backward(ppplpppzp)
    nrf_normal_losses_workspace_bytes(li)->z
    nrf_normal_losses(pppipiliffpppzp)
    nrf_ray_regularizers_workspace_bytes(li)->z
    nrf_ray_regularizers(pppiliipfffppppzp)
    nrf_mlp_backward_pn_workspace_bytes(pl)->z
    nrf_mlp_backward_pn(ppplpppzp)
    nrf_mlp_backward_f16_workspace_bytes(pl)->z
    nrf_mlp_backward_f16(ppplpppzp)
    nrf_mlp_backward_f16_lm(pppiplpppzp)
    nrf_mlp_backward_f16_lm_src(pplppiplpppzp)
    nrf_mask_sigma_grad_src(pplipp)
    nrf_mlp_backward_f16_flags(ppp)
    nrf_mlp_backward_f16_flags_async(ppp)
    nrf_mlp_backward_f16_flags_device(p)->p
    nrf_mlp_set_params(ppip)
    nrf_mlp_device_repack_images(p)
    nrf_mlp_set_input_rms_hint(pfp)
    nrf_mlp_set_split_scaling(pip)
    nrf_mlp_get_split_scales(pppp)
    nrf_hash_backward(pplppp)
    nrf_hash_backward_rays(pplippp)
    nrf_hash_backward_packed_workspace_bytes(p)->z
    nrf_hash_backward_rays_packed(pplipppzp)
    nrf_hash_backward_binned_workspace_bytes(pi)->z
    nrf_hash_backward_binned_workspace_bytes_for(pli)->z
    nrf_hash_backward_rays_binned(pplipppzp)
    nrf_hash_tv_loss(ppipifppp)
    nrf_adam_step(pppplffffip)
    nrf_adam_step_guarded(pppplffffipip)
    nrf_normalize_depth(plffpp)
    nrf_to_u8(plpp)
    nrf_render_view_dims(iipfppp)
    nrf_tile_partition(iiipp)
    nrf_comm_unique_id(p)
    nrf_comm_create(piip)
    nrf_comm_create_timeout(piidp)
    nrf_comm_wrap(pp)
    nrf_comm_destroy(p)->v
    nrf_comm_world(p)
    nrf_comm_rank(p)
    nrf_allgather_tiles(ppiiiipp)
    nrf_allreduce_grads(pppilipp)
    nrf_lerf_renderer_create(pp)
    nrf_lerf_renderer_destroy(p)->v
    nrf_lerf_renderer_nonfinite(pp)
    nrf_lerf_renderer_set_lanes(pi)
    nrf_lerf_set_prompts(ppipiip)
    nrf_lerf_render_rays_workspace_bytes(plp)->z
    nrf_lerf_render_rays(ppilpppppzp)
    nrf_lerf_batchify_rays_workspace_bytes(plip)->z
    nrf_lerf_batchify_rays(ppilipppppzp)
    nrf_lerf_render_rows_workspace_bytes(ppp)->z
    nrf_lerf_render_rows(pppppppppzp)
    nrf_lerf_head_relevancy_workspace_bytes(plii)->z
    nrf_lerf_head_relevancy(pplpipiiipppzp)
    nrf_lerf_point_relevancy_workspace_bytes(plil)->z
    nrf_lerf_point_relevancy(ppliipplpzp)
    nrf_lerf_relevancy_grid_workspace_bytes(piiiil)->z
    nrf_lerf_relevancy_grid(ppiiiiipplpzp)
    nrf_huber_rows_nanmean(pplifppp)
    nrf_lerf_head_backward_workspace_bytes(pli)->z
    nrf_lerf_head_backward(pppppilipfppppppzp)
    nrf_lerf_backward_points_workspace_bytes(pli)->z
    nrf_lerf_backward_points(ppppilipfppppzp)
    nrf_lerf_renderer_last_features(pppppppp)
    nrf_lerf_backward_points_src(pplpppppilipfppppzp)
    nrf_scratch_trim()->z
    nrf_device_bytes_in_use()->l
    nrf_set_render_lanes(i)
    nrf_get_render_lanes()
    nrf_set_live_colour(i)
    nrf_get_live_colour()
    nrf_live_points_workspace_bytes(l)->z
    nrf_live_points(plppppzp)
    nrf_set_fused_resample(i)
    nrf_get_fused_resample()
    nrf_dbg_resample(pppiliplqliippppppppp)
    nrf_renderer_set_lanes(pi)
    nrf_fp32_gemm_available()
    nrf_get_train_gemm()
    nrf_set_train_gemm(i)
    nrf_gemm_nt_bf16x3(pilipiipipip)
    nrf_gemm_tn_bf16x3(piipiilpiip)
    nrf_layer_grad_split(piipiilpiipp)
    nrf_gemm_nt_f16x3(pilipiipipip)
    nrf_profile_enable(i)
    nrf_profile_is_enabled()
    nrf_profile_read(ppi)
"""
SIGNATURES = {}          # name -> (return kind, argument kinds); a line that is not an entry stops the import, naming itself
for _entry in _ABI.split():
    _m = re.fullmatch(r"(nrf_\w+)\(([ilzfduqp]*)\)(?:->([lzpsv]))?", _entry)
    if _m is None or _m[1] in SIGNATURES:
        raise ValueError(f"nerfpp_amd._lib: malformed or repeated signature entry {_entry!r}")
    SIGNATURES[_m[1]] = (_m[3] or "i", _m[2])
SYMBOLS = list(SIGNATURES)
NRF_COMM_ID_BYTES = 128

_lib = None


class NrfError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NrfError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback for the HIP path)")
        L = C.CDLL(LIB_PATH)
        for name, (ret, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = _KINDS[ret]
            fn.argtypes = [_KINDS[k] for k in args]
        _lib = L
    return _lib


def check(status):
    if status != NRF_OK:
        L = lib()
        raise NrfError(f"{L.nrf_status_string(status).decode()}: {L.nrf_last_error().decode()}")
