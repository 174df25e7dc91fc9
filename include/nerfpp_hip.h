/*
 * nerfpp_hip.h -- C ABI of the MI355X-native (gfx950) NeRF / HashNeRF volume-rendering path.
 *
 * The reference (DeliriumV01D/NeRFpp) has no C ABI: its hot path sits behind C++ templates and
 * virtuals (BaseEmbedderImpl, BaseNeRFImpl, NeRFRenderer<...>).  This header is the boundary a
 * host binds instead: `extern "C"`, plain pointers and sizes, no torch types.  Each entry point
 * cites the reference interface it replaces (paths relative to the reference's src/).  The
 * LibTorch adapter classes (include/nerfpp_torch.h) and the Python mirror (nerfpp_amd/) are thin
 * callers of exactly these functions.
 *
 * Conventions
 *   - every `d_` pointer is DEVICE memory (hipMalloc / a torch tensor's data_ptr on the same GPU),
 *     fp32 row-major unless stated; every other pointer is HOST memory read during the call;
 *   - every launch goes to the caller's stream (`void *stream` is a hipStream_t; NULL = the
 *     per-process default stream).  No call synchronises the device, allocates device memory
 *     (handles own theirs; scratch comes from the caller through *_workspace_bytes) or throws;
 *   - return value: NRF_OK or an NRF_ERR_* code; nrf_last_error() gives the text (thread-local);
 *   - the caller owns all buffers; handles are created/destroyed explicitly and are immutable
 *     during a call (re-entrant: no per-call state is kept on a handle, unlike
 *     CuHashEmbedderImpl::QueryPoints, CuHashEmbedder.h:26-27).
 *   - there is NO CPU fallback: without a gfx950 device every compute entry returns NRF_ERR_HIP.
 */
#ifndef NERFPP_HIP_H
#define NERFPP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NRF_API __attribute__((visibility("default")))

enum {
    NRF_OK = 0,
    NRF_ERR_INVALID_ARG = 1,
    NRF_ERR_HIP = 2,          /* a HIP runtime call / kernel launch failed (no device, OOM, ...) */
    NRF_ERR_UNSUPPORTED = 3,  /* valid in the reference, not built here (message says what) */
    NRF_ERR_WORKSPACE = 4,    /* caller's workspace too small */
    NRF_ERR_NONFINITE = 5     /* non-finite values where finite ones are required: a matrix-core render produced inf / NaN network outputs (an fp16 operand left its
                                 range, see nrf_render_params.overflow_policy), or a lattice handed to nrf_isosurface_emit holds inf / NaN */
};

NRF_API int nrf_version(void);
NRF_API const char *nrf_last_error(void);
NRF_API const char *nrf_status_string(int status);

/* ---------------------------------------------------------------------------------------------
 * Rays                                                         RayUtils.h
 * ------------------------------------------------------------------------------------------- */

/* GetDirections + GetRays (RayUtils.h:5-46) for image rows [row0, row0+rows) of an h x w image.
 * K: host [9] row-major 3x3, c2w: host [12] row-major 3x4.  d_o, d_d: [rows*w, 3].
 * Ray r = (y-row0)*w + x (row-major, y outer) -- the reference's pixel<->ray mapping.
 * cone_angle (host, optional) receives ((1/fx + 1/fy)/2)*1.1 (RayUtils.h:35-43). */
NRF_API int nrf_get_rays(int h, int w, const float *K, const float *c2w, int row0, int rows,
                         float *d_o, float *d_d, float *cone_angle, void *stream);

/* NDCRays (RayUtils.h:49-83); in place allowed. */
NRF_API int nrf_ndc_rays(int h, int w, float focal, float near_plane, const float *d_o, const float *d_d, int64_t n,
                         float *d_o_out, float *d_d_out, void *stream);

/* ---- ray-batch producer of the training loop: NeRFDataset::get_batch / GetRayBatch (NeRFDataset.cpp:109-208), SURVEY 8f row N2 ----
 * nrf_precrop_bounds : CalculateBounds (:44-65), host only; out = {h_start, h_end, w_start, w_end}, inclusive.
 * nrf_rand_pixels    : the batch's pixel coordinates (:154-155 draws torch::randint): counter-based, element k of iteration `iter` is
 *                      lo + floor(u32(seed, stream, iter*n + k) * range / 2^32), streams 16 (rows) / 17 (columns) of include/nrf_rng.h.
 * nrf_rand_patches   : n_patches square patches of patch x patch pixels inside the same (inclusive) crop, for losses over neighbourhoods (nrf_ssim_loss): patch k's
 *                      origin row is h_start + floor(u32(seed, 19, iter*n_patches + k) * (h_end - h_start - patch + 2) / 2^32), its column the same with stream 20 and
 *                      the w bounds; element k*patch*patch + i*patch + j is pixel (oy + i, ox + j).  d_rand_h / d_rand_w [n_patches * patch * patch] feed nrf_ray_batch /
 *                      nrf_gather_pixels unchanged.  patch < 1, patch > 4096 or a crop smaller than the patch: NRF_ERR_INVALID_ARG, nothing launched.
 * nrf_ray_batch      : GetRayBatch (:109-145): rays through pixels (rand_h[k], rand_w[k]); cone_angle = (1/fx + 1/fy)/2 to host.
 * nrf_gather_pixels  : target_s = CurrentImage.index({rand_h, rand_w}) (:156); image [h, w, c] fp32 on the device. */
NRF_API int nrf_precrop_bounds(int h, int w, int iter, int precrop_iters, float precrop_frac, int *out);
NRF_API int nrf_rand_pixels(uint64_t seed, int64_t iter, int h_start, int h_end, int w_start, int w_end, int64_t n, int64_t *d_rand_h,
                            int64_t *d_rand_w, void *stream);
NRF_API int nrf_rand_patches(uint64_t seed, int64_t iter, int h_start, int h_end, int w_start, int w_end, int64_t n_patches, int patch, int64_t *d_rand_h,
                             int64_t *d_rand_w, void *stream);
NRF_API int nrf_ray_batch(const float *K, const float *c2w, const int64_t *d_rand_h, const int64_t *d_rand_w, int64_t n, float *d_o, float *d_d,
                          float *cone_angle, void *stream);
NRF_API int nrf_gather_pixels(const float *d_image, int h, int w, int c, const int64_t *d_rand_h, const int64_t *d_rand_w, int64_t n, float *d_out,
                              void *stream);

/* IntersectWithAABB (RayUtils.h:87-126). bbox: host [6] = min xyz, max xyz. */
NRF_API int nrf_aabb(const float *d_o, const float *d_d, const float *bbox, int64_t n, float near_plane,
                     float *d_near, float *d_far, void *stream);

/* The ray-batch assembly of NeRFRenderer::Render (NeRFRenderer.h:549-583):
 * viewdirs = d/||d||, near/far from the AABB, rays = cat[o, d, near, far, (viewdirs)].
 * d_rays: [n, 11] when use_viewdirs else [n, 8]. */
NRF_API int nrf_pack_rays(const float *d_o, const float *d_d, const float *bbox, int64_t n, int use_viewdirs,
                          float *d_rays, void *stream);

/* ... with the view directions taken from d_view_src [n,3] instead of d_d: Render() normalises rays_d into viewdirs BEFORE the NDC warp replaces
 * rays_o / rays_d (NeRFRenderer.h:549-568), so an Ndc + UseViewdirs batch packs the warped o, d with the un-warped directions.  d_rays: [n, 11]. */
NRF_API int nrf_pack_rays_viewsrc(const float *d_o, const float *d_d, const float *d_view_src, const float *bbox, int64_t n, float *d_rays, void *stream);

/* The pose branch of NeRFRenderer::Render (NeRFRenderer.h:541-583) for the row tile [row0, row0 + rows) of an h x w frame, as ONE kernel:
 * GetRays(h, w, K, c2w) -> view directions d/||d|| (from c2w's rays, before c2w_staticcam replaces the camera, :549-561, and before the NDC warp) ->
 * NDCRays(h, w, K[0], 1.f) when `ndc` (:563-568) -> IntersectWithAABB -> rays_ = cat[o, d, near, far, (viewdirs)].  Zero-initialise the struct.
 * `chunk` is BatchifyRays' Chunk (used by nrf_render_rows; results do not depend on it). */
typedef struct nrf_view {
    int h, w;                 /* frame size (after any RenderFactor, nrf_render_view_dims) */
    float K[9];               /* row-major 3x3 */
    float c2w[12];            /* row-major 3x4 */
    int has_staticcam;        /* c2w_staticcam given (honoured only with use_viewdirs, as in the reference) */
    float c2w_staticcam[12];
    int row0, rows;           /* the tile; ray r of the tile is pixel (row0 + r / w, r % w) */
    int use_viewdirs;         /* UseViewdirs: ray stride 11, else 8 */
    int ndc;                  /* Ndc */
    int chunk;                /* Chunk */
    float bbox[6];            /* BoundingBox: min xyz, max xyz */
} nrf_view;
/* d_rays: [rows*w, 8|11].  d_near_far (optional): DEVICE [2] floats receiving min(near), max(far) of the tile (NeRFRenderer.h:602-603) --
 * written on `stream`, no host synchronisation (the reference's two .item() calls stall the host once per frame). */
NRF_API int nrf_view_rays(const nrf_view *v, float *d_rays, float *d_near_far, void *stream);

/* min(near), max(far) over a packed ray batch (NeRFRenderer.h:602-603); results to host, synchronises `stream`. */
NRF_API int nrf_near_far_range(const float *d_rays, int64_t n, int ray_stride, float *near_min, float *far_max, void *stream);
/* ... the same into DEVICE memory (d_near_far [2] floats), in stream order, nothing waits: what a training loop wants (the reference's two .item() calls of
 * NeRFRenderer.h:602-603 stall its host once per rendered batch; the values are only read when a frame is post-processed). */
NRF_API int nrf_near_far_range_device(const float *d_rays, int64_t n, int ray_stride, float *d_near_far, void *stream);

/* torch::linspace(start, end, steps) as ATen's CPU kernel rounds it (one fused rounding per
 * element) -- for hosts without torch; the LibTorch / PyTorch callers pass torch::linspace itself. */
NRF_API int nrf_linspace(float start, float end, int steps, float *out_host);

/* z_vals (NeRFRenderer.h:393-402) and sample points pts = o + d*z (:419). d_t: [s] = linspace(0,1,s). */
NRF_API int nrf_z_vals(const float *d_rays, int ray_stride, int64_t n, const float *d_t, int s, int lindisp,
                       float *d_z, void *stream);
NRF_API int nrf_points(const float *d_rays, int ray_stride, const float *d_z, int64_t n, int s, float *d_pts, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Encoders                                                     BaseEmbedder.h:6-15 (plugin iface)
 * ------------------------------------------------------------------------------------------- */

/* EmbedderImpl::forward, sinusoidal PE (NeRF.cpp:4-39): [p,3] -> [p, 3+6*nfreq]. */
NRF_API int nrf_pe_encode(const float *d_x, int64_t p, int nfreq, float *d_out, void *stream);

/* Spherical harmonics: variant 0 = SHEncoderImpl (NeRF.cpp:131-201, degree 1..5),
 *                      variant 1 = CuSHEncoderImpl / CuSHKernel (CuSHEncoder.cu:4-118, degree 1..8).
 * [p,3] -> [p, degree^2]. */
enum { NRF_SH_LIBTORCH = 0, NRF_SH_CUDA = 1 };
NRF_API int nrf_sh_encode(const float *d_dirs, int64_t p, int degree, int variant, float *d_out, void *stream);

/* Multiresolution hash grid.
 *   NRF_HASH_NGP : HashEmbedderImpl  (NeRF.cpp:208-318)  fp32 table [L][2^T][F], int64 hash with the
 *                  Instant-NGP primes, floor()ed per-level resolution.
 *   NRF_HASH_CU  : CuHashEmbedderImpl (CuHashEmbedder.cpp:85-103 + CuHashEmbedder.cu:8-102) fp16 table
 *                  [L*2^T, F] (cast ONCE at upload, not per forward as .cu:257 does), uint32 hash with
 *                  per-level primes, un-floored scale, the level-offset overlap quirk (.cu:54),
 *                  blend in fp32 rounded once to fp16 (.cu:95). */
enum { NRF_HASH_NGP = 0, NRF_HASH_CU = 1 };

typedef struct nrf_hash_desc {
    int mode;                 /* NRF_HASH_NGP | NRF_HASH_CU */
    int n_levels;             /* L  (ctor arg n_levels, NeRFExecutor.h:430-432) */
    int n_features;           /* F  */
    int log2_hashmap_size;    /* T  */
    int base_resolution;
    int finest_resolution;
    float bbox[6];            /* min xyz, max xyz */
} nrf_hash_desc;

typedef struct nrf_hash nrf_hash;

NRF_API int nrf_hash_create(const nrf_hash_desc *desc, nrf_hash **out);
NRF_API void nrf_hash_destroy(nrf_hash *h);
NRF_API int nrf_hash_output_dims(const nrf_hash *h);              /* GetOutputDims() */
NRF_API int64_t nrf_hash_table_elems(const nrf_hash *h);          /* L * 2^T * F */

/* Upload the embedding table from an fp32 array in the reference's parameter layout
 * (NGP: embeddings_0..L-1 concatenated, each [2^T, F], NeRF.cpp:255-258;  CU: `embedder_embeddings`
 * [L*2^T, F], CuHashEmbedder.cpp:24).  `src` may be host or device memory (src_on_device).
 * STREAM ORDER: the upload, the fp32 -> fp16 cast of the CU mode and the re-bake of the dense image (see nrf_hash_set_dense_budget) are enqueued on `stream`
 * and NOT waited for (a training loop calls this every step) -- except when the dense image is (re)allocated, which completes before the call returns.  Encode /
 * render calls must therefore be issued on the SAME stream, or on one ordered behind it (an event recorded on `stream` after this call, or a synchronisation);
 * a render on an unrelated stream races with the cast and the bake.  (nrf_batchify_rays' lanes fork from the caller's stream and are ordered behind it.) */
NRF_API int nrf_hash_set_table(nrf_hash *h, const float *src, int src_on_device, void *stream);

/* NRF_HASH_CU only: per-level primes [L*3] (buffer `embedder_primes`, CuHashEmbedder.cpp:51-52) and
 * biases [L*3] (`embedder_biases`, :54-59; NULL = zeros).  Host pointers.  A zero or even multiplier is rejected (NRF_ERR_INVALID_ARG): the reference
 * only ever produces odd primes in [2^28, 2^30), and zeros -- an uninitialised buffer -- would hash every corner to row 0 without any error. */
NRF_API int nrf_hash_set_primes(nrf_hash *h, const int32_t *primes, const float *biases);

/* The renderer's fast path reads a DENSE image of the grid's coarse levels (every lattice vertex's table entries copied next to each other, baked from the
 * table at upload; outputs identical to the hashed lookup): `budget_bytes` of it are built, coarse to fine, default 24 GiB of the 288 GB (all 16 levels at
 * finest 512 take 4.4 GiB).  A training loop re-uploads the table every step and sets 0 (no bake); a renderer leaves the default.  Re-bakes immediately when a
 * table is present.  STREAM ORDER as nrf_hash_set_table: when the image is (re)allocated or released the call completes the bake / drains `stream` before it
 * returns; a re-bake into the existing image stays asynchronous on `stream`, and its readers must be ordered behind it there. */
NRF_API int nrf_hash_set_dense_budget(nrf_hash *h, int64_t budget_bytes, void *stream);
NRF_API int64_t nrf_hash_get_dense_budget(const nrf_hash *h);
/* Device memory the handle holds: the table in the mode's own type (fp16 CuHashEmbedder / fp32 HashEmbedder) and the baked image of the render fast path (dense coarse
 * levels + the level-major copy of the hashed ones; 0 before the first upload).  Replicated on every rank of a sharded render. */
NRF_API int nrf_hash_memory_bytes(const nrf_hash *h, int64_t *table_bytes, int64_t *baked_bytes);

/* CuHashEmbedder mode: the per-level position scales mul_l (host arrays of n_levels floats).  The reference computes them ON THE DEVICE, per thread, as
 * exp2f((log2f(finest) - log2f(base)) * l / (L - 1) + log2f(base)) (CuHashEmbedder.cu:40); nrf_hash_create evaluates the same expression with the host's
 * libm.  CUDA's exp2f / log2f are not libm's, and the features are fp16-ROUNDED blends: one ulp of mul_l flips the fp16 rounding of ~10 % of the features
 * of the Lego-sized grid and moves a rendered pixel by a few 1e-4 (tests/test_oracle_golden.py, sensitivity study).  A host that needs parity with a
 * particular CUDA build at the 1e-4 level reads the 16 values once from that build and sets them here; everything downstream then sees its voxels. */
NRF_API int nrf_hash_get_level_scales(const nrf_hash *h, float *scales_out);
NRF_API int nrf_hash_set_level_scales(nrf_hash *h, const float *scales, void *stream);

/* BaseEmbedderImpl::forward for the hash grid: x [p,3] -> (embedding [p, L*F] fp32, keep_mask [p] u8).
 * d_keep_mask may be NULL. */
NRF_API int nrf_hash_encode(const nrf_hash *h, const float *d_x, int64_t p, float *d_out, uint8_t *d_keep_mask, void *stream);
/* CuHashEmbedder mode: the same features level-major in fp16, d_feats [n_levels][p][n_features] halfs (16-byte aligned) -- the values the row-major call
 * returns (they are fp16-rounded there too, CuHashEmbedder.cu:95) in the layout a matrix-core consumer loads as operand fragments. */
NRF_API int nrf_hash_encode_lm_f16(const nrf_hash *h, const float *d_x, int64_t p, void *d_feats, uint8_t *d_keep_mask, void *stream);
/* ... into p columns of a wider table: level l of point i at d_feats + (l * pstride + i) * n_features halfs (d_feats = the first column to write, aligned to one
 * point's n_features * 2 bytes).  A renderer that keeps the coarse pass's columns next to the fine pass's new ones (see nrf_fine_depths_merge) encodes each once. */
NRF_API int nrf_hash_encode_lm_f16_strided(const nrf_hash *h, const float *d_x, int64_t p, void *d_feats, int64_t pstride, uint8_t *d_keep_mask, void *stream);

/* ---------------------------------------------------------------------------------------------
 * MLPs                                                         BaseNeRFImpl::forward (NeRF.h:33-42)
 * Parameters: ONE fp32 blob in the reference's named_parameters() == checkpoint order
 * (NeRFExecutor.h:1055-1070), Linear weights [out, in] row-major.
 * ------------------------------------------------------------------------------------------- */
enum {
    NRF_PREC_F32 = 0,      /* fp32 FMA chains in ascending k: the parity mode (== oracle bit for bit) */
    NRF_PREC_F16_MFMA = 1, /* fp16 operands on the matrix cores, fp32 accumulate: the fast mode */
    NRF_PREC_F16_SPLIT = 2 /* matrix cores with every operand carried as hi + lo fp16 pairs (22 significant bits, three MFMAs per
                              product): fp32-grade results at matrix-core speed.  Built for NeRFSmall, the classic 8 x 256 NeRF and
                              the fused LeRF passes (nrf_lerf_set_precision). */
};

typedef struct nrf_mlp_small_desc {      /* NeRFSmallImpl ctor (NeRF.cpp:322-360) */
    int input_ch, input_ch_views;
    int num_layers, hidden_dim, geo_feat_dim;
    int num_layers_color, hidden_dim_color;
    /* the predicted-normals head (NeRF.cpp:343-347, :393-407; the executor builds it only when n_importance == 0 && use_pred_normal, NeRFExecutor.h:487): a third
     * bias-free net on cat[sigma, geo_feat, input_pts] -> 3, appended to the output: [rgb, sigma, normal xyz] = 7 columns.  NRF_PREC_F32 only (the matrix-core
     * precisions answer NRF_ERR_UNSUPPORTED for such a handle); RawToOutputs ignores the extra columns (NeRFRenderer.h:279).  Zero-initialised fields = no head. */
    int use_pred_normal, num_layers_normals, hidden_dim_normals;
} nrf_mlp_small_desc;

typedef struct nrf_mlp_nerf_desc {       /* NeRFImpl ctor (NeRF.cpp:41-90) */
    int depth, width, input_ch, input_ch_views, output_ch, skip, use_viewdirs;
} nrf_mlp_nerf_desc;

typedef struct nrf_mlp nrf_mlp;

NRF_API int64_t nrf_mlp_small_param_count(const nrf_mlp_small_desc *d);
NRF_API int64_t nrf_mlp_nerf_param_count(const nrf_mlp_nerf_desc *d);
/* LeRFImpl (LeRF.cpp:3-26) described with nrf_mlp_small_desc: input_ch = input_ch_le, num_layers = num_layers_le, hidden_dim =
 * hidden_dim_le, geo_feat_dim = geo_feat_dim_le, hidden_dim_color = lang_embed_dim (other fields ignored). Output [p, lang_embed_dim + 1]. */
NRF_API int64_t nrf_mlp_lerf_param_count(const nrf_mlp_small_desc *d);
NRF_API int nrf_mlp_lerf_create(const nrf_mlp_small_desc *d, const float *params, int params_on_device, void *stream, nrf_mlp **out);
NRF_API int nrf_mlp_small_create(const nrf_mlp_small_desc *d, const float *params, int params_on_device, void *stream, nrf_mlp **out);
NRF_API int nrf_mlp_nerf_create(const nrf_mlp_nerf_desc *d, const float *params, int params_on_device, void *stream, nrf_mlp **out);
NRF_API void nrf_mlp_destroy(nrf_mlp *m);
NRF_API int nrf_mlp_output_dims(const nrf_mlp *m);
/* forward: x [p, input_ch + input_ch_views] -> out [p, output_dims] */
NRF_API int nrf_mlp_forward(const nrf_mlp *m, const float *d_x, int64_t p, int precision, float *d_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Compositing and hierarchical sampling
 * ------------------------------------------------------------------------------------------- */

/* NeRFRenderer::RawToOutputs (NeRFRenderer.h:199-282) + TruncExp::forward (CustomOps.cpp:5-9).
 * raw [n,s,c] (rgb at 0..2, sigma at 3), z [n,s], d [n,3] (stride d_stride floats).
 * Any output pointer may be NULL. */
NRF_API int nrf_raw2outputs(const float *d_raw, const float *d_z, const float *d_dirs, int d_stride, int64_t n, int s, int c,
                            int white_bkgr, float *d_rgb, float *d_disp, float *d_acc, float *d_weights, float *d_depth,
                            void *stream);

/* LeRF: the weights / depth part of LeRFRenderer::RawToLEOutputs (LeRFRenderer.cpp:27-76): the same sigma -> alpha -> weights
 * arithmetic as RawToOutputs with sigma at channel `sigma_ch` of a c-wide raw tensor and no colour. */
NRF_API int nrf_raw2weights(const float *d_raw, int c, int sigma_ch, const float *d_z, const float *d_dirs, int d_stride, int64_t n, int s,
                            float *d_weights, float *d_depth, float *d_disp, float *d_acc, void *stream);

/* The same with sample (ray, j)'s raw row read at row d_src[ray * s + j] (int32) of d_raw: the feature-reusing LeRF pass keeps sigma_le in feature-COLUMN order
 * (coarse columns, then the new samples') and composes through the merge map of nrf_fine_depths_merge instead of gathering first. */
NRF_API int nrf_raw2weights_gather(const float *d_raw, int c, int sigma_ch, const int32_t *d_src, const float *d_z, const float *d_dirs, int d_stride, int64_t n, int s,
                                   float *d_weights, float *d_depth, float *d_disp, float *d_acc, void *stream);

/* The LeRF head fused with its render pass on the matrix cores (fp16 operands, fp32 accumulate), for the reference's LeRF shape
 * (main.cpp:203-213: in 128, hidden 256, 2 + 2 layers, geo 32, embedding 768) -- the [N, S, 769] raw tensor is never formed.
 *   nrf_lerf_sigma            : sigma_le = LeRFImpl::forward(x)[..., -1] (LeRF.cpp:86-95), zeroed where keep is false (LeRFRenderer.cpp:22-23)
 *   nrf_lerf_render_embedding : out[n, 768] = sum_s weights[n,s] * normalize(le(x[n,s]))  (LeRF.cpp:96-108 + the sum of LeRFRenderer.h:45-54);
 *                               s must be a multiple of 32.  L2-normalise `out` afterwards (nrf_render_clip_embedding's last step).
 *                               Evaluated as W . sum_s (weights / ||W a||) a with ||W a||^2 = a^T (W^T W) a (the output layer is bias-free, hence linear): the
 *                               256 -> 768 layer runs once per ray.  Takes n * 256 floats of stream-ordered scratch (hipMallocAsync / hipFreeAsync).
 *                               The weight image holds W^T W and W each times a power of two chosen from max|W^T W| (fp16 range; mlp_lerf_mfma.hip), so `out` does not
 *                               depend on a power-of-two scale of W (pinned for W x 2^-8 .. 2^+8); the 1e-8 floor applies to ||W a|| with W at the image's scale, its
 *                               largest column norm in (sqrt 2, sqrt 8] -- the reference initialisation's own. */
NRF_API int nrf_lerf_mfma_available(const nrf_mlp *m);
/* Arithmetic of the four fused entries below, per handle: NRF_PREC_F16_MFMA (default: fp16 operands, fp32 accumulate) or NRF_PREC_F16_SPLIT (hi + lo fp16
 * operand pairs, three products: fp32-grade, as LeRFImpl::forward computes -- mlp_lerf_split_mfma.hip).  Call between, not during, passes. */
NRF_API int nrf_lerf_set_precision(nrf_mlp *m, int precision);
NRF_API int nrf_lerf_sigma(const nrf_mlp *m, const float *d_x, const uint8_t *d_keep, int64_t p, float *d_sigma, void *stream);
NRF_API int nrf_lerf_render_embedding(const nrf_mlp *m, const float *d_x, const float *d_weights, int64_t n, int s, float *d_out, void *stream);
/* ... reading the level-major fp16 features of nrf_hash_encode_lm_f16 (16 levels x 8 features: [16][p][8] halfs) instead of fp32 rows. */
NRF_API int nrf_lerf_sigma_lm(const nrf_mlp *m, const void *d_feats_lm, const uint8_t *d_keep, int64_t p, float *d_sigma, void *stream);
NRF_API int nrf_lerf_render_embedding_lm(const nrf_mlp *m, const void *d_feats_lm, const float *d_weights, int64_t n, int s, float *d_out, void *stream);
/* ... on columns of a wider level-major table ([16][pstride][8] halfs): _strided evaluates p consecutive columns starting at d_feats_lm; _gather reads column
 * d_src[i] for sample i of the n * s sorted depths (d_src = the merge map of nrf_fine_depths_merge; NULL = column i).  Same arithmetic, same results. */
NRF_API int nrf_lerf_sigma_lm_strided(const nrf_mlp *m, const void *d_feats_lm, int64_t pstride, const uint8_t *d_keep, int64_t p, float *d_sigma, void *stream);
/* Split precision only: kernel A also leaves the sigma net's second output (sigma, geo32: LE0's chained operand, 192 bytes per column as fragment planes,
 * nrf_lerf_geo_bytes(columns)) in d_geo, and the embedding pass starts at LE0 from it instead of re-evaluating the sigma net (224 of its 832 matrix
 * instructions per 32 points).  d_geo / d_feats_lm of a _strided call point at the call's first column; geo_stride = columns of the whole table.
 * Same values in the same order as the recomputation: results unchanged.  NRF_ERR_UNSUPPORTED in NRF_PREC_F16_MFMA. */
NRF_API size_t nrf_lerf_geo_bytes(int64_t columns);
NRF_API int nrf_lerf_sigma_geo_lm_strided(const nrf_mlp *m, const void *d_feats_lm, int64_t pstride, const uint8_t *d_keep, int64_t p, float *d_sigma,
                                          void *d_geo, int64_t geo_stride, void *stream);
/* The LeRF density net in EXACT fp32 on the matrix cores (sigma_lerf_f32.hip): d_sigma equals nrf_mlp_forward(..., NRF_PREC_F32)[..., -1] -- and the CPU oracle --
 * bit for bit (v_mfma_f32_32x32x2_f32 == the ascending-k fmaf chain), at ~0.8 of the 157 TFLOP/s fp32 matrix peak.  The coarse pass of a hierarchical LeRF render
 * consumes nothing but sigma_le (LeRFRenderer.cpp:139-170) and its weights choose the fine samples through a discontinuous function, so the split-precision render
 * runs its coarse pass through this entry: the fine sample set is then the fp32 path's own.  d_geo (optional): also leaves (sigma, geo32) as the (hi, lo) operand
 * planes of nrf_lerf_render_embedding_lm_geo, split from the exact values.  Level-major CuHashEmbedder features, same column conventions as the _strided entries. */
NRF_API int nrf_lerf_sigma_exact_available(const nrf_mlp *m);
NRF_API int nrf_lerf_sigma_exact_lm_strided(const nrf_mlp *m, const void *d_feats_lm, int64_t pstride, const uint8_t *d_keep, int64_t p, float *d_sigma,
                                            void *d_geo, int64_t geo_stride, void *stream);
NRF_API int nrf_lerf_render_embedding_lm_geo(const nrf_mlp *m, const void *d_feats_lm, int64_t pstride, const int32_t *d_src, const void *d_geo,
                                             int64_t geo_stride, const float *d_weights, int64_t n, int s, float *d_out, void *stream);
NRF_API int nrf_lerf_render_embedding_lm_gather(const nrf_mlp *m, const void *d_feats_lm, int64_t pstride, const int32_t *d_src, const float *d_weights, int64_t n,
                                                int s, float *d_out, void *stream);

/* RenderCLIPEmbedding (LeRFRenderer.h:45-54): out[n, embed_dim] = normalize(sum_s weights[n,s] * embeds[n,s,:embed_dim], eps 1e-8).
 * embeds rows are embed_stride floats apart (the raw LeRF output is [n,s,embed_dim+1]). */
NRF_API int nrf_render_clip_embedding(const float *d_embeds, int embed_stride, int embed_dim, const float *d_weights, int64_t n, int s,
                                      float *d_out, void *stream);

/* Relevancy(embeds, positives, negatives) (call sites LeRFRenderer.cpp:79, NeRFExecutor.h:824): [n, embed_dim] L2-normalised embeddings against
 * [n_pos, embed_dim] positive and [n_neg, embed_dim] negative ("canonical") phrase embeddings -> d_out [n, 2] = (p_positive, p_negative) of the pairwise softmax
 * (temperature 10) against the negative phrase the positive does worst against; column 0 is what the hosts consume (LeRFRenderer.h:18, NeRFExecutor.h:714).
 * PARITY UNPINNED: the function's source is external (DeliriumV01D/RuCLIP, RuCLIPProcessor.h, no pinned version, absent from the reference tree) -- this is the
 * published LERF relevancy score (Kerr et al. 2023, section 3.3; nerfstudio `get_relevancy`) that it mirrors, restated in oracle/nerf_oracle.c (orc_relevancy) and
 * checked against that and against known answers.  positive_id selects the row of d_positives (the reference passes one positive phrase: 0). */
NRF_API int nrf_lerf_relevancy(const float *d_embeds, int64_t n, int embed_dim, const float *d_positives, int n_pos, const float *d_negatives, int n_neg,
                               int positive_id, float *d_out, void *stream);

/* The relevancy image of RenderPath (NeRFExecutor.h:713-719): rel[..., 0].mul(255).to(kU8) -> cv::applyColorMap(COLORMAP_JET) -> d_bgr [n, 3] bytes in OpenCV's
 * B, G, R order.  d_relevancy rows are rel_stride floats apart (2 for nrf_lerf_relevancy's output).  nrf_colormap_jet_u8 maps bytes that already are the image
 * (the training-time preview, NeRFExecutor.h:825-831); nrf_colormap_jet_lut writes the 256 x 3 table to HOST memory.
 * PARITY UNPINNED: OpenCV is not in this image; the table is restated from OpenCV's published colormap (oracle/nerf_oracle.c, orc_colormap_jet_lut, says how). */
NRF_API int nrf_relevancy_image(const float *d_relevancy, int64_t n, int rel_stride, uint8_t *d_bgr, void *stream);
NRF_API int nrf_colormap_jet_u8(const uint8_t *d_gray, int64_t n, uint8_t *d_bgr, void *stream);
NRF_API int nrf_colormap_jet_lut(uint8_t *lut_host /*[256*3]*/);

/* ---- language targets from a cached CLIP pyramid: PyramidEmbedding (PyramidEmbedder.h:32-81, PyramidEmbedder.cpp:4-310) ----
 * The reference computes LeRF training targets on the host, one pixel per call of GetPixelValue inside an OpenMP loop (NeRFDataset.cpp:180-193), and its relevancy
 * preview the same way for every pixel of a view (NeRFExecutor.h:803-831).  A pyramid here holds the reference's cache (pyramid_embeddings.pt, PyramidEmbedding::Save /
 * Load, PyramidEmbedder.cpp:199-223) in device memory: one dense fp32 block [nh][nw][D] per (image, level), levels -1 .. max_zoom_out, for every level whose grid is
 * not empty.  Building a pyramid (RuCLIP over OpenCV tiles, PyramidEmbedder::operator() / GetNextSample) is not done here.
 *
 * nrf_pyramid_level_geometry : window size and grid of one level (GetNearestPatchIndicesSingleScale, :15-19, the reference's int / float / double mix): host only;
 *                              out = {win, nw, nh}; nw or nh <= 0 means the level has no grid.
 * nrf_pyramid_max_zoom_out   : PyramidEmbedderProperties::MaxZoomOut as the dataset sets it (NeRFDataset.cpp:86, :178): int(min(log2f(wmax / clip), log2f(hmax / clip)))
 *                              with integer quotients, over wh [n, 2] = {W, H} per view; host only.  A largest view narrower or lower than clip (log2f(0)) is rejected.
 * nrf_pyramid_create         : empty pyramid for n_images views of sizes wh [n, 2] = {W, H} (host).  D = lang_embed_dim, clip = clip_input_img_size (square, :73),
 *                              overlap = pyr_embedder_overlap.  Allocates every block; nrf_pyramid_memory_bytes = the sum of nw * nh * D * 4 over them.
 * nrf_pyramid_set_entries    : n cache entries: keys host int32 [n, 4] = {hor_pos_idx, vert_pos_idx, zoom_out_idx, data_img_id} (the std::map key), emb host fp32
 *                              [n, d] (the [1, D] tensors).  d must equal D; a key outside its image's levels or grid is rejected (NRF_ERR_INVALID_ARG, nothing
 *                              stored).  A key given again replaces the earlier row.  Synchronises `stream` (the host arrays are released before returning).
 * nrf_pyramid_pixel_values   : GetPixelValue(x, y, scale, img_id, properties, {W, H}) (:230-310) for n pixels: d_x, d_y device int64 [n], each converted to float as the
 *                              dataset's .to(kFloat) does; row k of d_out (out_stride floats apart, >= D) receives pixel k's [D] embedding.  The call sites' argument
 *                              orders differ and are the caller's: get_batch passes x = rand_h, y = rand_w (NeRFDataset.cpp:186-187), the preview x = column, y = row.
 *                              Bit for bit the reference's ATen fp32 arithmetic (the three degenerate Interpolate forms included); a scale above the top level gives
 *                              0/0, i.e. NaN rows, as the reference's does.  Both levels the scale selects (z1 and z2, :97-113) must have every entry, img_id must be a
 *                              view of the pyramid and scale a positive finite number: otherwise NRF_ERR_INVALID_ARG before any launch (the reference throws on the
 *                              undefined tensor of a missing map entry).  Pinned by a restatement of the reference's arithmetic (tests/test_pyramid_*.py), not by a
 *                              golden of the compiled reference (PyramidEmbedder.cpp needs OpenCV and RuCLIP).
 * nrf_pyramid_relevancy_preview : the preview loop of NeRFExecutor::Train (NeRFExecutor.h:803-831) for view img_id: GetPixelValue(i, j, scale) for every column i and
 *                              row j, Relevancy against the phrases (device [n_pos, D] / [n_neg, D], as nrf_lerf_relevancy takes them), cv::saturate_cast<uchar>(rel *
 *                              255) into d_gray [H * W] (row j, column i at j * W + i), and with d_bgr (optional, [H * W, 3]) cv::applyColorMap(COLORMAP_JET) as
 *                              nrf_colormap_jet_u8.  saturate_cast is OpenCV's cvRound (cvtss2si on x86: round half to even; NaN gives INT_MIN, i.e. 0) then a clamp.
 *                              Rows go through the workspace in chunks; nrf_pyramid_relevancy_preview_workspace_bytes(p, img_id, rows) sizes it for `rows` rows at
 *                              a time (NRF_ERR_WORKSPACE below one row).  PARITY UNPINNED beyond the pixel values, as nrf_lerf_relevancy and the colormap are:
 *                              OpenCV is not in this image. */
typedef struct nrf_pyramid nrf_pyramid;
NRF_API int nrf_pyramid_level_geometry(int img_w, int img_h, int clip, float overlap, int zoom, int *out /*[3] = win, nw, nh*/);
NRF_API int nrf_pyramid_max_zoom_out(const int *wh /*[n, 2]*/, int n_images, int clip, int *out);
NRF_API int nrf_pyramid_create(int d, int clip_size, float overlap, int max_zoom_out, int n_images, const int *wh /*[n, 2]*/, nrf_pyramid **out);
NRF_API int nrf_pyramid_destroy(nrf_pyramid *p);
NRF_API int64_t nrf_pyramid_memory_bytes(const nrf_pyramid *p);
NRF_API int nrf_pyramid_set_entries(nrf_pyramid *p, int64_t n, const int32_t *keys /*[n, 4]*/, const float *emb /*[n, d]*/, int d, void *stream);
NRF_API int nrf_pyramid_pixel_values(const nrf_pyramid *p, int img_id, float scale, const int64_t *d_x, const int64_t *d_y, int64_t n, float *d_out, int64_t out_stride,
                                     void *stream);
NRF_API size_t nrf_pyramid_relevancy_preview_workspace_bytes(const nrf_pyramid *p, int img_id, int rows);
NRF_API int nrf_pyramid_relevancy_preview(const nrf_pyramid *p, int img_id, float scale, const float *d_positives, int n_pos, const float *d_negatives, int n_neg,
                                          int positive_id, uint8_t *d_gray, uint8_t *d_bgr, void *d_workspace, size_t workspace_bytes, void *stream);

/* SamplePDF, deterministic branch (Sampler.h:6-43).  bins [n,nb], weights [n,nb-1], u [ns] device
 * (= linspace(0,1,ns)).  sum_vec: fp32 lanes of the host whose torch::sum order is reproduced for the
 * pdf normaliser (8 = any AVX2+/AVX-512 x86 build of ATen; 0 = order-free double accumulation).
 * d_inds (optional): the searchsorted indices, int64 like the reference's. */
NRF_API int nrf_sample_pdf(const float *d_bins, const float *d_weights, int64_t n, int nb, const float *d_u, int ns, int sum_vec,
                           float *d_samples, int64_t *d_inds, void *stream);

/* The fine-pass depth set of RenderRays (NeRFRenderer.h:427-431): z_mid, SamplePDF on weights[1:-1],
 * sort(cat(z, samples)).  z [n,s], weights [n,s] -> z_fine [n, s+ns]. */
NRF_API int nrf_fine_depths(const float *d_z, const float *d_weights, int64_t n, int s, const float *d_u, int ns, int sum_vec,
                            float *d_z_fine, void *stream);
/* ... and where each sorted depth came from.  s of the s + ns depths of a ray ARE its coarse depths (same z, hence the same sample point and the same
 * encoder features, bit for bit), so a fine pass need only encode the ns new ones:
 *   d_src [n, s+ns] int32 : column of sorted depth (ray, i) in a table holding the coarse pass's n*s points first (ray-major) and the n*ns new points after
 *                           them: ray*s + j for coarse depth j, n*s + ray*ns + j for new sample j
 *   d_z_new [n, ns]       : the new samples' depths in SamplePDF order (ascending)
 * nrf_render_rays does this internally; the entry serves hosts that drive the passes themselves (the LeRF render pass).  n (s + ns) < 2^31. */
NRF_API int nrf_fine_depths_merge(const float *d_z, const float *d_weights, int64_t n, int s, const float *d_u, int ns, int sum_vec,
                                  float *d_z_fine, int32_t *d_src, float *d_z_new, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Stochastic branches of RenderRays (Perturb > 0, cone rays, training-time noise).  The stage functions take the random
 * draws as explicit device arrays -- hand them the reference's own torch::rand / randn tensors and the results can be
 * compared value for value.  nrf_render_rays itself generates draws in-kernel from (seed, stream, GLOBAL element index)
 * with include/nrf_rng.h (streams NRF_RNG_*), so a render does not depend on Chunk or on the ray sharding;
 * nrf_rng_fill materialises the same draws: element k = draw(seed, rng_stream, index0 + k), uniform [0,1) or normal.
 * ------------------------------------------------------------------------------------------- */
NRF_API int nrf_rng_fill(uint64_t seed, uint32_t rng_stream, uint64_t index0, int64_t count, int normal, float *d_out, void *stream);

/* Stratified jitter (NeRFRenderer.h:404-417): z [n,s], t_rand [n,s] uniform -> out [n,s] (must not alias z). */
NRF_API int nrf_jitter_z(const float *d_z, const float *d_t_rand, int64_t n, int s, float *d_out, void *stream);

/* TangentScatter (NeRFRenderer.h:307-362).  d_pts [n,s,3] or NULL (= o + d*z from the packed rays); rays_d is read from the
 * packed rays (columns 3..5); u_r / u_theta [n,s] uniform draws; bbox: host [6] or NULL (no clamp). */
NRF_API int nrf_tangent_scatter(const float *d_pts, const float *d_rays, int ray_stride, const float *d_z, int64_t n, int s, float cone_angle,
                                const float *d_u_r, const float *d_u_theta, const float *bbox, float *d_out, void *stream);

/* Stochastic preconditioning + ReflectBoundary (NeRFRenderer.h:433-443, :285-304): pts [p,3] + noise [p,3]*alpha, reflected. */
NRF_API int nrf_precondition(const float *d_pts, const float *d_noise, float alpha, const float *bbox, int64_t p, float *d_out, void *stream);

/* RawToOutputs with raw_noise_std > 0 (NeRFRenderer.h:251-252): noise [n,s] normal draws. */
NRF_API int nrf_raw2outputs_noise(const float *d_raw, const float *d_z, const float *d_dirs, int d_stride, int64_t n, int s, int c, int white_bkgr,
                                  const float *d_noise, float noise_std, float *d_rgb, float *d_disp, float *d_acc, float *d_weights,
                                  float *d_depth, void *stream);

/* SamplePDF with det = false (Sampler.h:22-24) and the fine depth set built on it: u is [n, ns], one unsorted row per ray. */
NRF_API int nrf_sample_pdf_rand(const float *d_bins, const float *d_weights, int64_t n, int nb, const float *d_u, int ns, int sum_vec,
                                float *d_samples, int64_t *d_inds, void *stream);
NRF_API int nrf_fine_depths_rand(const float *d_z, const float *d_weights, int64_t n, int s, const float *d_u, int ns, int sum_vec,
                                 float *d_z_fine, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Renderer                                    NeRFRenderer<TEmbedder,TEmbedDirs,TNeRF> (NeRFRenderer.h:88-159)
 * ------------------------------------------------------------------------------------------- */
enum { NRF_DIRS_NONE = 0, NRF_DIRS_PE = 1, NRF_DIRS_SH_LIBTORCH = 2, NRF_DIRS_SH_CUDA = 3 };

typedef struct nrf_renderer_desc {
    const nrf_hash *hash;     /* position encoder: hash grid, or NULL for sinusoidal PE */
    int pe_freqs;             /* used when hash == NULL (Embedder multires, NeRFExecutor.h:427) */
    int dirs_encoder;         /* NRF_DIRS_* */
    int dirs_param;           /* PE: multires_views;  SH: degree */
    const nrf_mlp *mlp;
} nrf_renderer_desc;

/* NeRFRenderParams (NeRFRenderer.h:28-44) as RenderRays consumes them.  Zero-initialise the struct: all stochastic
 * fields 0 is the deterministic render path (Perturb = 0, RawNoiseStd = 0, ThinRay = true -- what FillRenderParams sets
 * at test time, NeRFExecutor.h:379-415, plus ThinRay). */
/* The coarse pass of a hierarchical render contributes only its compositing weights (NeRFRenderer.h:422-428), i.e. sigma, and those
 * weights choose the fine samples through searchsorted -- a discontinuous function.  NRF_COARSE_AUTO: with NRF_PREC_F16_SPLIT on the
 * HashNeRF fast path the coarse pass evaluates the sigma net ONLY, in exact fp32 on the matrix cores (v_mfma_f32_32x32x2_f32 ==
 * the ascending-k fma chain of NRF_PREC_F32, bit for bit), so the fine sample set equals the parity mode's; that kernel also hands the
 * sigma net's output (sigma, geo_feat) of the coarse points to the fine pass, which evaluates the colour net alone at its n_samples coarse
 * depths (their sigma is then NRF_PREC_F32's bit for bit) and the whole network at the n_importance new ones; every other case runs
 * the whole network in `precision`.  NRF_COARSE_FULL forces the latter, NRF_COARSE_SIGMA_F32 asks for the former in
 * NRF_PREC_F16_MFMA too.  A caller that wants d_raw_coarse always gets the whole network. */
enum { NRF_COARSE_AUTO = 0, NRF_COARSE_FULL = 1, NRF_COARSE_SIGMA_F32 = 2 };

typedef struct nrf_render_params {
    int n_samples;            /* NSamples */
    int n_importance;         /* NImportance */
    int lindisp;              /* LinDisp */
    int white_bkgr;           /* WhiteBkgr */
    int precision;            /* NRF_PREC_* for the MLP */
    int sum_vec;              /* see nrf_sample_pdf */
    /* stochastic branches; draws come from include/nrf_rng.h keyed by (seed, stream, (ray_base + ray)*S + sample) */
    float perturb;            /* Perturb > 0: stratified jitter + SamplePDF(det = false) */
    int has_cone;             /* !ThinRay: TangentScatter on both passes with `cone_angle` (GetRays, RayUtils.h:43-44) */
    float cone_angle;
    float raw_noise_std;      /* RawNoiseStd */
    float precond_alpha;      /* StochasticPreconditioningAlpha (fine pass only, as in the reference) */
    int has_bbox;             /* BoundingBox given: TangentScatter clamps to it; required by precond_alpha > 0 */
    float bbox[6];
    uint64_t seed;
    int64_t ray_base;         /* index of d_rays[0] within the whole image / ray batch */
    int coarse_mode;          /* NRF_COARSE_*: how the coarse pass is evaluated when n_importance > 0 (it only supplies SamplePDF's weights) */
    int overflow_policy;      /* NRF_OVERFLOW_*: what happens when a matrix-core precision's network outputs are not finite (below) */
} nrf_render_params;

/* The matrix-core precisions carry operands in fp16 (NRF_PREC_F16_MFMA) or as fp16 (hi, lo) pairs (NRF_PREC_F16_SPLIT): an activation beyond 65 504 becomes an inf there.
 * NeRFSmall's split image is range-scaled against that (nrf_mlp_set_input_rms_hint); whatever still overflows -- or any other family's network -- shows as inf / NaN network
 * outputs, which the final compositing kernel of every chunk records in a per-chunk word of the renderer (4 FMAs per sample).  What the render entries do with it:
 *   NRF_OVERFLOW_AUTO / _RERENDER  after the Chunk loop the words are read back (ONE host synchronisation at the end of nrf_render_rays / nrf_batchify_rays /
 *                                  nrf_render_rows) and every flagged chunk is rendered again in NRF_PREC_F32 into the same outputs: the call's results are finite-input
 *                                  correct whatever the weights.  The default.
 *   NRF_OVERFLOW_ERROR             same read-back; a flagged chunk makes the call return NRF_ERR_NONFINITE (outputs of that chunk are not to be used).
 *   NRF_OVERFLOW_DEFERRED          no synchronisation: the words are copied to pinned host memory behind the call's work and looked at by the first LATER render call on
 *                                  this renderer that finds the copy complete, which then returns NRF_ERR_NONFINITE before doing anything (or by nrf_renderer_nonfinite).
 *                                  Up to 32 calls' words may be in flight; the 33rd call waits for the oldest copy.  For pipelines that keep several frames in flight.
 *   NRF_OVERFLOW_IGNORE            no detection at all (the compositing kernel skips the test).
 * With nrf_set_live_colour on (the default) the fine pass does not evaluate the colour net at coarse depths whose sigma is not positive; their rows read (0, 0, 0, sigma).
 * A non-finite COLOUR at such a depth -- which met a zero weight and never reached a pixel -- therefore no longer sets the word; a non-finite sigma there still does. */
enum { NRF_OVERFLOW_AUTO = 0, NRF_OVERFLOW_RERENDER = 1, NRF_OVERFLOW_ERROR = 2, NRF_OVERFLOW_DEFERRED = 3, NRF_OVERFLOW_IGNORE = 4 };

typedef struct nrf_render_outputs {   /* NeRFRendererOutputs / NeRFRenderResult (NeRFRenderer.h:12-26); NULL = not wanted */
    float *d_rgb;             /* [n,3] */
    float *d_disp;            /* [n]   */
    float *d_acc;             /* [n]   */
    float *d_depth;           /* [n]   */
    float *d_weights;         /* [n, S_out]  S_out = n_samples + n_importance (or n_samples if n_importance == 0) */
    float *d_raw;             /* [n, S_out, 4] in depth order.  The fast paths keep the network outputs where they were computed (coarse depths | new samples) and the
                               * compositing kernel reads through the merge map; asking for d_raw adds one gather pass (16 B read + written per sample) */
    /* intermediates for stage-chained parity tests (optional) */
    float *d_z_coarse;        /* [n, n_samples] */
    float *d_raw_coarse;      /* [n, n_samples, 4] */
    float *d_weights_coarse;  /* [n, n_samples] */
    float *d_z_fine;          /* [n, n_samples + n_importance] */
} nrf_render_outputs;

/* Normal maps of a render: the *_normals entries below take this beside the two structs above, which keep their layout (a caller compiled against an earlier header
 * hands the library structs of that size).  The plain entries render no normals.
 *   NRF_NORMALS_DENSITY    d_normals [n,3] = sum_i w_i n_i over the final samples and weights in ascending order (summed in fp64, rounded once), n_i = -g / max(|g|, 1e-8),
 *                          g = nrf_density_grad at the point the fine network saw (the perturbed one with cone rays / preconditioning); a zero-weight sample
 *                          contributes 0.  Hash grid + NeRFSmall renderers, every precision.
 *   NRF_NORMALS_PREDICTED  d_pred_normals [n,3] = sum_i w_i (v / max(|v|, 1e-8)), v = raw_i[4:7] of a NeRFSmall with the predicted-normals head, NRF_PREC_F32 only.
 * RGB, disparity, accumulation, depth and weights equal the plain entry's bit for bit.  bits = 0 is the plain entry (same workspace size).  A set bit with a NULL
 * output, unknown bits (NRF_ERR_INVALID_ARG) or an unsupported renderer / network / precision (NRF_ERR_UNSUPPORTED, NRF_ERR_INVALID_ARG) fail before any launch. */
enum { NRF_NORMALS_DENSITY = 1, NRF_NORMALS_PREDICTED = 2 };
typedef struct nrf_render_normals {
    int bits;                 /* NRF_NORMALS_* */
    float *d_normals;         /* [n,3] when bits & NRF_NORMALS_DENSITY */
    float *d_pred_normals;    /* [n,3] when bits & NRF_NORMALS_PREDICTED */
} nrf_render_normals;

typedef struct nrf_renderer nrf_renderer;

NRF_API int nrf_renderer_create(const nrf_renderer_desc *desc, nrf_renderer **out);
NRF_API void nrf_renderer_destroy(nrf_renderer *r);
/* Totals since the renderer was created: chunks whose matrix-core render produced non-finite network outputs, and how many of them were rendered again in NRF_PREC_F32
 * (NRF_OVERFLOW_RERENDER).  Completes a pending NRF_OVERFLOW_DEFERRED check first (waits for that call's work).  Either pointer may be NULL. */
/* Where the most recent render call on this renderer left the hash features of its fine depths -- a SINGLE-chunk call (nrf_render_rays, or nrf_batchify_rays with
 * Chunk >= n) of the feature-reusing fast path on a CuHashEmbedder grid: the level-major fp16 table [16][cols] (half2; coarse columns first, the new samples' behind
 * them), the keep mask by column, and the merge map [n, sf] (sorted depth i of the batch -> its column).  They live in the caller's workspace: valid until the next
 * render call on this renderer or any other use of that workspace.  NRF_ERR_UNSUPPORTED when the last call left none (serial is set either way).  For nrf_mlp_backward_f16_lm_src /
 * nrf_mask_sigma_grad_src: a training step's backward reads the features its own forward render encoded instead of encoding the fine points again. */
NRF_API int nrf_renderer_last_features(const nrf_renderer *r, const void **d_feats_lm, int64_t *cols, const uint8_t **d_keep_cols, const int32_t **d_src, int64_t *n, int *sf,
                                       uint64_t *serial /* optional: a count of the chunks this renderer has rendered -- unchanged between two queries = no render in between */);
NRF_API int nrf_renderer_nonfinite(const nrf_renderer *r, int64_t *flagged_chunks, int64_t *rerendered_chunks);

/* RunNetwork (NeRFRenderer.h:164-194): pts [n,s,3], viewdirs [n,3] (or NULL) -> raw [n,s,4]
 * with sigma forced to 0 where the embedder's keep_mask is false (:187-188). */
NRF_API size_t nrf_run_network_workspace_bytes(const nrf_renderer *r, int64_t n, int s);
NRF_API int nrf_run_network(const nrf_renderer *r, const float *d_pts, const float *d_viewdirs, int64_t n, int s, int precision,
                            float *d_raw, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Mesh export (mesh.hip; no counterpart in the reference: its scenes are looked at through rendered images only)
 * ------------------------------------------------------------------------------------------- */
/* Density lattice: d_sigma [nz][ny][nx] (x fastest) = raw[..., 3] of nrf_run_network(NRF_PREC_F32) at P(i, j, k), bit for bit, keep-mask rule of
 * NeRFRenderer.h:187-188 included (outside the hash box a 4-column net gives 0).  bbox[6] (host): min xyz, max xyz; P = bmin + (float)i * step per axis,
 * step = (bmax - bmin) / (float)(n - 1), one fp32 rounding per operation; nx, ny, nz >= 2.  The colour net is not evaluated: hash grid + NeRFSmall and the classic
 * PE(10) / PE(4) network run their exact-fp32 density kernels (the coarse pass's), any other renderer the F32 network.  Work goes in slabs of slab_points lattice
 * points (<= 0: 2^22; at most 2^30), so the workspace is bounded whatever the resolution; the result does not depend on slab_points.  LeRF renderers are not covered. */
NRF_API size_t nrf_density_grid_workspace_bytes(const nrf_renderer *r, int nx, int ny, int nz, int64_t slab_points);
NRF_API int nrf_density_grid(const nrf_renderer *r, const float *bbox, int nx, int ny, int nz, float *d_sigma, int64_t slab_points,
                             void *d_workspace, size_t workspace_bytes, void *stream);
/* Isosurface of a lattice d_sigma [nz][ny][nx] (lattice points as above) at level iso: marching tetrahedra on the Kuhn split of each cell into 6 tetrahedra.
 *   inside: f > iso.  Edges start at lattice point a, 7 types in the order (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1); one vertex per crossed edge (one end
 *   inside), ordered by (linear index of a, type), at p = P(a) + t (P(b) - P(a)), t = (iso - f_a) / (f_b - f_a) (fp32).  Cells in linear order of their min corner c,
 *   tetrahedra in the axis-permutation order xyz, xzy, yxz, yzx, zxy, zyx (chain c, + e_p0, + e_p1, c + (1,1,1)); 1 or 3 corners inside: one triangle on the odd
 *   corner's three edges in chain order; 2 inside {a, b}, 2 outside {c, d}: (ac, ad, bd), (ac, bd, bc).  Counter-clockwise seen from outside (f <= iso), decided from the
 *   case and the permutation's parity.  Degenerate triangles (f_b == iso) are kept.  Normals (optional): n = -g / |g| (0 where |g| = 0) of the lattice gradient (central
 *   differences, one-sided at the border) interpolated with the same t.  Output order comes from integer prefix scans: two runs give the same arrays.
 * Two calls over one workspace: nrf_isosurface_count classifies, scans and returns the vertex and triangle counts and the number of non-finite lattice values -- it
 * SYNCHRONISES the stream to read them back (as does nrf_isosurface_emit, to check them); counts beyond int32 are refused (NRF_ERR_INVALID_ARG).  Then the host
 * allocates d_verts [V,3], d_faces [F,3] (int32), d_normals [V,3] (or NULL) and calls nrf_isosurface_emit with the same lattice, box, iso and workspace;
 * it returns NRF_ERR_NONFINITE (nothing written) when the lattice holds a non-finite value. */
NRF_API size_t nrf_isosurface_workspace_bytes(int nx, int ny, int nz);
NRF_API int nrf_isosurface_count(const float *d_sigma, int nx, int ny, int nz, const float *bbox, float iso, int64_t *n_verts, int64_t *n_tris, int64_t *n_nonfinite,
                                 void *d_workspace, size_t workspace_bytes, void *stream);
NRF_API int nrf_isosurface_emit(const float *d_sigma, int nx, int ny, int nz, const float *bbox, float iso, float *d_verts, int32_t *d_faces, float *d_normals,
                                int64_t n_verts, int64_t n_tris, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Connected components (components.hip; no counterpart in the reference)
 * ------------------------------------------------------------------------------------------- */
/* Which faces of a mesh, which set points of a lattice belong together.  A lock-free union-find on the device whose result is
 * canonical: components are numbered 0 .. K-1 in ascending order of their smallest member index (vertex id / linear lattice index), so two runs, and any correct
 * implementation, give the same array.  Both entries SYNCHRONISE the stream once to return *n_components (as nrf_isosurface_count does for its counts).
 *   nrf_mesh_components: d_faces [F,3] int32 over V vertices -> d_labels [V] int32: vertices that share a face share a label, a vertex used by no face gets -1; the
 *   component of a face is the label of its first vertex.  Degenerate ((a,a,b), (a,a,a)) and duplicate faces are legal; 0 <= V, F < 2^31.  A vertex index outside
 *   [0, V) gives NRF_ERR_INVALID_ARG: such a face is skipped (nothing is read or written at the index) and the labels are unspecified.
 *   nrf_lattice_components: d_mask [nz][ny][nx] uint8 (x fastest, non-zero = set) -> d_labels of the same shape, -1 where the mask is 0.  connectivity 6 (faces),
 *   26 (faces, edges, corners) or 14: the 7 edge types of the isosurface's Kuhn split, (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1), and their negatives
 *   -- the components of sigma > iso under 14 are exactly the solids whose surfaces nrf_isosurface_* emits.  Any other value is NRF_ERR_INVALID_ARG.  Neighbours
 *   never wrap across a row or a plane; nx, ny, nz >= 1, nx * ny * nz < 2^31. */
NRF_API size_t nrf_mesh_components_workspace_bytes(int64_t n_verts, int64_t n_tris);
NRF_API int nrf_mesh_components(const int32_t *d_faces, int64_t n_verts, int64_t n_tris, int32_t *d_labels, int64_t *n_components, void *d_workspace,
                                size_t workspace_bytes, void *stream);
NRF_API size_t nrf_lattice_components_workspace_bytes(int nx, int ny, int nz);
NRF_API int nrf_lattice_components(const uint8_t *d_mask, int nx, int ny, int nz, int connectivity, int32_t *d_labels, int64_t *n_components, void *d_workspace,
                                   size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Depth fusion (tsdf.hip; no counterpart in the reference)
 * ------------------------------------------------------------------------------------------- */
/* A truncated signed distance volume (TSDF) on the lattice of nrf_density_grid (P = bmin + (float)i * step, step = (bmax - bmin) / (float)(n - 1) per axis, x fastest,
 * nx, ny, nz >= 2; bbox[6] on the host), fused from rendered depth: d_tsdf [nz][ny][nx] fp32 (initial value 1), d_weight [nz][ny][nx] fp32 (initial value 0) and an
 * optional d_color [4][nz][ny][nx] (planes r, g, b and the colour weight cw; initial value 0).  Its level 0 is the surface (outside positive): -tsdf is a lattice for
 * nrf_isosurface_*.  None of the three entries takes a workspace, synchronises the stream or uses atomics; two runs give the same bits.
 * One observation: d_depth [h,w] (the ray parameter of nrf_get_rays' directions, camera-space z = -1: the depth map of a non-NDC render), d_acc [h,w] or NULL, d_rgb
 * [h,w,3] or NULL, the K and c2w the view was rendered with. */
typedef struct {
    const float *d_depth;
    const float *d_acc;
    const float *d_rgb;
    int h, w;
    float K[9];
    float c2w[12];
} nrf_tsdf_view;
/* nrf_tsdf_integrate: every lattice point takes the n_views views (a HOST array) in array order; each source-level fp32 operation below is rounded once.
 *   1. q = P - t (t = column 3 of c2w); xc = (R00*qx + R10*qy) + R20*qz, yc and zc the same with columns 1 and 2 of R; zd = -zc; the view is skipped unless zd > 0.
 *   2. u = fx*(xc/zd) + cx, v = cy - fy*(yc/zd) (the inverse of nrf_get_rays); fu = floorf(u + 0.5f), fv = floorf(v + 0.5f); skipped unless 0 <= fu < w and
 *      0 <= fv < h, compared as floats (NaN and huge values skip); the pixel is ((int)fu, (int)fv).
 *   3. d = depth[pixel].  With d_acc, a = acc[pixel]: a >= acc_min: d = d / a (the expected depth of what the ray hit); else a < acc_min and carve: a background
 *      observation, s = 1, no colour, on at step 5; otherwise (NaN a; a < acc_min without carve) skipped.  Skipped unless d is finite and d > 0.
 *   4. sdf = d - zd; skipped if sdf < -trunc; s = fminf(1, sdf / trunc).
 *   5. Wn = W + 1; D = (D*W + s) / Wn; W = fminf(Wn, max_weight).
 *   6. With d_color and d_rgb, after step 4 and where fabsf(sdf) <= trunc: cn = cw + 1; c = (c*cw + rgb) / cn per channel; cw = fminf(cn, max_weight).
 * Any n_views (0: NRF_OK, nothing done); up to 16 views per launch, their cameras in the kernel arguments: no device allocation, no copy, and one call over V views gives
 * the bits of V calls of one view each.  Per launch the volume moves 8 B per lattice point (40 B with d_color).  NRF_ERR_INVALID_ARG, nothing launched: a null
 * d_tsdf / d_weight / bbox / d_depth, n < 2 on an axis, h or w < 1, trunc or acc_min not finite or <= 0, max_weight < 1 (or NaN), a box with max <= min.
 * nrf_tsdf_observed: d_ok[i] = 1 iff weight > 0 at all 27 lattice points r + {-1,0,1}^3 (indices clamped into the lattice), r = (int)floorf(g + 0.5f),
 *   g = (pt - bmin) / step per axis, of d_pts [p,3]; a non-finite coordinate gives 0.  (floorf(g + 0.5f) is clamped to [-1, n] before the conversion, which changes
 *   no result.)  The band a surface was seen in: the zero level between the observed band behind a surface and the never-observed interior is no surface.
 * nrf_tsdf_sample_color: d_rgb [p,3] = the colour volume at d_pts, trilinear over the corners that hold a colour: i0 = clamp((int)floorf(g), 0, n-2) (clamped as a
 *   float, NaN as 0), f = fminf(fmaxf(g - (float)i0, 0), 1) per axis; corner weight (wx*wy)*wz, each factor f or 1 - f, corners in the order bit 0 = x, bit 1 = y,
 *   bit 2 = z; den = sum of the weights, num = sum of weight * c, both over the corners with cw > 0 and added in that order from 0; num / den, or 0 where den == 0. */
NRF_API int nrf_tsdf_integrate(float *d_tsdf, float *d_weight, float *d_color, int nx, int ny, int nz, const float *bbox, const nrf_tsdf_view *views, int n_views,
                               float trunc, float acc_min, float max_weight, int carve, void *stream);
NRF_API int nrf_tsdf_observed(const float *d_weight, int nx, int ny, int nz, const float *bbox, const float *d_pts, int64_t p, uint8_t *d_ok, void *stream);
NRF_API int nrf_tsdf_sample_color(const float *d_color, int nx, int ny, int nz, const float *bbox, const float *d_pts, int64_t p, float *d_rgb, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Mesh rasteriser (raster.hip; no counterpart in the reference)
 * ------------------------------------------------------------------------------------------- */
/* A deterministic z-buffer of a triangle list seen through the camera of nrf_get_rays (K [9] and c2w [12] on the HOST, as there): d_verts [V,3] fp32, d_faces [F,3]
 * int32 (counter-clockwise seen from outside), d_attr [V,n_attr] fp32 or NULL -> d_depth [h,w] (required), d_face [h,w] int32 or NULL, d_bary [h,w,3] or NULL,
 * d_out_attr [h,w,n_attr], d_stats [4] uint32 or NULL (ADDED to; the caller zeroes it).  0 <= F <= 2^31 - 2, 0 <= V < 2^31, 1 <= h, w <= NRF_RASTER_GUARD.
 * The call synchronises nothing and allocates nothing; two runs give the same bits, and any permutation of the face list gives the same depth bits.
 * Each source-level fp32 operation below is rounded once; the edge functions are int64 and exact.
 *   1. Per vertex: q = P - t (t = column 3 of c2w); xc = (R00*qx + R10*qy) + R20*qz, yc and zc the same with columns 1 and 2 of R; zd = -zc; u = fx*(xc/zd) + cx,
 *      v = cy - fy*(yc/zd) (steps 1-2 of nrf_tsdf_integrate without the pixel rounding).  Pixel centres sit at integer (u, v); zd is the ray parameter of
 *      nrf_get_rays' directions, the unit of DepthMap / AccMap.
 *   2. A face is CLIPPED (skipped whole; no polygon clipping) unless all three vertices have zd > near_z, fabsf(u) <= GUARD and fabsf(v) <= GUARD, compared as floats
 *      (NaN and +-inf clip).  A face with an index outside [0, V) is BAD: skipped before anything of it is dereferenced.
 *   3. X = (int)rintf(u * 256.0f), Y = (int)rintf(v * 256.0f) (round half to even).
 *   4. In int64, E_ab(p) = (bx-ax)*(py-ay) - (by-ay)*(px-ax); e0 = E_12(p), e1 = E_20(p), e2 = E_01(p) at the pixel centre p = (256 i, 256 j); A = E_01(v2).
 *      A == 0 is DEGENERATE: skipped.  cull == 1 draws front faces only: v grows downward, so a face that is counter-clockwise seen from outside has A < 0, and a
 *      face with A > 0 is CULLED.  cull == 0 draws both.
 *   5. s = sign(A).  Pixel (i, j) is inside iff for each edge k: s*e_k > 0, or s*e_k == 0 and the edge is top-left.  Edge k runs v1->v2, v2->v0, v0->v1 for
 *      k = 0, 1, 2; with (dx, dy) = s*(b - a) it is top-left iff dy < 0 || (dy == 0 && dx > 0).  Pixels visited: columns ceil(minX/256) .. floor(maxX/256) clamped
 *      to [0, w-1], rows likewise with Y and h.
 *   6. b_k = (float)((double)(s*e_k) / (double)(s*A)); r_k = 1.0f / zd_k; p_k = b_k * r_k; S = (p0 + p1) + p2; depth = 1.0f / S (perspective-correct).
 *   7. key = ((uint64)float_bits(depth) << 32) | face index; the pixel keeps the minimum key: the nearest face, and at an exact depth tie the lowest index.
 *   8. Resolve, a pass of its own: a hit pixel takes depth and face from the key, b_k recomputed by the same expressions, and
 *      attr_c = ((p0*a0c + p1*a1c) + p2*a2c) / S; a pixel no face covers gets depth 0, face -1, bary 0, attributes 0.
 *   9. d_stats += {drawn, clipped, degenerate or culled, bad index}: the four counts of one call sum to F.
 * A face whose clamped bounding box holds more than NRF_RASTER_WIDE_PIXELS pixels is rasterised by a whole workgroup (same arithmetic, same bits).
 * NRF_ERR_INVALID_ARG, message starting "nrf_raster_mesh", nothing launched or written: a null d_depth; a null d_verts, d_faces, K or c2w with F > 0; h or w < 1 or
 * > GUARD; n_attr < 0 or > NRF_RASTER_MAX_ATTR; n_attr > 0 with a null d_attr or d_out_attr; near_z not finite or <= 0; cull not 0 or 1; F or V out of range; a
 * workspace that is null or smaller than nrf_raster_workspace_bytes (0 for a shape the call refuses).  F == 0 is valid and writes the background. */
#define NRF_RASTER_SUBPIXEL 256          /* fixed-point steps per pixel */
#define NRF_RASTER_GUARD 16384           /* |u|, |v| beyond this clip the face; also the largest h or w */
#define NRF_RASTER_MAX_ATTR 8
#ifndef NRF_RASTER_WIDE_PIXELS           /* tuning builds set another (make EXTRA=-DNRF_RASTER_WIDE_PIXELS=n); no result depends on it */
#define NRF_RASTER_WIDE_PIXELS 256       /* bounding-box pixel count above which a face goes to the wide kernel */
#endif
NRF_API size_t nrf_raster_workspace_bytes(int64_t n_verts, int64_t n_faces, int h, int w);
NRF_API int nrf_raster_mesh(const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, const float *d_attr, int n_attr, int h, int w,
                            const float *K, const float *c2w, float near_z, int cull, float *d_depth, int32_t *d_face, float *d_bary, float *d_out_attr,
                            uint32_t *d_stats, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Geometry in space (geometry.hip; no counterpart in the reference)
 * ------------------------------------------------------------------------------------------- */
/* Comparing two surfaces in 3D: points drawn on a triangle list in proportion to area, the nearest point of one set for every point of another, and the sums that
 * Chamfer distance, Hausdorff distance and precision / recall at a distance are made of.  Each source-level fp32 operation below is rounded once; sqrtf and / are
 * correctly rounded.  Every entry takes a caller-owned workspace sized by its *_workspace_bytes twin (0 for a shape the entry refuses) and allocates nothing.  Only
 * nrf_mesh_sample_count synchronises the stream.  Refusals -- NRF_ERR_INVALID_ARG, or NRF_ERR_WORKSPACE for a workspace below the twin's size, the message starting
 * with the entry's name -- come before any launch or write.  Two runs of any entry give the same bits.
 *
 * Surface sampling: d_verts [V,3] fp32, d_faces [F,3] int32, 0 <= V, F < 2^31; density (points per unit area) finite and >= 0; a count call, then an emit call over
 * the same mesh, seed and workspace.
 *   1. Per face f: e1 = v1 - v0, e2 = v2 - v0 per component; c = e1 x e2 with every component fl(fl(a*b) - fl(c*d)): cx = e1y*e2z - e1z*e2y, cy = e1z*e2x - e1x*e2z,
 *      cz = e1x*e2y - e1y*e2x; s = (cx*cx + cy*cy) + cz*cz; area = 0.5f * sqrtf(s).
 *   2. a = area * density; n_f = (int)floorf(a) + (nrf_rng_uniform(seed, NRF_RNG_SURFACE_COUNT, f) < a - floorf(a)): the expectation of n_f is a.
 *   3. A face with an index outside [0, V) is BAD: n_f = 0, nothing of it is dereferenced.  A face with a non-finite vertex coordinate or a non-finite area is
 *      NON-FINITE: n_f = 0.  Neither enters the area.  n_f > NRF_SAMPLE_MAX_PER_FACE is CLAMPED to that constant.  d_stats [3] uint32 or NULL (ADDED to; the caller
 *      zeroes it) += {bad, non-finite, clamped}.
 *   4. The first point of face f is the exclusive integer prefix sum of n_f over the faces in order; *n_points is the total.  *total_area is the fp64 sum of
 *      (double)area over the faces that are neither bad nor non-finite, added in this order: blocks of 256 consecutive faces; within a block the 64 values of each of
 *      the 4 waves by the butterfly v += v[lane ^ o], o = 32, 16, 8, 4, 2, 1, then ((w0 + w1) + w2) + w3; the block sums b_k: thread t of 256 adds k = t, t + 256, ...
 *      in ascending order from 0.0, then s[t] += s[t + o] for t < o, o = 128, 64, ..., 1.  No atomics.
 *   5. nrf_mesh_sample_count returns both values to the host (the one synchronisation).  A total of 2^31 or more: NRF_ERR_INVALID_ARG, the message says so (the
 *      area is still returned).  density == 0 is valid: the area and zero points.  F == 0: zero points, area 0.
 *   6. nrf_mesh_sample_emit, for point p (global index) of face f: u = nrf_rng_uniform(seed, NRF_RNG_SURFACE_UV, 2p), v = nrf_rng_uniform(seed, NRF_RNG_SURFACE_UV,
 *      2p + 1); if u + v > 1.0f then u = 1.0f - u, v = 1.0f - v; P = (v0 + u*e1) + v*e2 per component.  d_points [n,3]; d_face [n] int32 or NULL gets f; d_uv [n,2] or
 *      NULL gets (u, v) after the reflection: P is the barycentric combination (1-u-v, u, v) of the face's corners.  n_points is the count call's; the kernel writes no
 *      point beyond it nor beyond the count call's own total (kept in the workspace), so a wrong n_points cannot overrun a buffer.
 *
 * Nearest points: d_query [nq,3], d_target [nt,3] fp32, 0 <= nq, nt < 2^31 -> d_dist2 [nq] fp32, d_index [nq] int32.
 *   CONTRACT.  d2(q, j) = (dx*dx + dy*dy) + dz*dz with dx = qx - tx and likewise y, z.  For a finite query the result is the minimum of the key
 *   ((uint64)float_bits(d2) << 32) | j over all finite targets j with d2 <= fl(max_dist * max_dist); max_dist >= 0, +inf for no limit.  So: the nearest target, on an
 *   exact tie the lowest index, the same bits whatever the grid, the order of the targets or the scheduling.  No such target: d2 = +inf, index = -1; a non-finite query
 *   gets the same.  A d2 that overflows to +inf with a valid index is a valid answer.  d_stats [3] uint32 or NULL (ADDED to) += {non-finite queries, non-finite targets,
 *   queries served by the fallback below}.  nt == 0 is valid; nq == 0 is valid and launches nothing.
 *   MECHANISM.  A uniform grid of nx * ny * nz cells over bbox[6] (HOST values: min xyz, max xyz; max > min, finite), x fastest; 1 <= nx, ny, nz <= NRF_NN_MAX_DIM and
 *   nx * ny * nz <= NRF_NN_MAX_CELLS.  Per axis inv_h = (float)n / (bmax - bmin), h = 1.0f / inv_h, and the cell coordinate of x is
 *   clamp((int)floorf((x - bmin) * inv_h), 0, n - 1): a point outside the box lives in a border cell, which therefore extends outward without bound.  Finite targets
 *   are counted per cell (integer atomics), the counts scanned, and the targets scattered into cell order as 16-byte records {x, y, z, index}; the order inside a
 *   cell may vary from run to run, the key minimum does not depend on it.  One lane per query scans ring r = 0, 1, ... of cells (Chebyshev distance r from the
 *   query's cell, clamped to the grid) and after ring r stops iff every cell has been scanned, or min(best_d2, fl(max_dist * max_dist)) < fl(B * B), strictly, with
 *   B = fl(fl((float)r * h_min) * 0.999f), h_min the smallest of the three h.
 *   WHY THE STOP IS EXACT.  Let tau(x) = (x - bmin) * inv_h in real arithmetic.  The computed value is fl(fl(x - bmin) * inv_h): two roundings, so for a coordinate
 *   whose computed cell is k (unclamped, or clamped at a border) tau >= k - e resp. tau < k + 1 + e with e <= 1024 * 2^-23 < 1.3e-4 (dims <= 1024).  A target not yet
 *   scanned after ring r sits in a cell at least r + 1 cells from the query's cell along some axis, so on that axis the real separation is at least
 *   (r - 2e) / inv_h >= r * (1 - 2.6e-4) / inv_h, for points in the outward-extending border cells too (they only lie farther out).  B is at most
 *   r * h_min * 0.999 * (1 + 2^-23), and h_min <= (1 / inv_h) * (1 + 2^-24) on every axis: B is a float no larger than that separation.  Rounding of -, * and + is
 *   monotone: |fl(qx - tx)| >= B, its square is >= fl(B * B), and adding the other two non-negative squares keeps that.  Every unscanned target therefore has
 *   d2 >= fl(B * B): it can neither beat nor tie a strictly smaller best, and once fl(B * B) exceeds fl(max_dist * max_dist) none of them counts.
 *   FALLBACK.  A query with no stop after ring NRF_NN_MAX_RINGS (an outlier, a sparse set, a query far outside the box) is appended to a list in the workspace; a second
 *   kernel, a fixed grid of workgroups striding the list by the count read on the device, brute-forces ALL records for each such query with a block-wide minimum of the
 *   key.  Both kernels form d2 through one inline function.  Every loop is bounded by a clamped range or a count; nothing waits on another workgroup.
 *
 * Distance statistics: d_dist2 [n] fp32 (0 <= n < 2^40), taus [n_tau] on the HOST (0 <= n_tau <= NRF_STATS_MAX_TAU, each finite and >= 0) -> d_out [4 + n_tau]
 * doubles on the device: over the FINITE entries, with d = sqrtf(d2) in fp32, {count, sum of (double)d, sum of (double)d2, max of d (0 where none), count(d <= tau_k)
 * ...}.  A +inf entry ("none within max_dist") is left out of the sums and is a miss for every tau; divide by n, not by count, for a recall.  Order: blocks of 4096
 * entries, lane t of 256 takes entries t, t + 256, ... in ascending order from 0.0; then the wave butterfly, the four wave sums and the ordered pass of step 4 above.
 * n == 0 gives zeros.  No synchronisation. */
#define NRF_SAMPLE_MAX_PER_FACE 65536    /* the most points one face receives */
#define NRF_NN_MAX_DIM 1024              /* the largest grid dimension: the stop rule's slack (0.999f) is proved for dims up to this */
#define NRF_NN_MAX_CELLS (1 << 26)       /* the largest nx * ny * nz: 4 B per cell twice over in the workspace */
#ifndef NRF_NN_MAX_RINGS                 /* tuning builds set another (make EXTRA=-DNRF_NN_MAX_RINGS=n); no result depends on it */
#define NRF_NN_MAX_RINGS 16              /* the last ring a query scans before it goes to the brute-force list */
#endif
#define NRF_STATS_MAX_TAU 4
NRF_API size_t nrf_mesh_sample_workspace_bytes(int64_t n_verts, int64_t n_faces);
NRF_API int nrf_mesh_sample_count(const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, float density, uint64_t seed, int64_t *n_points,
                                  double *total_area, uint32_t *d_stats, void *d_workspace, size_t workspace_bytes, void *stream);
NRF_API int nrf_mesh_sample_emit(const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, uint64_t seed, int64_t n_points, float *d_points,
                                 int32_t *d_face, float *d_uv, void *d_workspace, size_t workspace_bytes, void *stream);
NRF_API size_t nrf_nearest_points_workspace_bytes(int64_t nq, int64_t nt, int nx, int ny, int nz);
NRF_API int nrf_nearest_points(const float *d_query, int64_t nq, const float *d_target, int64_t nt, const float *bbox, int nx, int ny, int nz, float max_dist,
                               float *d_dist2, int32_t *d_index, uint32_t *d_stats, void *d_workspace, size_t workspace_bytes, void *stream);
NRF_API size_t nrf_distance_stats_workspace_bytes(int64_t n);
NRF_API int nrf_distance_stats(const float *d_dist2, int64_t n, const float *taus, int n_tau, double *d_out, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Mesh simplification (simplify.hip; no counterpart in the reference)
 * ------------------------------------------------------------------------------------------- */
/* Vertex clustering on a uniform grid: the vertices of a cell become one vertex, faces that lose a corner to a neighbour disappear, and of several faces that land on
 * the same three cells at most one survives, chosen by their net orientation.  d_verts [V,3] fp32, d_faces [F,3] int32; bbox[6] HOST values (min xyz, max xyz); a count
 * call, then an emit call over the same mesh, box, dims and workspace.  Each source-level fp32 operation below is rounded once; / is correctly rounded.  The
 * workspace is caller-owned, 8-byte aligned and sized by nrf_mesh_simplify_workspace_bytes (0 for a shape the entries refuse); nothing is allocated.  Refusals --
 * NRF_ERR_INVALID_ARG, or NRF_ERR_WORKSPACE for a workspace below the twin's size, the message starting with the entry's name -- come before any launch or write.
 * Two runs give the same bits, whatever the workspace held before.
 *   1. GRID.  0 <= V, F < 2^31; 1 <= nx, ny, nz <= NRF_SIMPLIFY_MAX_DIM; nx * ny * nz <= NRF_SIMPLIFY_MAX_CELLS; the box finite with max > min.  Per axis
 *      inv_h = (float)n / (bmax - bmin) and h = 1.0f / inv_h (as nrf_nearest_points forms them).  For a finite vertex t = (x - bmin) * inv_h and
 *      c = clamp((int)floorf(t), 0, n - 1); its cell is cx + nx * (cy + ny * cz).  A vertex with a non-finite coordinate has no cell.
 *   2. FACES.  Each face falls into the first class that applies: an index outside [0, V): BAD, nothing of it is dereferenced; a corner without a cell: NON-FINITE;
 *      two corners in one cell: COLLAPSED; the rest are candidates, each with a triple of three distinct cells (c0, c1, c2) in corner order.  A vertex is USED if it
 *      is a corner of a face that is neither BAD nor NON-FINITE.
 *   3. COINCIDENT FACES.  Sort a candidate's triple to (a < b < c); the face is EVEN if (c0, c1, c2) is a rotation of (a, b, c) and ODD otherwise.  For each distinct
 *      sorted triple net = #even - #odd over all candidates with it.  net == 0: none is kept; net > 0: the even candidate of lowest face index; net < 0: the odd
 *      candidate of lowest face index.  Every candidate not kept is REMOVED.  (Two sheets pressed onto the same three cells with opposite windings cancel, and a
 *      pocket folded onto itself leaves no fin.)  d_stats [4] uint32 or NULL (ADDED to; the caller zeroes it) += {bad, non-finite, collapsed, removed}.
 *   4. OUTPUT ORDER.  Kept faces are emitted in ascending input face index; d_face_src [n_out_faces] or NULL gets that index.  An output vertex exists for every cell
 *      that is a corner of a kept face; output vertices are numbered in ascending cell index.  Neither order depends on scheduling, on the hash table or on the order
 *      of the input vertices.  d_out_faces [n_out_faces,3] holds the output ids of (c0, c1, c2) in the face's own corner order: winding is preserved.  d_cluster [V]
 *      or NULL: the output id of v's cell, -1 if the cell has no output vertex or v has no cell.
 *   5. POSITION.  The members of an output vertex are the USED vertices of its cell.  Per member and axis o = clamp(t - (float)c, 0.0f, 1.0f) and
 *      q = (int64)(o * 1048576.0f); S is the int64 sum of q and m the member count (integer atomics: the order does not matter).
 *      tm = (float)((double)c + ((double)S / (double)m) * 2^-20) and P = bmin + tm * h.
 *   6. REPRESENTATIVE.  Per member d2 = (dx*dx + dy*dy) + dz*dz with dx = x - Px and likewise y, z; d_rep [n_out_verts] or NULL gets the low word of the minimum of
 *      the key ((uint64)float_bits(d2) << 32) | v: the member nearest the mean, on a tie the lowest index.  position == NRF_SIMPLIFY_POS_MEAN writes P to
 *      d_out_verts [n_out_verts,3], NRF_SIMPLIFY_POS_MEMBER the representative's own coordinates; any other value is refused.
 * nrf_mesh_simplify_count runs steps 1-4 and returns the two totals (its one synchronisation); they stay in the workspace.  nrf_mesh_simplify_emit takes them as the
 * sizes of the caller's buffers: it reads the workspace's pair back (it waits for the stream once, as nrf_isosurface_emit does) and refuses any other pair before
 * anything is written, so a wrong total can neither overrun a buffer nor leave one half filled.  V == 0 or F == 0 is valid and gives 0 / 0.
 * MECHANISM.  An open-addressing table of a power-of-two number of slots >= 2F, slot = {owner face, net, lowest even face, lowest odd face}.  The owner is set once by
 * a compare-and-swap from EMPTY and never changes; the slot's key is the sorted triple of its owner, read from per-face triples an EARLIER launch wrote, so no
 * multi-word key is ever published.  A face that meets a slot whose owner has its key adds +-1 to net and lowers its parity's minimum, otherwise it probes the next
 * slot; the walk is bounded by the slot count.  A second launch reads the finished slots.  Positions come from integer prefix sums over faces and over cells.  No
 * output depends on the hash function, the table size or the arrival order, and nothing waits on another workgroup. */
#define NRF_SIMPLIFY_MAX_DIM 1024
#define NRF_SIMPLIFY_MAX_CELLS (1 << 27)
#define NRF_SIMPLIFY_POS_MEAN 0
#define NRF_SIMPLIFY_POS_MEMBER 1
NRF_API size_t nrf_mesh_simplify_workspace_bytes(int64_t n_verts, int64_t n_faces, int nx, int ny, int nz);
NRF_API int nrf_mesh_simplify_count(const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, const float *bbox, int nx, int ny, int nz,
                                    int64_t *n_out_verts, int64_t *n_out_faces, uint32_t *d_stats, void *d_workspace, size_t workspace_bytes, void *stream);
NRF_API int nrf_mesh_simplify_emit(const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, const float *bbox, int nx, int ny, int nz, int position,
                                   int64_t n_out_verts, int64_t n_out_faces, float *d_out_verts, int32_t *d_out_faces, int32_t *d_rep, int32_t *d_face_src,
                                   int32_t *d_cluster, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Image metrics (image_metrics.hip; the reference has only the training loop's PSNR, NeRFExecutor.h:893)
 * ------------------------------------------------------------------------------------------- */
/* How good a frame is, on the device and in fp64 (in fp32 the variances E[x^2] - mu^2 cancel against c2: a flat pair 0.25 / 0.75 is off by 1.19e-4).  Images are
 * [b,h,w,c] fp32 contiguous (the layout of RGBMap), c in 1..4, h and w >= 11, b * c <= 65535; data_range L finite and > 0.
 *   nrf_ssim_window: HOST.  The 11 weights every kernel here uses: g[k] = exp(-(k-5)^2 / 4.5) (sigma 1.5) divided by the sum of the 11 values added in order k = 0..10.
 *   nrf_ssim: Wang et al. 2004 over the VALID region (h-10) x (w-10), per channel, every op a double op rounded once, in this order:
 *     c1 = (0.01 L) * (0.01 L), c2 = (0.03 L) * (0.03 L); the five planes x, y, x*x, y*y, x*y are filtered along the row first, then along the column, each 11-tap sum
 *     as acc = g[0] * a[0]; acc = acc + g[k] * a[k], k = 1..10 -> mx, my, exx, eyy, exy;
 *     mxx = mx*mx, myy = my*my, mxy = mx*my; sxx = exx - mxx, syy = eyy - myy, sxy = exy - mxy;
 *     cs = (2*sxy + c2) / ((sxx + syy) + c2); lum = (2*mxy + c1) / ((mxx + myy) + c1); ssim = lum * cs.
 *     d_means [b,c,2]: the mean of ssim and the mean of cs over the valid region.  d_map (optional) [b,h-10,w-10,c]: ssim per pixel -- a numpy float64 restatement of
 *     the order above equals it bit for bit.  The sums are fp64 tile partials in the workspace combined in one ordered pass, no atomics: two runs give the same bits, an
 *     image's means do not depend on the batch it came in, and they are the same with and without d_map.
 *   nrf_image_mse: d_mse [b] = the mean over an image's elems_per_image values of ((double)x - (double)y)^2; the same ordered reduction.
 *   nrf_ms_ssim: d_means [scales,b,c,2], 1 <= scales <= 5 and min(h, w) >> (scales - 1) >= 11.  Scale 0 is nrf_ssim's computation; each further scale first pools both
 *     images 2 x 2 in double, ((a00 + a01) + (a10 + a11)) * 0.25 (an odd trailing row or column is dropped; the pooled planes stay in the workspace as doubles), then
 *     runs the same computation on them.  Combining the scales is the caller's (nerfpp_amd/metrics.py: MSSSIM).
 * A bad shape, c, data_range, scales or a null pointer: NRF_ERR_INVALID_ARG; a workspace below the *_workspace_bytes twin: NRF_ERR_WORKSPACE.  A refusal
 * launches nothing and writes nothing.  No entry synchronises. */
NRF_API int nrf_ssim_window(double *out11);
NRF_API size_t nrf_ssim_workspace_bytes(int b, int h, int w, int c);
NRF_API int nrf_ssim(const float *d_x, const float *d_y, int b, int h, int w, int c, double data_range, double *d_means, double *d_map, void *d_workspace,
                     size_t workspace_bytes, void *stream);
NRF_API size_t nrf_image_mse_workspace_bytes(int b, int64_t elems_per_image);
NRF_API int nrf_image_mse(const float *d_x, const float *d_y, int b, int64_t elems_per_image, double *d_mse, void *d_workspace, size_t workspace_bytes, void *stream);
NRF_API size_t nrf_ms_ssim_workspace_bytes(int b, int h, int w, int c, int scales);
NRF_API int nrf_ms_ssim(const float *d_x, const float *d_y, int b, int h, int w, int c, double data_range, int scales, double *d_means, void *d_workspace,
                        size_t workspace_bytes, void *stream);

/* SSIM as a training loss: d_loss [2] = {1 - m, m}, m = the mean of nrf_ssim's ssim over ALL n = b * (h-10) * (w-10) * c valid values, and the gradient of
 * 1 - m with respect to x.  Images as above (the domain of nrf_ssim); weight finite and >= 0.  d_g_x [b,h,w,c] fp32 is ACCUMULATED into; d_grad64 (optional)
 * [b,h,w,c] is written.  Every op is a double op rounded once, in this order:
 *   1. mx, my, exx, eyy, exy, mxx, myy, mxy, sxx, syy, sxy, cs, lum, ssim as nrf_ssim states them; cd = (sxx + syy) + c2 and ld = (mxx + myy) + c1 are its denominators;
 *   2. per valid pixel  A = cs * (2*(my - lum*mx)/ld) + lum * (2*(cs*mx - my)/cd),  B = -(ssim/cd),  Cc = 2*lum/cd;
 *   3. the transposed window T(M) along one axis, M padded with 10 zeros on both sides: acc = g[0]*M[p]; acc = acc + g[k]*M[p-k], k = 1..10 -- along the column
 *      (image rows) first, then along the row: [h-10, w-10] -> [h, w];
 *   4. grad64 = -(((T(A) + 2*x*T(B)) + y*T(Cc))) / n, n as a double;  g_x[i] = g_x[i] + (float)(weight * grad64[i]); weight == 0 leaves g_x alone.
 * A numpy float64 restatement of this order equals d_grad64 by value (tests/ssim_loss_ref.py).  No atomics: the sum is fp64 workgroup partials in the workspace added in
 * one ordered pass, every gradient element has one writer; two runs give the same bits, the result is the same with and without d_grad64, and an image's
 * grad64 * n does not depend on the other images of the batch.  Refusals and the workspace as for the entries above. */
NRF_API size_t nrf_ssim_loss_workspace_bytes(int b, int h, int w, int c);
NRF_API int nrf_ssim_loss(const float *d_x, const float *d_y, int b, int h, int w, int c, double data_range, double weight, double *d_loss, float *d_g_x,
                          double *d_grad64, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Texture atlases (texture.hip; no counterpart in the reference)
 * ------------------------------------------------------------------------------------------- */
/* A per-face texture atlas: every face of a triangle list owns a right triangle of T x T / 2 texels of one image, so the resolution of the colour does not depend on
 * the face count.  Meant for meshes whose faces are of nearly one size (nrf_mesh_simplify_*).  The layout is integer arithmetic on (F, T) alone; no entry takes a
 * workspace, allocates, synchronises or uses atomics; each source-level fp32 operation below is rounded once, sqrtf and / are correctly rounded; two runs give the
 * same bits.  Refusals -- NRF_ERR_INVALID_ARG, the message starting with the entry's name -- come before any launch or write.
 *
 * LAYOUT of (F, T), F faces and a tile of T texels, NRF_ATLAS_MIN_TILE <= T <= NRF_ATLAS_MAX_TILE, 0 <= F <= 2^31 - 2:
 *   cells = (F + 1) / 2 (integer division); cols = the smallest integer with cols * cols >= cells; rows = (cells + cols - 1) / cols (0 where cells == 0);
 *   width = cols * T, height = rows * T.  The atlas is [height, width, C], row-major, texel (X, Y) in column X of row Y.
 *   Texel (X, Y) lies in cell (X / T) + cols * (Y / T) at the local indices i = X % T, j = Y % T.  Face f lives in cell f >> 1.  The texels of a cell with
 *   i + j <= T - 2 belong to its LOWER face 2 * cell, and (i, j) are that face's indices; the others belong to its UPPER face 2 * cell + 1, whose indices are the
 *   mirrored (T - 1 - i, T - 1 - j), so i + j <= T - 1 there.  A texel whose face is >= F (the upper half of the last cell of an odd F, the cells past the last face)
 *   has no owner.  Every texel has at most one owner.
 *   With n = T - 3 the corners 0, 1, 2 of a face sit at the centres of its texels (0, 0), (n, 0), (0, n): the texel with the face's indices (i, j) has the
 *   barycentrics b1 = (float)i / (float)n, b2 = (float)j / (float)n, b0 = (1.0f - b1) - b2.  Owned texels with i + j > n extrapolate in the plane of the face: they
 *   are the padding, and there is no dilation pass.  A bilinear footprint at a point of the face reads only texels with i + j <= n + 1 = T - 2, all of them the
 *   face's own in either half of a cell (tests/test_texture_host.py).
 * nrf_atlas_dims (host only): *width, *height of (n_faces, tile).  Refused: a tile outside [MIN, MAX], n_faces < 0 or > 2^31 - 2, a null pointer, a side above
 *   NRF_ATLAS_MAX_SIZE -- the message names 2 * (NRF_ATLAS_MAX_SIZE / tile)^2, the number of faces that fit.  F == 0 gives 0 x 0.
 *
 * nrf_atlas_texels: what to bake.  d_verts [V,3] fp32, d_faces [F,3] int32, d_normals [V,3] or NULL, 0 <= V < 2^31; one lane per texel of the atlas rows
 *   [row0, row0 + rows) (0 <= row0, 0 <= rows, row0 + rows <= height; rows == 0 does nothing) -> d_face [rows,width] int32 (required), d_bary [rows,width,3],
 *   d_pos [rows,width,3], d_rays [rows,width,11], each of the three or NULL.  A slab holds the bits of the same rows of a whole run.
 *   1. The owner f and the face's indices (i, j) by the layout; no owner: face -1.
 *   2. (v0, v1, v2) = d_faces[f]; an index outside [0, V): face -1, before anything of the face is dereferenced.
 *   3. e1 = v1 - v0, e2 = v2 - v0 per component; c = e1 x e2 with every component fl(fl(a*b) - fl(c*d)) as in nrf_mesh_sample_count step 1;
 *      s = (cx*cx + cy*cy) + cz*cz; len = sqrtf(s); unless len > 0 (as floats: zero and NaN fail) the face is degenerate: face -1.
 *   4. b1, b2, b0 as above; P = v0 + (b1*e1 + b2*e2) per component.
 *   5. N = c / len per component.  With d_normals: m = (b0*n0 + b1*n1) + b2*n2 per component, l = sqrtf((mx*mx + my*my) + mz*mz), and where l > 0, N = m / l.
 *   6. The ray, in the [n,11] form of nrf_pack_rays: origin P + offset*N, direction -N, near 0, far 2.0f*offset, view direction -N: a camera `offset` above the
 *      surface looking down the normal, through the surface to `offset` below it.
 *   7. A texel with face -1 gets zeros in d_bary, d_pos and d_rays.
 *   Refused: what nrf_atlas_dims refuses; V out of range; a null d_face with rows > 0; a null d_verts (with V > 0) or d_faces with F > 0; offset not finite or < 0;
 *   a row window outside the atlas.
 *
 * nrf_texture_sample: d_tex [height,width,C] of (n_faces, tile), 1 <= C <= NRF_TEXTURE_MAX_CHANNELS, at p >= 0 pairs of d_face [p] int32 and d_bary [p,3] (b0, b1,
 *   b2: what nrf_mesh_sample_emit's d_uv and nrf_raster_mesh's d_bary hold; b0 is not read) -> d_out [p,C].
 *   1. f < 0 or f >= n_faces: zeros.
 *   2. nf = (float)n; x = b1 * nf; x = 0 unless x > 0 (NaN gives 0); x = nf if x > nf.  y from b2 likewise.
 *   3. The face's indices (i, j) name the texel (X0 + i, Y0 + j) of an even f and (X0 + T - 1 - i, Y0 + T - 1 - j) of an odd f, with cell = f >> 1,
 *      X0 = (cell % cols) * T, Y0 = (cell / cols) * T.
 *   4. NRF_TEXTURE_NEAREST: i = (int)rintf(x), j = (int)rintf(y) (round half to even); if i + j > n + 1 then j = n + 1 - i (i <= n, so j >= 1: the owned texel of
 *      column i nearest in j); out_c = tex[texel (i, j)][c].
 *   5. NRF_TEXTURE_BILINEAR: ix = floorf(x), fx = x - ix, iy = floorf(y), fy = y - iy; gx = 1.0f - fx, gy = 1.0f - fy.  The corners (ix, iy), (ix + 1, iy),
 *      (ix, iy + 1), (ix + 1, iy + 1) carry the weights gx*gy, fx*gy, gx*fy, fx*fy; out_c starts at 0.0f and takes out_c = out_c + w * tex[corner][c] in that
 *      order.  A corner whose indices have i + j > n + 1 is NOT READ and its term is left out: at a point of the face its weight is 0 in exact arithmetic, and the
 *      texel belongs to a neighbour or to nobody, so whatever it holds (a NaN, too) never reaches the result.
 *   Refused: what nrf_atlas_dims refuses; C out of range; a filter that is neither constant; p < 0; with p > 0 a null d_face, d_bary or d_out, or a null d_tex
 *   where the atlas is not empty.  With n_faces == 0 every output is 0.
 *
 * nrf_texture_shade: deferred texturing of a nrf_raster_mesh result: d_face_map [h,w] int32 and d_bary_map [h,w,3] of the same d_verts, d_faces, K and c2w (HOST
 *   values, as there), the atlas of (F, tile) -> d_out [h,w,C].  Per pixel:
 *   1. f = face_map; f < 0 or f >= F, or a corner index outside [0, V): zeros.
 *   2. zd_k of the three corners by step 1 of nrf_raster_mesh, the same expressions.
 *   3. r_k = 1.0f / zd_k; p_k = b_k * r_k; S = (p0 + p1) + p2; beta_k = p_k / S: the barycentrics on the face, perspective-correct.
 *   4. nrf_texture_sample's steps 2-5 at (f, beta), by the same device function.
 *   Refused: what nrf_texture_sample refuses of (F, tile, C, filter); h or w < 1 or > NRF_RASTER_GUARD; V out of range; a null d_face_map, d_bary_map or d_out;
 *   with F > 0 a null d_verts (V > 0), d_faces, K, c2w or d_tex. */
#define NRF_ATLAS_MIN_TILE 4
#define NRF_ATLAS_MAX_TILE 64
#define NRF_ATLAS_MAX_SIZE 16384         /* the largest width or height */
#define NRF_TEXTURE_MAX_CHANNELS 8
#define NRF_TEXTURE_NEAREST 0
#define NRF_TEXTURE_BILINEAR 1
NRF_API int nrf_atlas_dims(int64_t n_faces, int tile, int *width, int *height);
NRF_API int nrf_atlas_texels(const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, const float *d_normals, int tile, float offset, int row0,
                             int rows, int32_t *d_face, float *d_bary, float *d_pos, float *d_rays, void *stream);
NRF_API int nrf_texture_sample(const float *d_tex, int64_t n_faces, int tile, int channels, const int32_t *d_face, const float *d_bary, int64_t p, int filter,
                               float *d_out, void *stream);
NRF_API int nrf_texture_shade(const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, const int32_t *d_face_map, const float *d_bary_map, int h,
                              int w, const float *K, const float *c2w, const float *d_tex, int tile, int channels, int filter, float *d_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Mesh adjacency, smoothing and vertex normals (smooth.hip; no counterpart in the reference)
 * ------------------------------------------------------------------------------------------- */
/* The inverted index of a triangle list -- per vertex its faces and its neighbours -- and the two gathers that read it.  The workspace is the caller's, 8-byte
 * aligned and sized by nrf_mesh_adjacency_workspace_bytes (0 for a refused shape); nothing is allocated; refusals -- NRF_ERR_INVALID_ARG or NRF_ERR_WORKSPACE, the
 * message starting with the entry's name -- come before any launch or write; two runs give the same bits whatever the workspace and the outputs held; each
 * source-level fp32 operation below is rounded once (no FMA contraction), / and sqrtf are correctly rounded.  V == 0 or F == 0 is valid everywhere.
 *
 * ADJACENCY of d_faces [F,3] int32 over n_verts = V vertices, 0 <= V, F < 2^31.  A face is skipped whole if it has a corner outside [0, V) (counted in stats[0];
 * nothing of it is dereferenced) or, failing that, two equal corners (stats[1]); the others are the VALID faces.  Two valid faces with the same corners are two faces.
 *   d_face_start [V+1] int64, d_face_list [n_incident] int32: row v = [d_face_start[v], d_face_start[v+1]) lists the valid faces with v as a corner in ascending face
 *     index; n_incident = 3 * (valid faces) = d_face_start[V].
 *   d_nbr_start [V+1] int64, d_nbr [n_neighbours] int32: row v lists the distinct vertices that share a valid face with v in ascending vertex index;
 *     d_nbr_faces [n_neighbours] int32, beside d_nbr: the number of valid faces that contain that edge -- 1 a boundary edge, 2 an interior edge, more a non-manifold
 *     one.  n_neighbours = d_nbr_start[V] = twice the number of undirected edges.
 *   d_flags [V] uint8: NRF_ADJ_BOUNDARY where some edge of the vertex has exactly one face, NRF_ADJ_NONMANIFOLD where some edge has more than two; 0 for a vertex
 *     no valid face uses.
 *   d_stats [8] int64, WRITTEN: {faces skipped for a bad index, faces skipped for a repeated corner, used vertices, undirected edges, boundary edges, non-manifold
 *     edges, the longest face row, the longest neighbour row}.
 *   Every output but d_face_list is the same for any order of the faces and any rotation or reflection of their corners; d_face_list is ascending in the face
 *   indices it is given.  Nothing depends on scheduling.
 * nrf_mesh_adjacency_count builds the rows in the workspace and returns the two totals (its one synchronisation).  nrf_mesh_adjacency_emit takes them as the sizes
 * of the caller's buffers: it reads the workspace's pair back (it waits for the stream once) and refuses any other pair before anything is written, as
 * nrf_mesh_simplify_emit does.  Refused besides: V or F out of range, a null d_faces with F > 0, a null or misaligned workspace, a null out-parameter; in emit
 * n_incident outside [0, 3F], n_neighbours outside [0, 6F], a null output that has elements (d_face_start, d_nbr_start and d_stats always have).
 * MECHANISM.  Degrees by integer atomics, row starts by integer prefix sums, rows filled through an integer cursor in arrival order and then sorted by rank (the
 * rank of an entry is the number of smaller ones, ties by position) -- first the faces of a row, then the 2 * len far ends of its half-edges, whose runs of equal
 * values are the neighbours and their face counts.  A row of at most NRF_ADJ_SHORT_ROW faces is sorted by one lane, a longer one by one workgroup of 256 lanes
 * (len^2 / 256 comparisons per lane: a hub of 4 096 faces is well under a millisecond's worth); the two paths run the same steps and give the same rows.
 *
 * nrf_mesh_smooth: Taubin's lambda|mu filter, or with mu == 0 the umbrella Laplacian, of d_x [V,C] fp32, 1 <= C <= NRF_SMOOTH_MAX_CHANNELS, over the neighbour rows
 *   above (d_nbr_start, d_nbr, d_nbr_faces, d_flags of the same V; n_neighbours = the length of d_nbr).  d_out [V,C] gets the result, d_tmp [V,C] is scratch (its
 *   final content is unspecified); d_x is not written.  iterations >= 0; 0 copies d_x to d_out.  One iteration is a step with factor lambda and then, if mu != 0, a
 *   step with factor mu.  One step, per vertex i and channel, from x (the previous step's values; every vertex reads the same x):
 *     1. J = the row of i in its stored order.  Under NRF_SMOOTH_CURVE a vertex with NRF_ADJ_BOUNDARY keeps only the neighbours with d_nbr_faces == 1: the boundary
 *        smooths as a curve and does not slide into the interior.  Under NRF_SMOOTH_FIXED a vertex with NRF_ADJ_BOUNDARY is copied.  An empty J copies the vertex.
 *     2. s = (..((x[j0] + x[j1]) + x[j2]) + ..), sequentially, at EVERY row length; m = s / (float)|J|; d = m - x[i]; out = x[i] + fl(f * d).
 *   Non-finite values propagate by IEEE rules (the payload of a NaN is unspecified).  One launch per step, one lane per vertex, a gather with no atomics.  An entry of
 *   d_nbr outside [0, V) and the part of a row outside [0, n_neighbours) are never dereferenced (rows of nrf_mesh_adjacency_emit have neither).  Under
 *   NRF_SMOOTH_FREE d_nbr_faces and d_flags are not read and may be NULL; NRF_SMOOTH_FIXED reads d_flags alone.
 *   Refused: V out of range, n_neighbours < 0, C, iterations < 0 or > 2^30 - 1 (the step count is an int), a lambda or mu that is not finite, a boundary mode
 *   that is none of the three; with V > 0 a null d_x, d_out, d_tmp, d_nbr_start or an array the mode reads, two of d_x, d_out, d_tmp equal, or one of them not
 *   aligned to a whole vertex (4, 8, 4, 16 bytes for C = 1 .. 4).
 *
 * nrf_mesh_vertex_normals: d_out [V,3] from d_verts [V,3], d_faces [F,3] and the face rows above (n_incident = the length of d_face_list).  Per face with corners
 *   (a, b, c) in the face's own order: e1 = b - a, e2 = c - a, n = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x), each product rounded, then the
 *   difference: outward for counter-clockwise faces.  NRF_NORMALS_AREA contributes n; NRF_NORMALS_UNIT contributes n / l per component with
 *   l = sqrtf((nx*nx + ny*ny) + nz*nz), and zeros where l == 0.  Per vertex S = the contributions of its row added sequentially in ascending face index (the first
 *   one starts the sum); len = sqrtf((Sx*Sx + Sy*Sy) + Sz*Sz); out = S / len per component, zeros where len == 0 or the row is empty.
 *   The sum follows the order of the faces: the result is deterministic, NOT invariant under a permutation of the faces.
 *   An entry of the row outside [0, F) or a face with a corner outside [0, V) is skipped, never dereferenced.  Refused: V or F out of range, n_incident outside
 *   [0, 3F], a weighting that is neither constant; with V > 0 a null d_verts, d_face_start, d_out, d_faces (F > 0) or d_face_list (n_incident > 0), d_out == d_verts. */
#define NRF_ADJ_BOUNDARY 1
#define NRF_ADJ_NONMANIFOLD 2
#define NRF_ADJ_SHORT_ROW 32             /* face rows up to this length are sorted by one lane, longer ones by one workgroup */
#define NRF_SMOOTH_MAX_CHANNELS 4
#define NRF_SMOOTH_FREE 0
#define NRF_SMOOTH_FIXED 1
#define NRF_SMOOTH_CURVE 2
#define NRF_NORMALS_AREA 0
#define NRF_NORMALS_UNIT 1
NRF_API size_t nrf_mesh_adjacency_workspace_bytes(int64_t n_verts, int64_t n_faces);
NRF_API int nrf_mesh_adjacency_count(const int32_t *d_faces, int64_t n_verts, int64_t n_faces, int64_t *n_incident, int64_t *n_neighbours, void *d_workspace,
                                     size_t workspace_bytes, void *stream);
NRF_API int nrf_mesh_adjacency_emit(const int32_t *d_faces, int64_t n_verts, int64_t n_faces, int64_t n_incident, int64_t n_neighbours, int64_t *d_face_start,
                                    int32_t *d_face_list, int64_t *d_nbr_start, int32_t *d_nbr, int32_t *d_nbr_faces, uint8_t *d_flags, int64_t *d_stats,
                                    void *d_workspace, size_t workspace_bytes, void *stream);
NRF_API int nrf_mesh_smooth(const float *d_x, float *d_out, float *d_tmp, int64_t n_verts, int channels, int iterations, float lambda, float mu, int boundary,
                            const int64_t *d_nbr_start, const int32_t *d_nbr, const int32_t *d_nbr_faces, const uint8_t *d_flags, int64_t n_neighbours, void *stream);
NRF_API int nrf_mesh_vertex_normals(const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, const int64_t *d_face_start,
                                    const int32_t *d_face_list, int64_t n_incident, int weighting, float *d_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Density gradient (normals.hip; the reference's calculate_normals, never finished there)
 * ------------------------------------------------------------------------------------------- */
/* d_sigma [p] (may be NULL) = raw[..., 3] of nrf_run_network(NRF_PREC_F32) at d_pts [p,3], bit for bit (keep mask of NeRFRenderer.h:187-188 included: it writes
 * column -1, so a 4-column net gives 0 outside the hash box and a 7-column one keeps sigma); d_grad [p,3] = d sigma / d x, forward mode: the encoder's derivative in
 * the cell the forward pass chooses (CuHashEmbedder: of the unrounded fp32 blend, 0 on an axis the box clamp moved; HashEmbedder: torch autograd of
 * HashEmbedderImpl::forward), the tangents through the sigma net in fp32 beside the exact primal, masked by its ReLUs; 0 where sigma is replaced by 0.  Hash grid
 * (either mode) + NeRFSmall with 32 features, hidden_dim 64 and 2 or 3 sigma-net layers; anything else is NRF_ERR_UNSUPPORTED.  The call needs no workspace
 * (the workspace size is 0; both arguments are accepted for symmetry with nrf_density_grid) and launches in bounded slabs. */
NRF_API size_t nrf_density_grad_workspace_bytes(const nrf_renderer *r, int64_t p);
NRF_API int nrf_density_grad(const nrf_renderer *r, const float *d_pts, int64_t p, float *d_sigma, float *d_grad, void *d_workspace, size_t workspace_bytes,
                             void *stream);

/* ---------------------------------------------------------------------------------------------
 * Closest point on a mesh (geometry.hip; no counterpart in the reference)
 * ------------------------------------------------------------------------------------------- */
/* For every query point the nearest FACE of a triangle list, the point on that face, its barycentrics and the squared distance: the exact point-to-triangle query
 * under the sampled point-to-point one of nrf_nearest_points.  It shares that entry's grid (bbox, dims, inv_h, h, the cell coordinate, NRF_NN_MAX_DIM / _MAX_CELLS /
 * _MAX_RINGS), its key, its stop rule and its conventions: fp32 operations rounded once each, / correctly rounded, caller-owned buffers, refusals (NRF_ERR_INVALID_ARG,
 * or NRF_ERR_WORKSPACE for a short workspace, the message starting with the entry's name) before any launch or write, two runs the same bits.
 *
 * Order of calls.  nrf_face_grid_count (workspace of nrf_face_grid_workspace_bytes) returns *n_refs and *n_large to the host: the ONE synchronisation.  The caller
 * allocates nrf_face_grid_bytes(F, dims, n_refs, n_large) bytes; nrf_face_grid_build fills them from the same mesh, box, dims and workspace (untouched in between).
 * The workspace may then go; any number of nrf_closest_on_mesh calls read the grid buffer (both directions of a distance, slab after slab of a bake).  Build and
 * query synchronise nothing.
 *
 * CONTRACT.
 *   Faces.  d_verts [V,3] fp32, d_faces [F,3] int32, 0 <= V, F < 2^31.  A face with a corner outside [0, V) is BAD, a face with a non-finite vertex coordinate is
 *   NON-FINITE (the classes of nrf_mesh_sample_count, without its area test: a face of finite corners whose area overflows is a face here).  Both are skipped whole,
 *   nothing of a bad face is dereferenced.  Repeated corners and zero area do not make a face invalid.
 *   Cell box of a face.  Per axis cell(min of the three coordinates) .. cell(max of the three), cell() the clamped cell coordinate of nrf_nearest_points.
 *   Binned and large faces.  A face whose cell box holds at most NRF_FG_MAX_FACE_CELLS cells has one reference in every cell of the box (integer atomics count, the
 *   counts are scanned, a cursor scatters; the order inside a cell may vary, nothing depends on it); n_refs is their number, refused at 2^32 or more (the message says
 *   so).  A face with a larger box goes to the large list (n_large entries), which every query tests in full.  NRF_FG_MAX_FACE_CELLS is a tuning constant: no result
 *   depends on it, nor on the grid.
 *   Closest point of query q on the face (a, b, c), the Voronoi-region form of Ericson, Real-Time Collision Detection, 5.1.5.  Per component ab = b - a, ac = c - a,
 *   ap = q - a, bp = q - b, cp = q - c.  dot(x, y) = (xx*yx + xy*yy) + xz*yz.  d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp),
 *   d6 = dot(ac, cp); vc = d1*d4 - d3*d2, vb = d5*d2 - d1*d6, va = d3*d6 - d5*d4 (each product rounded, then the difference).  The first region that holds, in
 *   this order, gives (v, w) and P per component:
 *     A        d1 <= 0 and d2 <= 0                          (0, 0)    P = a
 *     B        d3 >= 0 and d4 <= d3                         (1, 0)    P = b
 *     edge AB  vc <= 0 and d1 >= 0 and d3 <= 0              v = d1 / (d1 - d3), w = 0                                          P = a + v*ab
 *     C        d6 >= 0 and d5 <= d6                         (0, 1)    P = c
 *     edge AC  vb <= 0 and d2 >= 0 and d6 <= 0              v = 0, w = d2 / (d2 - d6)                                          P = a + w*ac
 *     edge BC  va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0    w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), v = 1.0f - w              P = b + w*(c - b)
 *     interior otherwise                                    denom = 1.0f / ((va + vb) + vc), v = vb * denom, w = vc * denom    P = (a + ab*v) + ac*w
 *   Then P is clamped per component to the face's own coordinate box, lo = min(a, b, c), hi = max(a, b, c): P = P < lo ? lo : (P > hi ? hi : P), a form under which a
 *   NaN stays a NaN.  Then d2 = (dx*dx + dy*dy) + dz*dz with dx = qx - Px (nn_d2, the function nrf_nearest_points uses).  (v, w) is the pair nrf_mesh_sample_emit
 *   writes: P is about (1 - v - w) a + v b + w c; the clamp moves P by rounding errors only and leaves (v, w) as computed.
 *   Result.  For a finite query the minimum of the key ((uint64)float_bits(d2) << 32) | f over all valid faces f with d2 <= fl(max_dist * max_dist); max_dist >= 0,
 *   +inf for no limit.  A NaN d2 (a zero-area face can give 0 / 0) fails that comparison and never wins; on an exact tie, across a shared edge or vertex, the lowest
 *   face index wins.  d_dist2 [nq], d_face [nq] int32, and, each or NULL, d_uv [nq,2] = (v, w) and d_point [nq,3] = P of the winning face.  No such face: +inf, -1,
 *   zeros; a non-finite query gets the same.  A d2 that overflows to +inf with a valid face is a valid answer.  d_stats [4] uint32 or NULL (ADDED to; the caller
 *   zeroes it): nrf_closest_on_mesh adds [0] non-finite queries and [3] queries served by the fallback, nrf_face_grid_count adds [1] bad and [2] non-finite faces.
 *   F == 0 is valid everywhere; nq == 0 is valid and launches nothing.
 * SCAN AND STOP.  One lane per query: first the large list, then ring r = 0, 1, ... of cells exactly as nrf_nearest_points walks them, every reference of every cell of
 *   the ring (a face met twice is harmless: the minimum is idempotent), and after ring r the same stop: every cell scanned, or min(best_d2, fl(max_dist * max_dist)) <
 *   fl(B * B), strictly, B = fl(fl((float)r * h_min) * 0.999f).
 * WHY THE STOP STAYS EXACT.  The clamp puts every coordinate of P between the face's smallest and largest coordinate on that axis, and the cell coordinate is monotone
 *   in x (fl(x - bmin), the product with inv_h > 0, floorf and the clamp all are): P's cell lies inside the face's cell box.  A binned face without a reference in the
 *   cube of radius r around the query's cell has a cell box that misses the cube on some axis, so P is a "target in a cell at least r + 1 away on that axis" and WHY
 *   THE STOP IS EXACT of nrf_nearest_points applies to P word for word: d2 >= fl(B * B).  Large faces are never unscanned.  Without the clamp the computed P can leave
 *   the box by a rounding error and the argument fails: the clamp is part of the definition, not an optimisation.
 * FALLBACK.  A query with no stop after ring NRF_NN_MAX_RINGS is appended to a list in the workspace; a second kernel, a fixed grid of workgroups striding the list by
 *   the count read on the device, brute-forces ALL faces for it with a block-wide minimum of the key.  Rings, large list and fallback form the candidate through one
 *   inline function.  Every loop is bounded by a clamped range or a count; nothing waits on another workgroup.
 * REFUSED: V, F, nq or the dims out of range; a null bbox, d_faces (F > 0), d_verts (V > 0 and F > 0), n_refs / n_large (count), d_query, d_dist2 or d_face (nq > 0); a
 *   box nrf_nearest_points refuses; max_dist < 0 or NaN; n_refs outside [0, 2^32) or n_large outside [0, F]; a null or misaligned (8 bytes) workspace or grid buffer, a
 *   short workspace; a grid buffer whose size is not nrf_face_grid_bytes of these F, dims, n_refs and n_large.  The build also writes what it was built for (F, dims,
 *   counts, the bits of the box) at the head of the buffer; a query whose arguments pass the host's size check but disagree with that head reads nothing more of the
 *   buffer and writes nothing. */
#ifndef NRF_FG_MAX_FACE_CELLS            /* tuning builds set another (make EXTRA=-DNRF_FG_MAX_FACE_CELLS=n); no result depends on it */
#define NRF_FG_MAX_FACE_CELLS 64         /* the largest cell box of a binned face; a face with more cells goes to the large list */
#endif
NRF_API size_t nrf_face_grid_workspace_bytes(int64_t n_faces, int nx, int ny, int nz);
NRF_API size_t nrf_face_grid_bytes(int64_t n_faces, int nx, int ny, int nz, int64_t n_refs, int64_t n_large);
NRF_API int nrf_face_grid_count(const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, const float *bbox, int nx, int ny, int nz,
                                int64_t *n_refs, int64_t *n_large, uint32_t *d_stats, void *d_workspace, size_t workspace_bytes, void *stream);
NRF_API int nrf_face_grid_build(const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, const float *bbox, int nx, int ny, int nz,
                                int64_t n_refs, int64_t n_large, void *d_grid, size_t grid_bytes, void *d_workspace, size_t workspace_bytes, void *stream);
NRF_API size_t nrf_closest_on_mesh_workspace_bytes(int64_t nq);
NRF_API int nrf_closest_on_mesh(const float *d_query, int64_t nq, const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, const float *bbox,
                                int nx, int ny, int nz, int64_t n_refs, int64_t n_large, const void *d_grid, size_t grid_bytes, float max_dist, float *d_dist2,
                                int32_t *d_face, float *d_uv, float *d_point, uint32_t *d_stats, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Ray casting on a mesh (raycast.hip; no counterpart in the reference)
 * ------------------------------------------------------------------------------------------- */
/* For every ray the first face of a triangle list it hits (closest mode) or whether it hits any (any mode), over the face grid of nrf_face_grid_count / _build, whose
 * buffer is read unchanged; cosine-weighted directions around normals; and the two fused into ambient occlusion.  Conventions as above: fp32 operations rounded once
 * each (-ffp-contract=off), / and sqrtf correctly rounded, caller-owned buffers, refusals before any launch or write, two runs the same bits.  No output depends on
 * the grid, the order of the faces (beyond the tie-break the key states) or the scheduling: tests/raycast_ref.py restates every output by brute force over all
 * (ray, face) pairs and knows nothing of grids.
 *
 * CONTRACT.
 *   Rays.  d_rays [n, stride] fp32, 8 <= stride <= NRF_RC_MAX_STRIDE: the library's packed ray row o[3], d[3], near, far, ... (nrf_pack_rays, nrf_atlas_texels).  d is
 *   not normalised; t is in units of d, the renderer's z (the point is o + d*t).  The range is [lo, hi] = [max(near, 0), far] (near > 0 ? near : 0); far = +inf is
 *   allowed; lo <= hi false: an empty range, a miss.  A ray with a non-finite o or d, d == 0 on all three axes, or a NaN near or far is INVALID: the miss values, and
 *   counted in d_stats[0].
 *   Faces.  Valid, bad and non-finite faces exactly as for nrf_face_grid_count: bad and non-finite faces are skipped whole, zero area does not make a face invalid.
 *   Candidate of face (a, b, c) for a ray, Moeller-Trumbore.  dot(x, y) = (x0*y0 + x1*y1) + x2*y2; x cross y = (x1*y2 - x2*y1, x2*y0 - x0*y2, x0*y1 - x1*y0), every
 *   product rounded, then the difference.  ab = b - a, ac = c - a, p = d cross ac, det = dot(ab, p), inv = 1.0f / det, tv = o - a, v = dot(tv, p) * inv,
 *   q = tv cross ab, w = dot(d, q) * inv, t = dot(ac, q) * inv, then t = t + 0.0f (-0.0f becomes +0.0f: as bits, -0.0f lies above every positive t, and a ray that
 *   starts in a face's plane would lose to everything behind it).
 *   ACCEPTED iff all hold (a NaN fails every comparison and never wins):
 *     det != 0, and cull agrees: NRF_RC_CULL_NONE any sign; NRF_RC_CULL_BACK det > 0 (the faces nrf_raster_mesh draws with cull == 1: counter-clockwise seen from
 *     the ray's origin); NRF_RC_CULL_FRONT det < 0;
 *     v >= 0, w >= 0, v + w <= 1.0f;
 *     lo <= t <= hi and t < +inf (with t = +inf the point o + t*d is not a number on an axis where d is 0);
 *     the surface point P = (a + ab*v) + ac*w per component, clamped to the face's coordinate box in the NaN-keeping form of nrf_closest_on_mesh (one inline function
 *     serves both), and the ray point Pu = o + t*d per component (product and sum rounded) agree: |Pu - P|_inf <= tau, tau = 2^NRF_RC_TAU_LOG2 * max(|o|_inf, |Pu|_inf).
 *   The last rule is what makes a walk over a grid provably complete; it is grid-free and removes only hits whose t is numerically meaningless.  Measured in fp32
 *   numpy (tests/test_raycast_host.py repeats it): the worst |Pu - P|_inf / max(|o|_inf, |Pu|_inf) over the candidates that pass the other rules is 2^-14.9 on the
 *   tests' ordinary ray sets (three sphere levels, also shifted by 100 units; rays at vertices and edges among them) and 2^-17.4 on 1 000 rays grazing the sphere
 *   within 0.5 % of its radius, nothing rejected; the only candidates the rule removes there belong to rays that lie IN a face's plane (det a rounding error,
 *   ratio 2^-0.7 .. 2^-2.5).  2^-12 leaves a factor of seven above the worst ordinary ratio.
 *   Result, NRF_RC_CLOSEST.  The minimum of ((uint64)float_bits(t) << 32) | f over the accepted candidates of all valid faces: t >= +0 orders as its bits, and on an
 *   exact tie in t, across a shared edge or vertex, the lowest face index wins.  d_t [n], d_face [n] int32, and, each or NULL, d_uv [n,2] = (v, w), d_point [n,3] =
 *   P of the winning face and d_hit [n] uint8 = 1 on a hit.  A miss: +inf, -1, zeros, 0.
 *   Result, NRF_RC_ANY.  d_hit [n] = 1 iff some accepted candidate exists; d_t, d_face, d_uv and d_point must be NULL (which candidate a walk meets first is not
 *   defined).  d_hit of any mode equals isfinite(d_t) of closest mode.
 *   d_stats [4] uint32 or NULL, ADDED to, laid out as for nrf_closest_on_mesh: [0] invalid rays, [3] rays served by the fallback ([1], [2] are nrf_face_grid_count's).
 * WALK.  One lane per ray.  cell() is the clamped cell coordinate of nrf_nearest_points, h_min the grid's smallest cell edge, |box|_inf the largest absolute
 *   coordinate of bbox.
 *   1. A pass over the faces sets a flag in the workspace if a valid face has a coordinate outside [bbox min, bbox max] (never a host hint).  With the flag set every
 *      valid ray with a non-empty range goes to the fallback.
 *   2. Far origin: 4 * fl(2^-12 * |o|_inf) > h_min sends the ray to the fallback.
 *   3. Clip.  The box is widened on every side by margin = h_min + 2^-10 * |box|_inf.  Per axis with d != 0: ta = (lo_a - o_a) / d_a, tb = (hi_a - o_a) / d_a,
 *      swapped so that ta <= tb, ta = ta * (1 - 2^-10) where ta > 0, tb = tb * (1 + 2^-10); t0 = max(lo, all ta), t1 = min(hi, all tb).  An axis with d == 0 whose o
 *      lies outside the widened box, or t0 <= t1 false: a miss.
 *   4. The large list is tested in full (any mode stops at the first accepted candidate, here and below).
 *   5. Steps.  dt = h_min / |d|_inf; t_0 = t0, t_k = fl(t0 + fl((float)k * dt)), replaced by t1 where it passes t1 (and t1 > t_k-1).  t_k <= t_k-1: the fallback.
 *      Pa = o + t_k-1 * d, Pb = o + t_k * d per component; tau_k = 2^-12 * max(|o|_inf, |Pa|_inf, |Pb|_inf); 4 * tau_k <= h_min false: the fallback.  The step
 *      looks up every cell of [cell(min(Pa, Pb) - 2 tau_k), cell(max(Pa, Pb) + 2 tau_k)] per axis, except those of the previous lookup's range (their references have
 *      all been tested: a candidate does not depend on the step).
 *   6. Stop after step k iff best_t <= t_k (any mode: a candidate was accepted), or t_k >= t1.  Still open after NRF_RC_MAX_STEPS steps: the fallback.
 * WHY THE WALK CANNOT MISS.
 *   Monotone.  Per component fl(o + fl(t*d)) is monotone in t (a rounded product with a constant and a rounded sum with a constant are), and cell() is monotone in
 *   its argument.  So for t in [t_k-1, t_k], Pu(t) lies per axis between Pa and Pb, and tau(t) <= tau_k.
 *   A step is complete.  An accepted candidate with t in the step has P within tau_k of that span per axis, so cell(P) lies in [cell(min - 2 tau_k),
 *   cell(max + 2 tau_k)]: the factor 2 absorbs the roundings of the subtraction, of min - 2 tau_k and of the comparison, all far below tau_k.  The clamp puts cell(P)
 *   inside the face's cell box.  So the face has a reference in a looked-up cell or is on the large list.  Steps are closed intervals that share their end points
 *   and cover [t0, t1].
 *   The stop is exact.  After step k every accepted candidate with t <= t_k has been seen (steps 1 .. k cover [t0, t_k], and none lies before t0, below).  An unseen
 *   candidate has t > t_k >= best_t strictly: it can neither win nor tie.
 *   The clip loses nothing.  All valid faces lie in the box (step 1), so P does, and Pu is within tau of the box.  After step 2, 2^-12 |o|_inf <= h_min / 4; and
 *   tau = 2^-12 |Pu|_inf with |Pu|_inf <= |box|_inf + tau gives tau < 2^-11 |box|_inf.  Either way tau <= max(h_min / 4, 2^-11 |box|_inf), less than the margin by
 *   more than 3/4 h_min + 2^-11 |box|_inf.  Pu_a(t) is monotone, so the t with Pu_a(t) within tau of the box form an interval; the computed ta and tb differ from
 *   the exact parameters of the WIDENED box by two roundings (2^-22 relative, a displacement below 2^-22 (|box|_inf + margin + |o|_inf) <= 2^-12 h_min + 2^-21
 *   |box|_inf along the axis), the factors 1 -+ 2^-10 only widen the interval, and an axis with d == 0 has Pu_a = o_a for every finite t.
 *   The large list is never unscanned.
 * FALLBACK.  Exact and slow, counted in d_stats[3]: rays are appended to a list in the workspace; a second kernel, a fixed grid of workgroups striding the list by the
 *   count read on the device, tests ALL faces for each with a block-wide minimum of the key.  The conditions, each with a test: a valid face outside the box; a far
 *   origin (step 2, or 4 * tau_k > h_min at a step); a step that does not advance; a ray still open after NRF_RC_MAX_STEPS steps.  Walk, large list and fallback
 *   form the candidate through one inline function.  Every loop is bounded by a clamped range or a count; nothing waits on another workgroup.
 * HEMISPHERE DIRECTIONS.  nrf_hemisphere_dirs: d_dirs [n, k, 3], direction j around normal i a pure function of (seed, index0 + i, j); no trigonometry.
 *   n-hat: len2 = dot(n, n); a non-finite n, or len2 == 0 or not finite, is a BAD normal: k zero directions, counted once in d_stats[0].  Else n-hat = n / sqrtf(len2)
 *   per component.  Marsaglia's disc: for attempt a = 0 .. NRF_HEMI_ATTEMPTS - 1, with u(c) = nrf_rng_uniform(seed, NRF_RNG_HEMI_DIR, ((index0 + i) << 20) | (j << 4)
 *   | c): x1 = 2 u(2a) - 1, x2 = 2 u(2a + 1) - 1 (both exact), s = x1*x1 + x2*x2; the first attempt with s < 1 gives r = sqrtf(1 - s), q = ((2 x1) r, (2 x2) r,
 *   1 - 2 s), a uniform point of the unit sphere; no such attempt (probability 0.215^8): q = (0, 0, 1).  v = n-hat + q, l2 = dot(v, v); l2 < NRF_HEMI_MIN_LEN2: the
 *   direction is n-hat, else v / sqrtf(l2) per component.  A uniform point of the sphere tangent to the surface, seen from the point of contact: the cosine law.
 * AMBIENT OCCLUSION.  nrf_mesh_ambient_occlusion: ray (i, j) has o = p_i + offset * n-hat_i per component, d = direction j of point index0 + i, the range
 *   [0, max_dist], no culling, any mode; d_ao [n] = (float)(k - hits) / (float)k, exact as the count is an integer.  A bad normal or a non-finite p makes the k rays
 *   of the point invalid: they miss, d_ao is 1, d_stats[0] grows by k.  No ray or direction is written.  The call equals nrf_hemisphere_dirs followed by
 *   nrf_ray_cast_mesh(NRF_RC_ANY) bit for bit, and its d_stats[0] and [3] are those of that nrf_ray_cast_mesh call (nrf_hemisphere_dirs given NULL stats: with stats it
 *   would add one more per bad normal to [0]): both share one device function for the walk and one for the directions.  One lane
 *   per ray of the flattened [n, k] rays, a point's hits counted by ballot and popcount into an integer counter of the workspace (integer atomics: no order to
 *   depend on); a ray the walk gives up is tested against all faces by its wave at once.  Workspace: nrf_ray_cast_workspace_bytes(n).  n * k <= NRF_AO_MAX_RAYS
 *   per call; index0 lets a caller go slab by slab with the same draws.
 * REFUSED (NRF_ERR_INVALID_ARG, or NRF_ERR_WORKSPACE for a short workspace): n, V, F or the dims out of range; stride outside [8, NRF_RC_MAX_STRIDE]; a cull or mode
 *   that is none of the constants; a null bbox, d_faces (F > 0), d_verts (V > 0 and F > 0), d_rays (n > 0); closest mode with a null d_t or d_face, any mode with a null
 *   d_hit or a non-null d_t, d_face, d_uv or d_point; a box nrf_nearest_points refuses, or whose widening is not finite; n_refs, n_large, grid buffer and workspace as
 *   for nrf_closest_on_mesh; k outside [1, NRF_HEMI_MAX_K]; index0 < 0 or index0 + n > NRF_HEMI_MAX_INDEX; n * k > 2^31 - 1 (nrf_hemisphere_dirs) or > NRF_AO_MAX_RAYS; a null d_normals,
 *   d_dirs, d_points or d_ao (n > 0); an offset that is not finite; max_dist < 0 or NaN.  A grid buffer that passes the size check but whose head disagrees with the
 *   arguments: nothing more of it is read and nothing is written.  n == 0 is valid and launches nothing; F == 0 is valid: every ray misses. */
#define NRF_RC_CLOSEST 0
#define NRF_RC_ANY 1
#define NRF_RC_CULL_NONE 0
#define NRF_RC_CULL_BACK 1
#define NRF_RC_CULL_FRONT 2
#define NRF_RC_TAU_LOG2 (-12)            /* the consistency bound of t and P, relative to max(|o|_inf, |Pu|_inf) */
#define NRF_RC_MAX_STEPS 1024            /* steps of the walk before a ray goes to the fallback: about the cells of the longest axis a grid can have.  The far-origin
                                            rules keep every point of a walk within 1024 h_min of the origin of the coordinates, so no walk has more than ~2050 steps
                                            whatever the cap; 1024 is reached by a ray through all cells of a 1024-cell axis and by little else */
#define NRF_RC_MAX_STRIDE 64             /* floats per packed ray row */
#define NRF_RNG_HEMI_DIR 12              /* the stream of nrf_rng.h the disc draws of a direction come from: the next after its own ids (NRF_RNG_SURFACE_UV = 11) */
#define NRF_HEMI_ATTEMPTS 8              /* disc rejections per direction */
#define NRF_HEMI_MAX_K 65536             /* directions per normal: j takes 16 bits of the draw's index */
#define NRF_HEMI_MAX_INDEX ((int64_t)1 << 40)
#define NRF_AO_MAX_RAYS ((int64_t)1 << 38)          /* n * k of one nrf_mesh_ambient_occlusion call: a lane per ray, 2^30 workgroups */
#define NRF_HEMI_MIN_LEN2 9.5367431640625e-07f          /* 2^-20: below it n-hat + q has no direction and n-hat itself is used */
NRF_API size_t nrf_ray_cast_workspace_bytes(int64_t n_rays);
NRF_API int nrf_ray_cast_mesh(const float *d_rays, int64_t n_rays, int stride, const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces,
                              const float *bbox, int nx, int ny, int nz, int64_t n_refs, int64_t n_large, const void *d_grid, size_t grid_bytes, int cull, int mode,
                              float *d_t, int32_t *d_face, float *d_uv, float *d_point, uint8_t *d_hit, uint32_t *d_stats, void *d_workspace, size_t workspace_bytes,
                              void *stream);
NRF_API int nrf_hemisphere_dirs(const float *d_normals, int64_t n, int k, uint64_t seed, int64_t index0, float *d_dirs, uint32_t *d_stats, void *stream);
NRF_API int nrf_mesh_ambient_occlusion(const float *d_points, const float *d_normals, int64_t n, int k, float offset, float max_dist, uint64_t seed, int64_t index0,
                                       const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, const float *bbox, int nx, int ny, int nz,
                                       int64_t n_refs, int64_t n_large, const void *d_grid, size_t grid_bytes, float *d_ao, uint32_t *d_stats, void *d_workspace,
                                       size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Mesh voxelisation (voxel.hip; no counterpart in the reference)
 * ------------------------------------------------------------------------------------------- */
/* Scan conversion of a triangle list onto the lattice of nrf_density_grid / nrf_tsdf_integrate (P = bmin + (float)i * step, step = (bmax - bmin) / (float)(n - 1)
 * per axis, x fastest, nx, ny, nz >= 2, fewer than 2^31 points; bbox[6] on the HOST): what is INSIDE a mesh.  d_verts [V,3] fp32, d_faces [F,3] int32
 * (counter-clockwise seen from outside), 0 <= V < 2^31, 0 <= F <= 2^31 - 2 -> each or NULL (not all three): d_winding [nz][ny][nx] int32, the winding number;
 * d_sdf [nz][ny][nx] fp32, the signed distance truncated at +-trunc, outside positive (the TSDF's convention: -sdf is a lattice for nrf_isosurface_*); d_face
 * [nz][ny][nx] int32, the nearest face within trunc or -1.  d_stats [4] uint32 or NULL (ADDED to; the caller zeroes it): [0] CLIPPED, [1] BAD, [2] NON-FINITE faces;
 * [3] is not touched.  The work is a scatter, proportional to the faces and to what they cover, not a gather over the lattice; integer atomics only (an add, a
 * 64-bit min), so the result depends neither on scheduling nor on the order of the face list (beyond the tie-break by index the key states): two runs give the same
 * bits, and so does any permutation of the faces (d_face then names the same face by its new index).  The call synchronises nothing and allocates nothing.
 * Each source-level fp32 operation below is rounded once, / and sqrtf correctly; the edge functions are int64 and exact.
 *   Faces.  The classes of nrf_face_grid_count (one inline function): a face with a corner outside [0, V) is BAD, a face with a non-finite coordinate is NON-FINITE;
 *   both are skipped whole, nothing of a bad face is dereferenced.  Repeated corners and zero area do not make a face invalid.
 * WINDING (an orthographic raster along +z; the twin of nrf_raster_mesh's steps 3-5).
 *   1. Per vertex: gx = (Px - bminx) / stepx, gy and gz likewise (lattice units); X = (int)rintf(gx * 256.0f), Y = (int)rintf(gy * 256.0f) (NRF_RASTER_SUBPIXEL;
 *      round half to even).  A valid face with a vertex where fabsf(gx) or fabsf(gy) exceeds NRF_RASTER_GUARD, compared as floats (+-inf clips), is CLIPPED: left
 *      out of the winding pass only (the distance pass takes it).  A NON-ZERO d_stats[0] VOIDS THE WINDING and the sign of d_sdf: a crossing is missing.
 *   2. In int64, E_ab(p) = (bx-ax)*(py-ay) - (by-ay)*(px-ax); e0 = E_12(p), e1 = E_20(p), e2 = E_01(p) at the column p = (256 i, 256 j); A = E_01(v2).  A == 0
 *      contributes nothing: a face parallel to z has no projected area.  s = sign(A); s = +1 is a face whose normal has a +z component (counter-clockwise seen from
 *      outside, x to the right and y up).
 *   3. Column (i, j) is covered iff step 5 of nrf_raster_mesh calls it inside: for each edge k, s*e_k > 0, or s*e_k == 0 and the edge is top-left (edge k runs
 *      v1->v2, v2->v0, v0->v1; with (dx, dy) = s*(b - a) top-left iff dy < 0 || (dy == 0 && dx > 0)).  Columns visited: ceil(minX/256) .. floor(maxX/256) clamped to
 *      [0, nx-1], rows likewise with Y and ny.
 *      WHY THE WINDING OF A CLOSED MESH IS EXACT.  Two faces that share an edge take its endpoints from the same two vertex records, so both see the same snapped
 *      segment, in opposite directions.  A column strictly off the segment is on one definite side.  A column exactly ON it has e == 0 for both, and the top-left
 *      rule, which looks only at s*(b - a), decides: where the faces continue each other across the edge (equal s) the directions s*(b - a) are opposite and exactly
 *      one of them is top-left -- the column belongs to exactly one face; where they fold back at a silhouette (opposite s) the directions are equal and the column
 *      belongs to both or to neither, which adds +1 - 1 or nothing.  So along every column of the snapped mesh each sheet is crossed exactly once, no column is
 *      counted twice on an edge or lost in a crack, and the sum below is the winding number of the snapped surface -- an integer with no tolerance in it.
 *   4. Crossing height, in lattice units: b_k = (float)((double)(s*e_k) / (double)(s*A)); zc = (b0*gz0 + b1*gz1) + b2*gz2.
 *   5. t = ceilf(zc) - 1.0f; skipped unless t >= 0 (a crossing at or below level 0, and a NaN); kc = (int)fminf(t, (float)(nz - 1)), the largest k with (float)k < zc;
 *      one integer atomic add of s on delta[kc][j][i].
 *   6. winding(i, j, k) = the sum of delta[k'][j][i] over k' >= k: the +z-facing crossings above the point minus the -z-facing ones.  1 inside an outward-oriented
 *      closed solid and 0 outside; -1 inside an inverted solid, 2 inside two nested like-oriented shells, 0 in a cavity whose shell faces inward.  A point with
 *      zc == k exactly counts as not below the face.
 * DISTANCE (a scatter over each face's dilated lattice box; skipped, with its part of the workspace, when d_sdf and d_face are both NULL).
 *   7. Per valid face and axis, lo / hi the smallest / largest of the three coordinates: fl = floorf((lo - trunc - bmin) / step) - 1.0f, fh = ceilf((hi + trunc -
 *      bmin) / step) + 1.0f (the subtractions left to right).  The box is EMPTY unless fh >= 0 and fl <= (float)(n - 1) on every axis; else its indices are
 *      (int)fmaxf(fl, 0) .. (int)fminf(fh, (float)(n - 1)).
 *   8. Per lattice point P of the box: d2 between P and the face by the closest-point function of nrf_closest_on_mesh (one inline function: Ericson's regions, the
 *      clamp to the face's coordinate box, nn_d2).  Where d2 <= T2 = fl(trunc * trunc) (a NaN d2 fails), a 64-bit atomic min of ((uint64)float_bits(d2) << 32) | f
 *      on the point's key, initially d2 = +inf, f = -1.  The final key is the nearest face, the lowest index on a tie: nrf_closest_on_mesh(max_dist = trunc) there.
 *   WHY THE BOX IS COMPLETE.  Let Q be the closest point the function returns for lattice point P and face f, and suppose d2 <= T2.  The clamp keeps every
 *      coordinate of Q inside [lo, hi] of the face on that axis.  d2 = fl(fl(dx*dx + dy*dy) + dz*dz) with dx = fl(Px - Qx) is at least dx*dx less three roundings, and
 *      T2 is trunc*trunc within one, so |Px - Qx| <= trunc (1 + 3u), u = 2^-24: Px >= lo - trunc (1 + 3u), and likewise Px <= hi + trunc (1 + 3u).  Px itself is
 *      bmin + i*step within two roundings, and fl((lo - trunc - bmin) / step) is the real quotient within three.  All these errors are a few ulp of the largest
 *      magnitude among bmin, bmax, lo, hi and trunc; on a lattice whose points fp32 can tell apart (that magnitude below 2^20 steps -- any lattice this call accepts
 *      around a mesh of its own scale) they sum to less than one step, so i >= floor(quotient) - 1 = fl, and i <= fh the same way: the extra lattice step on each side
 *      pays for the rounding of the bounds.  Points visited needlessly are filtered by the comparison with T2, so the box is an optimisation of "every face against
 *      every lattice point", never part of the result.
 * FINISH (fused into the pass of step 6: the volume is read once).
 *   9. dist = key found ? sqrtf(d2) : trunc; dist = fminf(dist, trunc).  d_face = the key's face or -1.
 *  10. inside = winding != 0 (NRF_VOX_NONZERO: nested like-oriented shells merge into one solid), winding > 0 (NRF_VOX_POSITIVE: a reversed inner shell is
 *      subtracted, an inverted solid is empty) or winding & 1 (NRF_VOX_ODD: parity).  d_sdf = inside ? -dist : dist.
 * A face whose columns (step 3) or lattice box (step 7) hold more than NRF_VOXEL_WIDE_COLUMNS / NRF_VOXEL_WIDE_POINTS entries is scanned by a whole workgroup (same
 * device functions, same bits).  Every loop is bounded by a clamped range or a count; nothing waits on another workgroup.
 * d_workspace: 256-byte aligned, nrf_mesh_voxelize_workspace_bytes (0 for a shape the call refuses; 12 B per lattice point + 16 B per vertex + 8 B per face).  A call
 * without distance outputs needs only the part before the key lattice (8 B per point less).
 * NRF_ERR_INVALID_ARG, message starting "nrf_mesh_voxelize", nothing launched or written: a null bbox; a null d_faces, or a null d_verts with V > 0, with F > 0;
 * all three outputs NULL; n < 2 on an axis or 2^31 lattice points or more; an empty, inverted or non-finite box (or a step that is not finite and > 0); trunc not
 * finite or <= 0 while d_sdf or d_face is asked for (otherwise trunc is not read); a rule outside the three; V or F out of range; a null, misaligned or short
 * workspace.  F == 0 is valid: winding 0, sdf +trunc, face -1. */
#define NRF_VOX_NONZERO 0
#define NRF_VOX_POSITIVE 1
#define NRF_VOX_ODD 2
#ifndef NRF_VOXEL_WIDE_COLUMNS           /* tuning builds set another (make EXTRA=-DNRF_VOXEL_WIDE_COLUMNS=n); no result depends on either */
#define NRF_VOXEL_WIDE_COLUMNS 256       /* columns of a face's clamped bounding box above which the wide kernel rasterises it */
#endif
#ifndef NRF_VOXEL_WIDE_POINTS
#define NRF_VOXEL_WIDE_POINTS 256        /* lattice points of a face's dilated box above which the wide kernel scans it */
#endif
NRF_API size_t nrf_mesh_voxelize_workspace_bytes(int64_t n_verts, int64_t n_faces, int nx, int ny, int nz);
NRF_API int nrf_mesh_voxelize(const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, const float *bbox, int nx, int ny, int nz, float trunc,
                              int rule, int32_t *d_winding, float *d_sdf, int32_t *d_face, uint32_t *d_stats, void *d_workspace, size_t workspace_bytes,
                              void *stream);

/* ---------------------------------------------------------------------------------------------
 * Registration (align.hip; no counterpart in the reference)
 * ------------------------------------------------------------------------------------------- */
/* Bringing one surface into the frame of another: a pose on the device, points moved through it, the sums of one ICP iteration over given pairs, and the small
 * solve that updates the pose without a host round trip.  An iteration is nrf_align_apply -> nrf_closest_on_mesh (or nrf_nearest_points and a gather) ->
 * nrf_align_sums -> nrf_align_solve on one stream; nothing in it synchronises or allocates.  Conventions as above: caller-owned buffers, refusals before any launch
 * or write, two runs the same bits.  Everything below is fp64 arithmetic on fp32 data: each source-level operation rounded once (-ffp-contract=off), / and sqrt
 * correctly rounded, nothing but + - * / sqrt and comparisons.  tests/align_ref.py restates every step in numpy float64 and the GPU tests compare bit for bit.
 *
 * CONTRACT.
 *   State.  d_state: 8 doubles, 8-byte aligned: a unit quaternion (w, x, y, z), a scale s > 0, a translation t[3]; the pose is x -> s R x + t.
 *   nrf_align_state_init: pose == NULL (a HOST pointer) writes (1, 0, 0, 0, 1, 0, 0, 0); else pose[8] with the quaternion divided by
 *   sqrt(((w*w + x*x) + y*y) + z*z) per component, s and t as given.
 *   R(w, x, y, z), row-major, wherever a rotation is formed from a quaternion:
 *     R00 = 1 - 2*(y*y + z*z)   R01 = 2*(x*y - w*z)       R02 = 2*(x*z + w*y)
 *     R10 = 2*(x*y + w*z)       R11 = 1 - 2*(x*x + z*z)   R12 = 2*(y*z - w*x)
 *     R20 = 2*(x*z - w*y)       R21 = 2*(y*z + w*x)       R22 = 1 - 2*(x*x + y*y)
 *   dot(a, b) = (a0*b0 + a1*b1) + a2*b2.
 *   nrf_align_apply.  One lane per point.  M = s*R per entry; y_a = (float)(((M_a0*x0 + M_a1*x1) + M_a2*x2) + t_a).  rotate_only == 1 (normals):
 *   y_a = (float)((R_a0*x0 + R_a1*x1) + R_a2*x2), no s, no t, not renormalised.  d_out may be d_points (the three inputs are read before the first write).
 *   nrf_align_sums.  Pair i is (y_i, p_i) = (d_y[i], d_p[i]), a moved point and its target, with d_face[i] the face of the target mesh p_i lies on: exactly what
 *   nrf_closest_on_mesh writes, so its max_dist is the trim.  A pair is DROPPED, tested in this order and counted in d_stats [4] uint32 (ADDED to; or NULL):
 *     [0] d_face[i] < 0 (no pair);  [1] a non-finite coordinate of y_i or p_i;  and, NRF_ALIGN_PLANE only,
 *     [2] face d_face[i] is bad or non-finite (the classes of nrf_face_grid_count, one inline function; an index >= F is bad);  [3] its normal has zero length.
 *   The fp32 values are converted to fp64 first; d = p - y per component.
 *   NRF_ALIGN_POINT, NRF_ALIGN_POINT_COLUMNS = 19 columns: [0] 1; [1..3] y_a; [4..6] p_a; [7 + 3a + b] y_a*p_b; [16] dot(y, y); [17] dot(p, p); [18] dot(d, d).
 *   The mesh arguments are not read.
 *   NRF_ALIGN_PLANE, NRF_ALIGN_PLANE_COLUMNS = 37 columns.  With (A, B, C) the face's corners: e1 = B - A, e2 = C - A (fp64 differences of the converted
 *   corners), c = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x), len2 = (cx*cx + cy*cy) + cz*cz (len2 > 0 false: dropped), len = sqrt(len2),
 *   n = c / len per component (three divisions).  r = dot(n, d).  The row a[7] = (y1*n2 - y2*n1, y2*n0 - y0*n2, y0*n1 - y1*n0, n0, n1, n2, dot(n, y)): the
 *   coefficients of (alpha, beta, gamma, tx, ty, tz, sigma) in the linearised residual r - a.x of the update y -> (1 + sigma)(y + omega x y) + t.
 *   Columns: [0..27] a_i*a_j for i <= j, i-major; [28 + i] a_i*r; [35] 1; [36] r*r.
 *   ORDER OF A SUM.  Block k takes pairs [k*NRF_ALIGN_TILE, (k+1)*NRF_ALIGN_TILE); lane t of 256 adds its entries t, t + 256, ... in ascending order, dropped pairs
 *   skipped, into one accumulator per column from 0.0; then steps 1 and 2 of the ordered sum (nrf_mesh_sample_count, step 4) give the block's partial.  The
 *   workspace holds [max(1, ceil(n / NRF_ALIGN_TILE))][columns] partials; n == 0 gives one row of zeros.  So a total is unchanged by any permutation of the pairs
 *   that keeps every pair in its lane's set of its block in the same relative order -- and by nothing more: swapping two pairs between lanes or tiles may change
 *   the last bits.
 *   nrf_align_solve (n and mode as given to nrf_align_sums, the same workspace).  One workgroup: steps 3 and 4 of the ordered sum per column give the totals T;
 *   one thread computes the update (dq, ds, dt) and a flag, composes it into d_state and writes a row of the history.
 *   NRF_ALIGN_POINT (Horn's closed form).  cnt = T[0]; cnt >= 3 false: NRF_ALIGN_FLAG_FEW_PAIRS.  Sy = T[1..3], Sp = T[4..6]; ybar = Sy / cnt, pbar = Sp / cnt;
 *     S_ab = T[7 + 3a + b] - (Sy_a*Sp_b) / cnt;  vy = T[16] - dot(Sy, Sy) / cnt;  vy > 0 false: NRF_ALIGN_FLAG_NO_SPREAD.  The symmetric 4x4
 *     N00 = (Sxx + Syy) + Szz, N11 = (Sxx - Syy) - Szz, N22 = (Syy - Sxx) - Szz, N33 = (Szz - Sxx) - Syy, N01 = Syz - Szy, N02 = Szx - Sxz, N03 = Sxy - Syx,
 *     N12 = Sxy + Syx, N13 = Szx + Sxz, N23 = Syz + Szy.  Cyclic Jacobi on A = N with V = I: NRF_ALIGN_JACOBI_SWEEPS sweeps over the pairs (p, q) = (0,1), (0,2),
 *     (0,3), (1,2), (1,3), (2,3).  A[p][q] == 0: the pair is skipped.  th = (A[q][q] - A[p][p]) / (2*A[p][q]); |th| > NRF_ALIGN_JACOBI_BIG_THETA (th*th would
 *     overflow): t = 0.5 / th, else t = (th >= 0 ? 1 : -1) / (|th| + sqrt(th*th + 1)); c = 1 / sqrt(t*t + 1), s = t*c.  Then for k = 0..3 the columns
 *     (A[k][p], A[k][q]) <- (c*A[k][p] - s*A[k][q], s*A[k][p] + c*A[k][q]), then for k = 0..3 the rows (A[p][k], A[q][k]) <- (c*A[p][k] - s*A[q][k],
 *     s*A[p][k] + c*A[q][k]), then V's columns as A's.  The eigenvector: column k of V with the largest A[k][k] (the lowest k on a tie), negated where its w < 0,
 *     divided by its norm sqrt(((w*w + x*x) + y*y) + z*z) (not > 0 or not finite: NRF_ALIGN_FLAG_BAD_ROTATION): dq, always a proper rotation.  dR = R(dq).
 *     ds = 1, or with scale: the sum over (a, b) = (0,0), (0,1), .. (2,2), in that order from the first term, of dR_ab*S_ba, divided by vy; ds > 0 false or not
 *     finite: NRF_ALIGN_FLAG_BAD_SCALE.  dt_a = pbar_a - ds*((dR_a0*ybar0 + dR_a1*ybar1) + dR_a2*ybar2).
 *   NRF_ALIGN_PLANE (Gauss-Newton on the point-to-plane residual).  m = 7 with scale, else 6 (the leading block); T[35] >= m false: NRF_ALIGN_FLAG_FEW_PAIRS.
 *     H = the symmetric matrix of columns 0..27, g = columns 28..34.  Cholesky, for j = 0..m-1: d = H[j][j], then d = d - L[j][k]*L[j][k] for k = 0..j-1; d > 0 false
 *     or not finite: NRF_ALIGN_FLAG_BAD_PIVOT; L[j][j] = sqrt(d); for i > j: v = H[i][j], v = v - L[i][k]*L[j][k] for k = 0..j-1, L[i][j] = v / L[j][j].  Forward:
 *     z_i = (g_i - L[i][0]*z_0 - ... - L[i][i-1]*z_i-1) / L[i][i], the subtractions left to right; backward, i = m-1..0: x_i = (z_i - L[i+1][i]*x_i+1 - ... -
 *     L[m-1][i]*x_m-1) / L[i][i].  A non-finite x_i: NRF_ALIGN_FLAG_BAD_PIVOT.  dq = (1, x0/2, x1/2, x2/2) divided by sqrt(((1 + a*a) + b*b) + c*c) of its vector
 *     part (not finite: NRF_ALIGN_FLAG_BAD_ROTATION); dt = (x3, x4, x5); ds = 1 + x6 with scale (ds > 0 false: NRF_ALIGN_FLAG_BAD_SCALE), else 1.
 *   Compose (flag == NRF_ALIGN_FLAG_OK): q' = dq (x) q, the Hamilton product with each component summed left to right in the order
 *     w' = dw*w - dx*x - dy*y - dz*z,  x' = dw*x + dx*w + dy*z - dz*y,  y' = dw*y - dx*z + dy*w + dz*x,  z' = dw*z + dx*y - dy*x + dz*w,
 *     divided by its norm; t'_a = ds*((dR_a0*t0 + dR_a1*t1) + dR_a2*t2) + dt_a; s' = ds*s.  With any other flag the update is the identity: d_state keeps its
 *     bits and the row reports dq = (1, 0, 0, 0), ds = 1, dt = 0.
 *   History.  d_history [n_history][8] doubles or NULL; row `iteration` = (pairs kept, the sum of dot(d, d) resp. r*r, the flag, 2*sqrt((dx*dx + dy*dy) + dz*dz)
 *     of dq -- the angle of the update for a small one --, sqrt(dot(dt, dt)), ds, the new s, 0).
 * d_workspace: 8-byte aligned, nrf_align_workspace_bytes(n, mode) (0 for a shape the calls refuse).
 * REFUSED (NRF_ERR_INVALID_ARG, or NRF_ERR_WORKSPACE for a short workspace; nothing launched or written): n outside [0, 2^31 - 1]; a mode that is neither
 *   constant; rotate_only or scale outside {0, 1}; a null d_state; a null d_points, d_out, d_y, d_p or d_face with n > 0; NRF_ALIGN_PLANE with a null d_verts or
 *   d_faces, or V, F outside [0, 2^31 - 1]; a pointer that is not aligned to its element; d_history given with iteration outside [0, n_history); a pose with a
 *   non-finite entry, a zero quaternion or s <= 0; a null or misaligned workspace. */
#define NRF_ALIGN_POINT 0
#define NRF_ALIGN_PLANE 1
#define NRF_ALIGN_TILE 1024              /* pairs per block partial */
#define NRF_ALIGN_POINT_COLUMNS 19
#define NRF_ALIGN_PLANE_COLUMNS 37
#define NRF_ALIGN_JACOBI_SWEEPS 8        /* the off-diagonal of the 4x4 reaches 1e-16 of the diagonal after 4 */
#define NRF_ALIGN_JACOBI_BIG_THETA 1e150 /* above it th*th + 1 is not formed */
#define NRF_ALIGN_FLAG_OK 0
#define NRF_ALIGN_FLAG_FEW_PAIRS 1
#define NRF_ALIGN_FLAG_NO_SPREAD 2
#define NRF_ALIGN_FLAG_BAD_PIVOT 3
#define NRF_ALIGN_FLAG_BAD_SCALE 4
#define NRF_ALIGN_FLAG_BAD_ROTATION 5
NRF_API int nrf_align_state_init(const double *pose, double *d_state, void *stream);
NRF_API int nrf_align_apply(const float *d_points, int64_t n, const double *d_state, int rotate_only, float *d_out, void *stream);
NRF_API size_t nrf_align_workspace_bytes(int64_t n, int mode);
NRF_API int nrf_align_sums(const float *d_y, const float *d_p, const int32_t *d_face, int64_t n, int mode, const float *d_verts, int64_t n_verts,
                           const int32_t *d_faces, int64_t n_faces, uint32_t *d_stats, void *d_workspace, size_t workspace_bytes, void *stream);
NRF_API int nrf_align_solve(int64_t n, int mode, int scale, int iteration, int n_history, double *d_state, double *d_history, void *d_workspace,
                            size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Mesh BVH (bvh.hip, bvh.h, sort.h; no counterpart in the reference)
 * ------------------------------------------------------------------------------------------- */
/* A second acceleration structure for the two queries above: a linear bounding-volume hierarchy over the faces (Karras, Maximizing Parallelism in the Construction of
 * BVHs, Octrees, and k-d Trees, 2012), one face per leaf.  It needs no box, no dims, no large-face list and no fallback, its build makes no host round trip, and its
 * queries return the bits of nrf_closest_on_mesh / nrf_ray_cast_mesh: both results are defined grid-free as the minimum of a packed key over all valid faces, the
 * candidates are formed by the same inline functions, and a subtree is skipped only by a proven bound.  Conventions as above: fp32 operations rounded once each,
 * / correctly rounded, caller-owned buffers, refusals before any launch or write, two runs the same bytes.  The face grid stays what a Mesh gets by default.
 *
 * SORT.  nrf_sort_pairs_u32: d_keys [n] uint32 with a payload d_values [n] int32 (NULL: the payload is the index 0 .. n - 1) ordered by bits [begin_bit, end_bit) of
 *   the key into d_keys_out / d_values_out (whole keys are written, not the masked bits).  A least-significant-digit radix sort in 8-bit digits (the last digit may be
 *   narrower), STABLE: pairs with equal bits keep their input order, so d_values_out with a NULL d_values is np.argsort(bits, kind="stable").  Per pass: a digit
 *   histogram per block of 2 048 elements; the exclusive scan of the [256 digits x blocks] counts in digit-major order; a scatter that ranks every element inside its
 *   block among the equal digits before it.  No atomics on global memory, no synchronisation; the passes ping-pong between the outputs and two arrays of the workspace
 *   (nrf_sort_workspace_bytes(n)), the inputs are only read.  0 <= n <= 2^31 - 1; n == 0 launches nothing; begin_bit == end_bit copies.  REFUSED: n or the bits out
 *   of range (0 <= begin_bit <= end_bit <= 32), a null d_keys, d_keys_out or d_values_out (n > 0), an output that is its input, a null, misaligned (8 bytes) or
 *   short workspace.
 *
 * BUILD.  nrf_mesh_bvh_build fills a buffer of nrf_mesh_bvh_bytes(F) bytes with a workspace of nrf_mesh_bvh_workspace_bytes(F) bytes, both pure functions of F; the
 *   workspace may go (or be overwritten) once the build has run.  The host reads nothing back.
 *   Classes.  Valid, bad and non-finite faces exactly as for nrf_face_grid_count; d_stats [4] uint32 or NULL, ADDED to: [1] bad, [2] non-finite faces.  n_valid, the
 *   number of valid faces, is counted on the device.
 *   Mesh box.  Per axis the smallest and largest corner coordinate of the valid faces, exact: integer atomic min / max on the image of a float, u = bits(x),
 *   u = (u >> 31) ? ~u : u | 2^31, whose unsigned order is the float's with -0 below +0.  No valid face: lo = +inf, hi = -inf.
 *   Morton code of a valid face, 30 bits.  Per axis c = lo_f * 0.5f + hi_f * 0.5f, the centre of the face's coordinate box (lo_f / hi_f the smallest / largest of the
 *   three corners); e = hi - lo of the mesh box; e > 0 and e < +inf false: cell 0, else x = floorf(((c - lo) / e) * 1024.0f), cell = (int)min(max(x, 0), 1023) (a NaN
 *   x gives 0).  Bit k of the x / y / z cell is bit 3k / 3k + 1 / 3k + 2 of the code.  A face that is not valid gets the code 2^30, above every valid one.
 *   Leaves.  Four stable 8-bit passes of the sort over the codes, payload the face index: sorted position k holds face leaf_face[k], positions 0 .. n_valid - 1 the
 *   valid faces, ascending in the unique 64-bit key (code << 32) | f.  Equal codes (copies of a face, coincident centres) need no special case.
 *   Topology.  One lane per internal node i in [0, n_valid - 1): Karras's direction, range and split on the length of the common prefix of the 64-bit keys.  Node i
 *   covers a range [l, r] of sorted positions with i == l or i == r and splits it after position s, the last whose key shares the range's longest common prefix with
 *   the first key's next bit: the node of [l, s] has index s, the node of [s + 1, r] index s + 1, a range of one position is that leaf; node 0 is the root.  The tree,
 *   numbering included, equals the top-down recursion "split where the highest differing bit of the range's first and last key changes" (tests/bvh_ref.py).
 *   NRF_BVH_MAX_DEPTH.  A key has at most 62 significant bits (a valid code is below 2^30) and every level of the tree lengthens the common prefix by at least one
 *   bit, so no leaf lies deeper than 62 edges below the root.  64 bounds the refit's launches and the traversal stack (which holds at most one node per level).
 *   Boxes.  The box of a leaf is its face's coordinate box, the box of a node the per-axis min / max of its children's.  A node stores its two CHILDREN's boxes.  The
 *   refit is NRF_BVH_MAX_DEPTH launches with nothing handed over inside a launch (the L2s of the XCDs are not coherent, and a fence per thread costs microseconds):
 *   launch p finishes the nodes whose two children were finished by an earlier launch and marks them p; a mark equal to p counts as not finished, so no launch reads
 *   data the same launch wrote.  A device counter of unfinished nodes lets the launches after the tree's height return after one load per block.  min / max are exact
 *   and order-free: the buffer is the same bytes on every run (the build zeroes it first, padding and unused nodes included).
 *   Layout of the buffer (every piece starts at a multiple of 256 bytes, as the workspaces do):
 *     head       8 x int64: "NRFBVH01" (0x4e52464256483031), F, n_valid, then per axis x, y, z the mesh box as bits(lo) | bits(hi) << 32, then 0, 0
 *     leaf_face  F x int32
 *     node       max(F - 1, 0) x 64 bytes: lo0[3], hi0[3], lo1[3], hi1[3] fp32 (the boxes of child 0 and child 1), child[2], parent, 0 as int32.  A child >= 0 is an
 *                internal node, -(k + 1) the leaf at sorted position k; the root's parent is -1; nodes n_valid - 1 .. F - 2 stay zero.
 *   n_valid == 0: an empty tree, every query misses.  n_valid == 1: no internal node; the tree is leaf 0 alone and a query tests face leaf_face[0] without a box.
 *   REFUSED: V or F out of range, a null d_faces (F > 0) or d_verts (V > 0 and F > 0), a null or misaligned (64 bytes) BVH buffer, a buffer whose size is not
 *   nrf_mesh_bvh_bytes(F), a null, misaligned (8 bytes) or short workspace.  A query or nrf_bvh_point_codes whose F passes the size check but disagrees with the head
 *   (magic, F, 0 <= n_valid <= F) reads nothing more of the buffer and writes nothing.
 *
 * CLOSEST POINT.  nrf_bvh_closest_on_mesh: outputs, d_stats[0], max_dist and the result exactly as nrf_closest_on_mesh defines them; d_stats[3] is never touched,
 *   there is no fallback.  The workspace pair is accepted as it comes: nrf_bvh_query_workspace_bytes(n) is 0 and d_workspace may be NULL.
 *   Traversal.  One lane per query, a private stack of NRF_BVH_MAX_DEPTH node indices, from the root.  For a node's two child boxes [lo, hi]: per axis
 *   g = q < lo ? lo - q : (q > hi ? q - hi : 0), b2 = (gx*gx + gy*gy) + gz*gz.  The child with the smaller b2 first; a child is SKIPPED iff
 *   b2 > min(best_d2, fl(max_dist * max_dist)), strictly (best_d2 = +inf before the first candidate): an equal bound descends, so the lowest face index wins a tie.  A
 *   leaf is a candidate through the closest-point function above, folded into the same key.
 *   WHY IT IS EXACT.  The clamp of the closest-point function puts every coordinate of P inside the face's coordinate box, hence inside the box of every ancestor.
 *   Per axis, with lo <= P <= hi: q < lo gives q - P <= q - lo < 0, so |fl(q - P)| >= fl(lo - q) = g (rounding is monotone and odd); likewise q > hi; else g = 0.  The
 *   rounded square and the two rounded sums of non-negative terms are monotone in every argument, in the same order for both: b2 <= d2 for every face under the node
 *   and every finite q, also where either overflows to +inf.  A face that could win or tie has d2 <= min(best_d2, fl(max_dist^2)), so its ancestors are not skipped.
 *
 * RAY CAST.  nrf_bvh_ray_cast_mesh: rays, cull, mode, outputs, d_stats[0] and the result exactly as nrf_ray_cast_mesh defines them; no far-origin rule, no premise on
 *   the faces, no step cap, no fallback, d_stats[3] never touched.
 *   Node test, for a child box [lo, hi] and a valid ray: M = max(|o|_inf, |lo|_inf, |hi|_inf), m = 2^-10 * M (M < 2^-100: m = +inf, every node is visited: a scene
 *   at the scale of the denormals is searched exhaustively).  Per axis wlo = lo - m, whi = hi + m.  An axis with d == 0 whose o lies outside [wlo, whi]: a miss.  Else
 *   ta = (wlo - o) / d, tb = (whi - o) / d, swapped so that ta <= tb.  t_in = max(ray lo, all ta), t_out = min(ray hi, all tb).  The child is VISITED iff
 *   t_in <= t_out and t_in <= best_t (not strictly: an equal t with a lower face index must still be found; best_t = +inf before the first candidate).  The child
 *   with the smaller t_in first.  Any mode stops at the first accepted candidate.
 *   WHY THE TRAVERSAL CANNOT MISS.  Let a candidate of a face under the node be accepted at t, and take an axis with d > 0 (d < 0 mirrors).  P lies in the node's box
 *   (the clamp), so |P|_inf <= M, and the consistency rule gives |Pu - P| <= tau = 2^-12 max(|o|_inf, |Pu|_inf) <= 2^-12 (M + tau), tau <= 2^-12 (1 + 2^-11) M: on
 *   this axis Pu >= lo - tau.  Suppose t < ta.  Both are floats and ta = fl(x / d) with x = fl(wlo - o), so t < x / d exactly (a float below the rounded quotient is
 *   below the quotient), t * d < x, fl(t * d) <= x (x is a float, rounding is monotone) and Pu = fl(o + fl(t * d)) <= fl(o + x).  fl(o + fl(wlo - o)) differs from
 *   wlo by two roundings of values no larger than 2 (1 + 2^-10) M, and wlo from lo - m by one: Pu <= lo - 2^-10 M + 2^-21 M < lo - tau, a contradiction.  So
 *   ta <= t, likewise t <= tb; denormal ta or products change nothing (the argument uses monotonicity, and M >= 2^-100 keeps m and the roundings of the sums normal);
 *   an infinite wlo or whi only widens.  On an axis with d == 0, Pu = o for every finite t, so o lies within tau < m of [lo, hi].  lo_ray <= t <= hi_ray is part of the
 *   acceptance.  Hence t_in <= t <= t_out for every ancestor of an accepted candidate, and an unseen candidate that could win or tie has t <= best_t, so t_in <= best_t.
 *   No result depends on the margin.
 *
 * SPATIAL ORDER.  nrf_bvh_point_codes writes d_codes [n] uint32, the Morton code above of the point at d_points + i * stride (3 <= stride <= NRF_RC_MAX_STRIDE floats:
 *   3 for points, the ray stride for ray origins) against the mesh box in the head, the coordinate itself in place of c, clamped the same way.  Both queries take
 *   d_order, int32 [n] or NULL: lane i serves element d_order[i] and writes that element's outputs.  d_order must be a permutation of 0 .. n - 1 (an entry outside is
 *   skipped; a repeated one leaves another element unwritten): sorting the codes with nrf_sort_pairs_u32 gives one.  The outputs do not depend on it. */
#define NRF_BVH_MAX_DEPTH 64
NRF_API size_t nrf_sort_workspace_bytes(int64_t n);
NRF_API int nrf_sort_pairs_u32(const uint32_t *d_keys, const int32_t *d_values, int64_t n, int begin_bit, int end_bit, uint32_t *d_keys_out, int32_t *d_values_out,
                               void *d_workspace, size_t workspace_bytes, void *stream);
NRF_API size_t nrf_mesh_bvh_bytes(int64_t n_faces);
NRF_API size_t nrf_mesh_bvh_workspace_bytes(int64_t n_faces);
NRF_API int nrf_mesh_bvh_build(const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, void *d_bvh, size_t bvh_bytes, uint32_t *d_stats,
                               void *d_workspace, size_t workspace_bytes, void *stream);
NRF_API size_t nrf_bvh_query_workspace_bytes(int64_t n);
NRF_API int nrf_bvh_closest_on_mesh(const float *d_query, int64_t nq, const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, const void *d_bvh,
                                    size_t bvh_bytes, const int32_t *d_order, float max_dist, float *d_dist2, int32_t *d_face, float *d_uv, float *d_point,
                                    uint32_t *d_stats, void *d_workspace, size_t workspace_bytes, void *stream);
NRF_API int nrf_bvh_ray_cast_mesh(const float *d_rays, int64_t n_rays, int stride, const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces,
                                  const void *d_bvh, size_t bvh_bytes, const int32_t *d_order, int cull, int mode, float *d_t, int32_t *d_face, float *d_uv,
                                  float *d_point, uint8_t *d_hit, uint32_t *d_stats, void *d_workspace, size_t workspace_bytes, void *stream);
NRF_API int nrf_bvh_point_codes(const float *d_points, int64_t n, int stride, const void *d_bvh, size_t bvh_bytes, int64_t n_faces, uint32_t *d_codes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Point clouds (points.hip, bvh.hip, align.hip; no counterpart in the reference)
 * ------------------------------------------------------------------------------------------- */
/* What a scan, a COLMAP cloud or unprojected depth needs and a mesh tool cannot give: a hierarchy over the points themselves, the k nearest neighbours of every
 * query, normals and local shape from them, outlier scores, and the plane-mode sums of the registration from given normals.  Conventions as above: fp32 operations
 * rounded once each, caller-owned buffers, refusals before any launch or write, two runs the same bytes; every result is defined without the structure and
 * tests/points_ref.py restates it bit for bit.
 *
 * BUILD.  nrf_point_bvh_build over d_points [n, 3] fills a buffer of nrf_point_bvh_bytes(n) (== nrf_mesh_bvh_bytes(n)) bytes with a workspace of
 *   nrf_point_bvh_workspace_bytes(n).  DEFINITION: apart from its first word, "NRFPBV01" (0x4e52465042563031), the buffer is byte for byte what nrf_mesh_bvh_build
 *   writes for verts = d_points and the n faces (i, i, i).  So the leaf box is the point, its code comes from c = p * 0.5f + p * 0.5f, a point with a non-finite
 *   coordinate is not valid (code 2^30, sorted last, d_stats[2] += 1; d_stats [4] uint32 or NULL, entry 1 is never touched), and everything the Mesh BVH section
 *   states of classes, box, codes, leaves, topology, depth, boxes and layout holds with "point" for "face"; tests/bvh_ref.py restates the tree as it is.  It is the
 *   same kernels with another leaf source: no face array exists, no host round trip.  nrf_point_bvh_codes is nrf_bvh_point_codes against the box of a point buffer
 *   (d_order for nrf_bvh_knn, as SPATIAL ORDER describes).  The two magics keep a mesh buffer out of the point queries and the reverse.
 *   REFUSED: n outside [0, 2^31 - 1], a null (n > 0) or misaligned d_points, a null or misaligned (64 bytes) buffer, a size that is not nrf_point_bvh_bytes(n), a
 *   null, misaligned (8 bytes) or short workspace.
 *
 * K NEAREST.  nrf_bvh_knn, 1 <= k <= NRF_KNN_MAX_K.  d2(q, j) is the squared distance of nrf_nearest_points: dx = qx - px, .., d2 = (dx*dx + dy*dy) + dz*dz.  For a
 *   finite query i the candidates are the points j with finite coordinates, d2 <= fl(max_dist * max_dist), and -- exclude_self == 1 -- j != i (the query IS point i
 *   of the cloud).  Slots 0 .. k - 1 of row i of d_dist2 / d_index [nq, k] hold, ascending, the k smallest keys (bits(d2) << 32) | j over the candidates, as d2 and j;
 *   slots past the last candidate hold +inf / -1; d_count [nq] (or NULL) the number of filled slots.  A non-finite query: every slot empty, count 0,
 *   d_stats[0] += 1 (d_stats [4] uint32 or NULL; nothing else is touched).  The same bits whatever the tree, d_order or the scheduling; with k == 1 and
 *   exclude_self == 0 the outputs are those of nrf_nearest_points bit for bit.  d_order as for the mesh queries.  The workspace pair is accepted as it comes
 *   (nrf_bvh_query_workspace_bytes is 0).
 *   Traversal.  As nrf_bvh_closest_on_mesh: one lane per query, a stack of NRF_BVH_MAX_DEPTH node indices, the child with the smaller b2 first.  A child is SKIPPED
 *   iff b2 > min(d2 of the k-th best key held, fl(max_dist^2)), strictly; the k-th best is +inf until k candidates are held.  An equal bound descends, so a lower
 *   index still displaces an equal distance.
 *   WHY IT IS EXACT.  For a point leaf lo == hi == p: q < p gives g = fl(p - q) = -fl(q - p), q > p gives g = fl(q - p), q == p gives g = 0 = |fl(q - p)| (rounding
 *   is odd), so g*g == dx*dx per axis and the same two sums follow: b2 == d2 bit for bit, and the traversal takes the bound of a leaf child as the candidate's d2.
 *   For an ancestor the monotonicity argument of the mesh query applies unchanged (p lies inside every ancestor's box): b2 <= d2.  A candidate that belongs to the
 *   result has a key <= the k-th best key held at any time, so d2 <= its value and d2 <= fl(max_dist^2): no ancestor is skipped.
 *   The list.  k keys in registers, instantiated for 1, 8, 16 and 32 entries (the smallest that holds k), kept in descending order by an unrolled compare-and-select
 *   insertion: no indexed private array, no LDS (DESIGN 8u has the compiler's resource figures).
 *
 * NORMALS.  nrf_points_normals: d_index [n, k] is what nrf_bvh_knn wrote for the cloud against itself with exclude_self == 1.  For point i the set is i itself, then
 *   the slots of row i with 0 <= index < n in slot order; m its size.  All values converted to fp64 first.  mean = (the sum in that order from p_i) / m per
 *   component; with d = x - mean, the six sums cxx, cxy, cxz, cyy, cyz, czz of d_a*d_b in the same order from the first term.  Cyclic Jacobi on the symmetric 3x3 with
 *   V = I: NRF_POINTS_JACOBI_SWEEPS sweeps over the pairs (0,1), (0,2), (1,2), the rotation of nrf_align_solve verbatim (a zero off-diagonal is skipped, the
 *   NRF_ALIGN_JACOBI_BIG_THETA branch, columns of A, rows of A, columns of V).  Eigenvalues l0 <= l1 <= l2 = the diagonal ascending, the lowest column first on a
 *   tie.  The normal is column l0 of V divided by sqrt((x*x + y*y) + z*z) per component, its sign chosen in fp64, then rounded to fp32 once.  SIGN: with d_toward
 *   (toward_stride 0: one viewpoint [3]; 3: one per point [n, 3]) negated where dot(n, toward - p_i) < 0 (the dot of the registration, the difference in fp64);
 *   without, negated where the component of largest magnitude (the lowest axis on a tie) is negative.  Orientation by propagation is not offered.
 *   DEGENERATE: m < 3, a non-finite coordinate in the set, a non-finite eigenvalue or norm, a norm that is not > 0, or l1 > 0 false (coincident or collinear
 *   points): the normal and the eigenvalues are zeros and d_stats[0] += 1 (d_stats [1] uint32 or NULL).  d_eigen [n, 3] (or NULL) gets (float)l0, l1, l2: sums, not
 *   divided by m; surface variation is l0 / (l0 + l1 + l2).
 *   NRF_POINTS_JACOBI_SWEEPS.  Census over every neighbourhood of the test clouds (tests/test_points_host.py: 3 372 sets at k = 8 and 16): the largest
 *   off-diagonal magnitude relative to the largest diagonal magnitude, worst set after sweeps 1 .. 6: 3.2e-1, 3.4e-2, 9.5e-7, 1.9e-22, 3.2e-38, 1.3e-54.  It stays
 *   below 1e-16 on every set from sweep 4 on; the constant is that count plus a margin of 2 (a sweep converges quadratically and costs three rotations).
 *
 * SCORES.  nrf_knn_mean_distance: s_i = (the fp32 sum from 0 of sqrtf(d2) over the slots of row i with d2 < +inf, in slot order) / (float)count; +inf where none.
 *   count here is the number of slots with d2 < +inf, read from d_dist2 alone.  It can be BELOW nrf_bvh_knn's d_count: with max_dist = +inf a d2 that overflows to
 *   +inf (coordinates apart by about 1e19 or more) fills a slot with a valid index, which d_count counts and the score leaves out.
 *   nrf_value_stats: d_out [4] doubles = count, sum of (double)v, sum of (double)v * (double)v and max(0, largest v) over the finite entries of d_values [n], in the
 *   order of nrf_distance_stats (4 096 entries per block, the ordered sum); no atomics, no synchronisation.  Workspace: nrf_value_stats_workspace_bytes(n), 8-byte aligned.
 *
 * PLANE SUMS FROM GIVEN NORMALS.  nrf_align_sums_normals forms the 37 columns of NRF_ALIGN_PLANE in the same order into the same workspace
 *   (nrf_align_workspace_bytes(n, NRF_ALIGN_PLANE)); nrf_align_solve follows unchanged.  Pair i is (d_y[i], d_p[i]) with the normal d_n[i] [n, 3], already
 *   gathered for the pair; d_index[i] < 0: no pair (d_stats[0]); a non-finite y or p: [1]; c = the converted d_n[i], len2 = (cx*cx + cy*cy) + cz*cz; len2 > 0 false
 *   or len2 not finite: [3]; n = c / sqrt(len2).  [2] is never touched.  The SIGN of a normal changes no column: the row a and the residual r are both odd in n, and
 *   every column is a product of two of them (or constant); negation is exact.
 *
 * REFUSED (nothing launched or written): a count or k out of range, an exclude_self or toward_stride outside its values, a negative or NaN max_dist, a required
 *   pointer that is null, a pointer not aligned to its element, a buffer of the wrong size; a buffer with the wrong magic or head is read no further and nothing is
 *   written. */
#define NRF_KNN_MAX_K 32
#define NRF_POINTS_JACOBI_SWEEPS 6
NRF_API size_t nrf_point_bvh_bytes(int64_t n);
NRF_API size_t nrf_point_bvh_workspace_bytes(int64_t n);
NRF_API int nrf_point_bvh_build(const float *d_points, int64_t n, void *d_bvh, size_t bvh_bytes, uint32_t *d_stats, void *d_workspace, size_t workspace_bytes,
                                void *stream);
NRF_API int nrf_point_bvh_codes(const float *d_query, int64_t nq, int stride, const void *d_bvh, size_t bvh_bytes, int64_t n, uint32_t *d_codes, void *stream);
NRF_API int nrf_bvh_knn(const float *d_query, int64_t nq, const float *d_points, int64_t n, const void *d_bvh, size_t bvh_bytes, const int32_t *d_order, int k,
                        float max_dist, int exclude_self, float *d_dist2, int32_t *d_index, int32_t *d_count, uint32_t *d_stats, void *d_workspace,
                        size_t workspace_bytes, void *stream);
NRF_API int nrf_points_normals(const float *d_points, int64_t n, const int32_t *d_index, int k, const float *d_toward, int toward_stride, float *d_normals,
                               float *d_eigen, uint32_t *d_stats, void *stream);
NRF_API int nrf_knn_mean_distance(const float *d_dist2, int64_t n, int k, float *d_score, void *stream);
NRF_API size_t nrf_value_stats_workspace_bytes(int64_t n);
NRF_API int nrf_value_stats(const float *d_values, int64_t n, double *d_out, void *d_workspace, size_t workspace_bytes, void *stream);
NRF_API int nrf_align_sums_normals(const float *d_y, const float *d_p, const float *d_n, const int32_t *d_index, int64_t n, uint32_t *d_stats, void *d_workspace,
                                   size_t workspace_bytes, void *stream);

/* RenderRays (NeRFRenderer.h:366-459) over one chunk of n packed rays [n, 8 | 11].
 * d_t: [n_samples] linspace(0,1,n_samples); d_u: [n_importance] linspace(0,1,n_importance). */
NRF_API size_t nrf_render_rays_workspace_bytes(const nrf_renderer *r, int64_t n, const nrf_render_params *p);
NRF_API int nrf_render_rays(const nrf_renderer *r, const float *d_rays, int ray_stride, int64_t n, const nrf_render_params *p,
                            const float *d_t, const float *d_u, const nrf_render_outputs *out,
                            void *d_workspace, size_t workspace_bytes, void *stream);

/* BatchifyRays (NeRFRenderer.h:465-525): the host loop over Chunk-sized slices of a packed ray batch, inside the library -- every output of `out`
 * is the whole batch's buffer ([n, ...]), slice i of the loop writes its rows in place (what the reference's torch::cat assembles afterwards), and
 * p->ray_base advances with the slice so the counter-based draws of the stochastic branches do not depend on Chunk.  Workspace: one chunk's per lane
 * (nrf_set_render_lanes).  A renderer is bound to ONE device and ONE caller at a time: its lane streams and fork / join events are created on first use, follow the
 * renderer to another device when a later call comes from there, and are shared by every call -- concurrent calls on one renderer from several host threads are not supported. */
NRF_API size_t nrf_batchify_rays_workspace_bytes(const nrf_renderer *r, int64_t n, int chunk, const nrf_render_params *p);
NRF_API int nrf_batchify_rays(const nrf_renderer *r, const float *d_rays, int ray_stride, int64_t n, int chunk, const nrf_render_params *p,
                              const float *d_t, const float *d_u, const nrf_render_outputs *out, void *d_workspace, size_t workspace_bytes, void *stream);

/* NeRFRenderer::Render for a pose (NeRFRenderer.h:530-605), restricted to the row tile of `v`: nrf_view_rays + nrf_batchify_rays + the tile's
 * Near / Far in ONE call -- what a rank of the row-tile sharding issues per frame; ~25 asynchronous launches, no synchronisation, no allocation.
 * out: buffers for the TILE's rows*w rays.  d_rays_out (optional): receives the packed rays [rows*w, 8|11] (else they live in the workspace).
 * d_near_far (optional): see nrf_view_rays.  p->ray_base is taken as the index of the FRAME's first ray; the tile adds row0 * w itself.
 * ndc together with cone rays (p->has_cone): NDCRays' factor on cone_angle is the NDC direction's norm over itself (RayUtils.h:73-81), exactly 1: p->cone_angle is used as is. */
NRF_API size_t nrf_render_rows_workspace_bytes(const nrf_renderer *r, const nrf_view *v, const nrf_render_params *p);
NRF_API int nrf_render_rows(const nrf_renderer *r, const nrf_view *v, const nrf_render_params *p, const float *d_t, const float *d_u,
                            const nrf_render_outputs *out, float *d_rays_out, float *d_near_far, void *d_workspace, size_t workspace_bytes, void *stream);
/* The three render entries with normal maps (nrf_render_normals above); same arguments and results otherwise. */
NRF_API size_t nrf_render_rays_normals_workspace_bytes(const nrf_renderer *r, int64_t n, const nrf_render_params *p, int bits);
NRF_API int nrf_render_rays_normals(const nrf_renderer *r, const float *d_rays, int ray_stride, int64_t n, const nrf_render_params *p, const float *d_t, const float *d_u,
                                    const nrf_render_outputs *out, const nrf_render_normals *normals, void *d_workspace, size_t workspace_bytes, void *stream);
NRF_API size_t nrf_batchify_rays_normals_workspace_bytes(const nrf_renderer *r, int64_t n, int chunk, const nrf_render_params *p, int bits);
NRF_API int nrf_batchify_rays_normals(const nrf_renderer *r, const float *d_rays, int ray_stride, int64_t n, int chunk, const nrf_render_params *p, const float *d_t,
                                      const float *d_u, const nrf_render_outputs *out, const nrf_render_normals *normals, void *d_workspace, size_t workspace_bytes,
                                      void *stream);
NRF_API size_t nrf_render_rows_normals_workspace_bytes(const nrf_renderer *r, const nrf_view *v, const nrf_render_params *p, int bits);
NRF_API int nrf_render_rows_normals(const nrf_renderer *r, const nrf_view *v, const nrf_render_params *p, const float *d_t, const float *d_u, const nrf_render_outputs *out,
                                    const nrf_render_normals *normals, float *d_rays_out, float *d_near_far, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Training step: NeRFExecutor::Train, NeRFExecutor.h:862-995.
 *   render (nrf_render_rays) -> huber loss -> backward of the FINE pass only (z_samples are detached, NeRFRenderer.h:429):
 *   RawToOutputs -> sigma mask -> MLP -> hash grid -> Adam(lr, betas (0.9, 0.99), eps 1e-15) (:539).
 * All gradients fp32; accumulations use hardware fp32 atomics (order-free definition: compare with a tolerance).
 * ------------------------------------------------------------------------------------------- */
/* torch::nn::functional::huber_loss (delta 1, mean) and torch::mse_loss (:882-887).  d_loss_mse: device [2] = (huber, mse);
 * d_grad (optional): d huber / d pred, same shape as pred. */
NRF_API int nrf_huber_loss(const float *d_pred, const float *d_target, int64_t count, float *d_loss_mse, float *d_grad, void *stream);

/* Backward of RawToOutputs (NeRFRenderer.h:199-282) w.r.t. raw given d loss / d RGBMap [n,3]; TruncExp::backward clamps its
 * argument to [-100, 5] (CustomOps.cpp:11-15). */
NRF_API int nrf_raw2outputs_backward(const float *d_raw, const float *d_z, const float *d_dirs, int d_stride, int64_t n, int s, int c, int white_bkgr,
                                     const float *d_g_rgb, float *d_g_raw, void *stream);
/* ... of a forward that ran with raw_noise_std > 0: d_noise [n,s] are the same normal draws (nrf_rng_fill(seed, NRF_RNG_NOISE_FINE, ...)). */
NRF_API int nrf_raw2outputs_backward_noise(const float *d_raw, const float *d_z, const float *d_dirs, int d_stride, int64_t n, int s, int c,
                                           int white_bkgr, const float *d_noise, float noise_std, const float *d_g_rgb, float *d_g_raw, void *stream);
/* d/d sigma = 0 where keep is false: the backward of `outputs_flat[~keep_mask, -1] = 0` (NeRFRenderer.h:187-188). */
NRF_API int nrf_mask_sigma_grad(const uint8_t *d_keep, int64_t p, int c, float *d_g_raw, void *stream);

/* Backward of the MLP, fp32: NeRFSmallImpl::forward (NeRF.cpp:322-412) or -- round 5 -- the classic NeRFImpl::forward (NeRF.cpp:92-126: biases, the skip concat
 * cat[input_pts, h], the view-direction head or output_linear).  x [p, in_dims] as given to nrf_mlp_forward, g_out [p, output dims] (4 with view directions).
 * d_g_params (blob layout) is ACCUMULATED into; d_g_x (optional) receives d loss / d x[:, :input_ch] as [p, input_ch].  Pinned by LibTorch autograd through the compiled
 * NeRF.cpp (goldens train_hash, mlp_nerf_bwd*, train_classic). */
NRF_API size_t nrf_mlp_backward_workspace_bytes(const nrf_mlp *m, int64_t p);
NRF_API int nrf_mlp_backward(const nrf_mlp *m, const float *d_x, const float *d_g_out, int64_t p, float *d_g_params, float *d_g_x,
                             void *d_workspace, size_t workspace_bytes, void *stream);
/* Training the predicted-normals head (normal_loss.hip): the two losses of NeRF.h:308-326 whose call site the reference left commented out (NeRFExecutor.h:929-952)
 * because it never computed the density normals they need.  Per batch of n rays x s samples, coarse-only NRF_PREC_F32 renders of a 7-column NeRFSmall:
 *   w = d_weights [n,s] (the render's, a constant), nrm = -g / max(|g|, 1e-8) with g = d_density_grad [n*s,3] (nrf_density_grad at the points the network saw, a
 *   constant: the NRF_NORMALS_DENSITY definition without the composite), pred = d_raw[..., 4:7] as it is (not normalised), v = -d_dirs (rays_d as the batch holds it):
 *   L_pn = mean over n*s*3 of (w pred - w nrm)^2                        PredNormalLoss, torch::mse_loss
 *   L_or = mean over rays of sum_i w_i min(0, pred_i . v)^2             OrientationLoss on the PREDICTED normals, torch::mean over rays
 * d_losses: device [2] = (L_pn, L_or), unweighted.  d_g_raw [n*s,7]: columns 4:7 receive d (pred_normal_weight L_pn + orientation_weight L_or) / d pred; columns 0:4
 * are not touched (nrf_raw2outputs_backward(c = 7) fills them, and zeroes 4:7: call it first; nrf_mask_sigma_grad(c = 7) afterwards mirrors the forward's column -1
 * mask, which with 7 columns is the normal's z).  A sample with w == 0 contributes exactly 0 whatever pred and g hold.  The sums are fp64 in a fixed order (block
 * partials in the workspace, one ordered pass): two runs give the same bits.  c != 7: NRF_ERR_UNSUPPORTED. */
NRF_API size_t nrf_normal_losses_workspace_bytes(int64_t n, int s);
NRF_API int nrf_normal_losses(const float *d_weights, const float *d_density_grad, const float *d_raw, int c, const float *d_dirs, int d_stride, int64_t n, int s,
                              float pred_normal_weight, float orientation_weight, float *d_g_raw, float *d_losses, void *d_workspace, size_t workspace_bytes, void *stream);
/* Two regularisers on how density is distributed along a ray (ray_reg.hip), both functions of one ray's (sigma_i, w_i, z_i): the distortion loss of mip-NeRF 360 on the
 * render's weights and the reference's SigmaSparsityLoss (NeRF.h:302-306, a Cauchy loss on sigma that the reference declares and never calls).  Per batch of n rays x s samples:
 *   alpha_i, T_i, w_i are recomputed from d_raw[..., 3], d_z, |d_dirs| and the optional draws d_noise [n,s] (NULL: none) exactly as nrf_raw2outputs(_noise) /
 *   nrf_raw2outputs_backward_noise do: d_weights_out (optional, [n,s]) receives the render's Weights bit for bit.
 *   t_i = (z_i - z_0) / (z_{s-1} - z_0); sample i owns [t_i, t_{i+1}]: m_i = (t_i + t_{i+1}) / 2, dl_i = t_{i+1} - t_i; the last sample (the 1e10 tail) has m = t_{s-1},
 *   dl = 0.  A ray whose span z_{s-1} - z_0 is not > 0 (a missed ray, s == 1) contributes 0 to both losses and its gradient rows are not touched.
 *   L_dist   = mean over the n rays of [ sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 dl_i ]      evaluated in O(s) by prefix / suffix sums (z ascends)
 *   L_sparse = mean over the n rays of sum_i log(1 + 2 sp_i^2), sp_i = max(raw[i,3], 0)                 (the density compositing uses, without the noise draw)
 * d_losses: device [2] = (L_dist, L_sparse), unweighted.  d (distortion_weight L_dist + sparsity_weight L_sparse) / d raw[..., 3] is ADDED to column 3 of d_g_raw [n,s,c]
 * -- L_dist through nrf_raw2outputs_backward's own chain from d/dw (TruncExp's clamped derivatives, the 1 - alpha >= 1e-10 guard, the relu mask on sigma + noise); z
 * carries no gradient.  No other column is read or written: call it after nrf_raw2outputs_backward(_noise) (and nrf_normal_losses) and before nrf_mask_sigma_grad*, which
 * then zeroes the regularisers' gradient outside the box with the image loss's.  c is 4 or 7 (NRF_ERR_UNSUPPORTED otherwise).  A weight of exactly 0 skips its term and
 * leaves its loss word 0; both 0: NRF_OK without a launch, both words 0, d_g_raw and d_weights_out untouched, no workspace needed.  A negative or non-finite weight or
 * s < 1: NRF_ERR_INVALID_ARG; a workspace below nrf_ray_regularizers_workspace_bytes(n, s) (one fp32 row per ray + one fp64 pair per four rays): NRF_ERR_WORKSPACE; nothing
 * is launched then.  The loss sums are fp64 block partials combined in one ordered pass, no atomics: two runs give the same bits in d_losses and d_g_raw. */
NRF_API size_t nrf_ray_regularizers_workspace_bytes(int64_t n, int s);
NRF_API int nrf_ray_regularizers(const float *d_raw, const float *d_z, const float *d_dirs, int d_stride, int64_t n, int s, int c, const float *d_noise, float noise_std,
                                 float distortion_weight, float sparsity_weight, float *d_g_raw, float *d_losses, float *d_weights_out, void *d_workspace,
                                 size_t workspace_bytes, void *stream);
/* nrf_mlp_backward for a NeRFSmall WITH the predicted-normals head and a g_out [p,7] whose columns 4:7 carry a gradient: they go back through the normals net (its
 * weight gradients are accumulated into d_g_params), and the gradient of its input cat[sigma, geo_feat, input_pts] (NeRF.cpp:396) is added to the sigma net's output
 * gradient and to d_g_x.  With g_out[:, 4:7] == 0 the first two nets' gradients and d_g_x equal nrf_mlp_backward's and the head's are 0.  (nrf_mlp_backward on such a
 * handle reads the same 7-column rows and leaves the head's gradient at 0.)  fp32 layer products only; a handle without the head: NRF_ERR_UNSUPPORTED. */
NRF_API size_t nrf_mlp_backward_pn_workspace_bytes(const nrf_mlp *m, int64_t p);
NRF_API int nrf_mlp_backward_pn(const nrf_mlp *m, const float *d_x, const float *d_g_out, int64_t p, float *d_g_params, float *d_g_x,
                                void *d_workspace, size_t workspace_bytes, void *stream);
/* nrf_mlp_backward's gradients on the matrix cores (fp16 operands, fp32 accumulation, power-of-two loss scaling chosen on the device from
 * max|g_out|): one fused kernel per 2^22 points, forward + gradient chain + weight gradients.  Built for in 32 / views 16 / 64-wide /
 * 2-3 sigma + 3-4 colour layers; NRF_ERR_UNSUPPORTED otherwise.  Same arguments as nrf_mlp_backward.  The workspace is a fixed ~25 MB (one slot of operand
 * fragments per resident wave), whatever p. */
NRF_API size_t nrf_mlp_backward_f16_workspace_bytes(const nrf_mlp *m, int64_t p);
NRF_API int nrf_mlp_backward_f16(const nrf_mlp *m, const float *d_x, const float *d_g_out, int64_t p, float *d_g_params, float *d_g_x,
                                 void *d_workspace, size_t workspace_bytes, void *stream);
/* ... with the network input given the way the renderer's fast path has it instead of as [p, 48] fp32 rows: d_feats_lm = the level-major fp16 hash features of
 * nrf_hash_encode_lm_f16 ([16][p][2] halfs), d_dirs_f16 = [p / s][16] fp16 direction features, one row per RAY (point i belongs to ray i / s). */
NRF_API int nrf_mlp_backward_f16_lm(const nrf_mlp *m, const void *d_feats_lm, const void *d_dirs_f16, int s, const float *d_g_out, int64_t p, float *d_g_params,
                                    float *d_g_x, void *d_workspace, size_t workspace_bytes, void *stream);
/* Overflow report of the last nrf_mlp_backward_f16(_lm) that used `d_workspace` (the chain runs on fp16 operands behind a loss scale taken from max |g_out|):
 * flags_out[0] != 0: the incoming gradient held an inf / NaN; flags_out[1] != 0: an accumulated parameter gradient is not finite.  Host array of 2; synchronises
 * `stream`.  A caller skips (or rescales) the optimizer step when either is set. */
/* nrf_mlp_backward_f16_lm with the features read through a column map: point q reads column d_src[q] of the level-major table [16][pstride] (what
 * nrf_renderer_last_features hands over); nrf_mask_sigma_grad_src: nrf_mask_sigma_grad with the keep mask given by column the same way. */
NRF_API int nrf_mlp_backward_f16_lm_src(const nrf_mlp *m, const void *d_feats_lm, int64_t pstride, const int32_t *d_src, const void *d_dirs_f16, int s, const float *d_g_out, int64_t p,
                                        float *d_g_params, float *d_g_x, void *d_workspace, size_t workspace_bytes, void *stream);
NRF_API int nrf_mask_sigma_grad_src(const uint8_t *d_keep_cols, const int32_t *d_src, int64_t p, int c, float *d_g_raw, void *stream);
NRF_API int nrf_mlp_backward_f16_flags(const void *d_workspace, uint32_t *flags_out, void *stream);
/* The same two words without a host wait in the training step: _async copies them to h_flags2 (two uint32; pinned memory keeps the copy asynchronous) in `stream`'s order
 * -- read them after the stream, or an event recorded behind the call, has passed; _device returns where they live on the device, for nrf_adam_step_guarded: the
 * optimizer step is then skipped ON THE DEVICE when the chain overflowed, and the host learns of it one step later (nerfpp_amd/train.py). */
NRF_API int nrf_mlp_backward_f16_flags_async(const void *d_workspace, uint32_t *h_flags2, void *stream);
NRF_API const uint32_t *nrf_mlp_backward_f16_flags_device(const void *d_workspace);
/* Replace the parameter blob (same layout) and refresh the derived operands (transposed layers, matrix-core images).
 * NeRFSmall handles do it ON THE DEVICE in stream order (a gather + hi / lo split per image, no host round trip, nothing waits): work already issued on `stream`
 * reads the old images, work issued after reads the new ones; other streams of the caller's are the caller's to order.  The LeRF head of the built dimensions does it
 * on the device too when `params` is a device pointer (its Gram matrix W^T W in double with the host packer's summation order, the images by the host packer's own layout
 * function compiled for the device; checked byte for byte against the host packer when the handle is created) with ONE 4-byte read-back (the Gram matrix's
 * power-of-two scale is a launch argument).  The classic 8 x 256 network does it on the device as NeRFSmall does (its three images are gathers of [blob | merged
 * views layer]: the gather maps are decoded from the host packers run on probe blobs and verified against the host-packed images when the handle is created; the merged
 * layer is re-derived by a device kernel with the host's double sums).  Anything else (and NRF_MLP_HOST_REPACK=1) copies the blob to the host, repacks there and
 * synchronises `stream`. */
NRF_API int nrf_mlp_set_params(nrf_mlp *m, const float *params, int params_on_device, void *stream);
/* Number of derived images nrf_mlp_set_params refreshes on the device for this handle (0: the host repack). */
NRF_API int nrf_mlp_device_repack_images(const nrf_mlp *m);
/* NRF_PREC_F16_SPLIT, NeRFSmall (bias-free: NeRF.cpp:322-412): range safety.  ReLU is positively homogeneous, so the split-precision operand image holds 2^e_l W_l per
 * layer and the kernels take the product of the scales out of (rgb, sigma) again -- exact in fp32 -- while every fp16 (hi, lo) pair the matrix cores read (weights, and the
 * activations between layers) has two NORMAL halves whatever the magnitude of the checkpoint's weights: a model trained with xavier gain 0.1 (|W| ~ 0.01), a sigma head
 * scaled by 100, weights x 2^-8 or x 2^6 all render as accurately as weights near 1.  The exponents are chosen on the device from the blob itself at create time and at
 * every nrf_mlp_set_params (per-layer RMS row norms -> an RMS model of the activations, target RMS 8; mlp.hip, k_small_scales), in stream order.
 * nrf_mlp_set_input_rms_hint: the expected RMS of the position features (default 0.25; a renderer built on a hash grid sets it from the table).
 * nrf_mlp_get_split_scales: the exponents in force as powers of two -- group_scales_out[12] (sigma-net layers, colour layer 0's direction columns / geo columns, colour
 * layers 1..), kernel_scales_out[8] ([0] 2^-S_sigma, [1] 2^-S_colour, [2] 2^S_hidden); synchronises `stream`.  All 1 for other families and with NRF_SPLIT_UNSCALED=1. */
NRF_API int nrf_mlp_set_input_rms_hint(nrf_mlp *m, float rms, void *stream);
/* on = 0: the split images from the blob as it is (all exponents 0) -- the representation of rounds 4-5, kept as an A/B switch and for tests of the non-finite word */
NRF_API int nrf_mlp_set_split_scaling(nrf_mlp *m, int on, void *stream);
NRF_API int nrf_mlp_get_split_scales(const nrf_mlp *m, float *group_scales_out, float *kernel_scales_out, void *stream);

/* Backward of the hash grid w.r.t. its table: d_g_emb [p, L*F] -> d_g_table, fp32 in the table's own layout, ACCUMULATED into.
 * NRF_HASH_NGP: nn::Embedding's index_add of the trilinear weights (NeRF.cpp:279-298).  NRF_HASH_CU: CuHashEmbedderBackwardKernel
 * (CuHashEmbedder.cu:105-216) -- contributions rounded to fp16 after the x128 gradient scaling exactly as there, but accumulated
 * in fp32 instead of with fp16 atomics. */
NRF_API int nrf_hash_backward(const nrf_hash *h, const float *d_x, int64_t p, const float *d_g_emb, float *d_g_table, void *stream);

/* The same gradient for points that are the samples of rays, pts [n, s, 3] ray-major (what a training step has): consecutive samples
 * of a ray that share a voxel are summed in registers before the atomic add -- the count of scattered float atomics is the cost. */
NRF_API int nrf_hash_backward_rays(const nrf_hash *h, const float *d_pts, int64_t n, int s, const float *d_g_emb, float *d_g_table, void *stream);
/* ... with both features of an entry (n_features == 2) in ONE 64-bit integer atomic: two 32-bit fixed-point fields, scaled by a power of
 * two that a device-side pass derives from a rigorous bound on any entry's total (sum over the points of max_f |g|, per level), so the fields
 * cannot overflow; decoded and ACCUMULATED into d_g_table (fp32) at the end.  Half the atomics of nrf_hash_backward_rays -- the L2 atomic
 * rate, not bytes, bounds this pass.  Resolution: (bound / 2^30) per addend, i.e. ~(active entries of a level) * 2^-30 relative to a typical
 * entry.  d_workspace: nrf_hash_backward_packed_workspace_bytes(h), 256-byte aligned; no host synchronisation. */
NRF_API size_t nrf_hash_backward_packed_workspace_bytes(const nrf_hash *h);
NRF_API int nrf_hash_backward_rays_packed(const nrf_hash *h, const float *d_pts, int64_t n, int s, const float *d_g_emb, float *d_g_table,
                                          void *d_workspace, size_t workspace_bytes, void *stream);
/* The same gradient with the contributions MERGED before they reach memory: 8-byte records {word in bin, two 25-bit fixed-point fields} are binned by ranges of 2^14 table words
 * (count pass, scan, emit pass), each bin is summed in one workgroup's LDS and added to d_g_table without atomics.  Same groups, same scale, integer sums:
 * the result equals nrf_hash_backward_rays_packed bit for bit.  log2_hashmap_size <= 19.  Workspace: nrf_hash_backward_binned_workspace_bytes(h, s)
 * (~0.27 GB at s = 192: 2^18 points x 8 corners x levels x 8 bytes), 256-byte aligned. */
NRF_API size_t nrf_hash_backward_binned_workspace_bytes(const nrf_hash *h, int s);
/* ... for batches of at most n rays: the record buffer (8 B x 8 corners x levels per sample) is sized for min(n, one 2^18-point pass) instead of the whole pass */
NRF_API size_t nrf_hash_backward_binned_workspace_bytes_for(const nrf_hash *h, int64_t n, int s);
NRF_API int nrf_hash_backward_rays_binned(const nrf_hash *h, const float *d_pts, int64_t n, int s, const float *d_g_emb, float *d_g_table,
                                          void *d_workspace, size_t workspace_bytes, void *stream);

/* TotalVariationLoss of the LibTorch HashEmbedder (NeRF.h:255-300, NeRFExecutor.h:896-913; NRF_HASH_NGP grids): the cube of
 * (cube_size + 1)^3 lattice vertices at min_vertex (host [3]; the reference draws it with torch::randint) of `level`.
 * d_loss (device, 1 float) += weight * loss;  d_g_table (optional, table layout) += weight * d loss / d table. */
NRF_API int nrf_hash_tv_loss(const nrf_hash *h, const float *d_table, int level, const int *min_vertex, int cube_size, float weight, float *d_loss,
                             float *d_g_table, void *stream);

/* torch::optim::Adam::step without weight decay / amsgrad; t = 1, 2, ... */
NRF_API int nrf_adam_step(float *d_p, const float *d_g, float *d_m, float *d_v, int64_t n, float lr, float beta1, float beta2, float eps, int t,
                          void *stream);
/* nrf_adam_step that updates NOTHING (parameters and moments alike) when any of the n_flags (<= 16) words at d_flags is non-zero at the time the kernel runs */
NRF_API int nrf_adam_step_guarded(float *d_p, const float *d_g, float *d_m, float *d_v, int64_t n, float lr, float beta1, float beta2, float eps, int t,
                                  const uint32_t *d_flags, int n_flags, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Image-space tail of NeRFExecutor::RenderPath (NeRFExecutor.h:690, :698-700; TorchTensorToCVMat, NeRFRenderer.h:58-68)
 * ------------------------------------------------------------------------------------------- */
/* depth' = (depth - near) / (far - near) with the frame's scalar Near / Far (nrf_near_far_range).  In place allowed. */
NRF_API int nrf_normalize_depth(const float *d_depth, int64_t n, float near_, float far_, float *d_out, void *stream);
/* u8 = (uint8)clamp(x * 255, 0, 255): what cv::imwrite receives for RGB / disparity / normalised depth. */
NRF_API int nrf_to_u8(const float *d_x, int64_t n, uint8_t *d_out, void *stream);

/* The render-factor step of NeRFExecutor::RenderView (NeRFExecutor.h:618-627), host only: with render_factor != 0 the frame is rendered
 * downsampled, h1 = (int)(h / render_factor), w1 = (int)(w / render_factor) (int / float -> float -> int, as the reference's
 * `h = h / rparams.RenderFactor` does with its float field) and fx, fy, cx, cy of K (host [9], row-major) are divided by it in fp32;
 * render_factor == 0 copies.  NeRFExecutor::RenderPath (:657-662) scales h, w and a local focal but hands Render() the ORIGINAL k --
 * callers that mirror RenderPath pass k unchanged and only use h1 / w1 (K1 may be NULL). */
NRF_API int nrf_render_view_dims(int h, int w, const float *K, float render_factor, int *h1, int *w1, float *K1);

/* ---------------------------------------------------------------------------------------------
 * Multi-GPU: whole-image render batches partitioned by ray into contiguous row tiles, one process per GPU, the model replicated
 * read-only; per-tile pixels return to every rank with ONE RCCL collective per step over xGMI (north_star).  The reference
 * is single-GPU (no counterpart).  RCCL is resolved with dlopen at first use -- the copy already mapped into the process (LibTorch's)
 * if there is one -- so this library has no link-time RCCL dependency; without RCCL the nrf_comm_* calls return NRF_ERR_UNSUPPORTED.
 * NRF_RCCL_LIBRARY=<path> in the environment names the copy to use instead (a host that maps several; the tests' threads-as-ranks stand-in).
 * ------------------------------------------------------------------------------------------- */
/* Rank `rank` of `world` renders image rows [row0, row0 + rows): contiguous, the first h % world ranks one row taller.  Host only. */
NRF_API int nrf_tile_partition(int h, int world, int rank, int *row0, int *rows);

#define NRF_COMM_ID_BYTES 128
typedef struct nrf_comm nrf_comm;
/* Rendezvous as in NCCL: rank 0 calls nrf_comm_unique_id (id_out: host [NRF_COMM_ID_BYTES]) and hands the bytes to every rank by any
 * out-of-band means (a file, a socket, torch.distributed, MPI); every rank then calls nrf_comm_create on ITS device
 * (hipSetDevice first; blocks until all `world` ranks arrive).  nrf_comm_wrap adopts a live ncclComm_t the host already owns
 * (it is not destroyed by nrf_comm_destroy). */
NRF_API int nrf_comm_unique_id(void *id_out);
NRF_API int nrf_comm_create(const void *id, int world, int rank, nrf_comm **out);
/* ... with a bounded rendezvous: the (ordinary, blocking) ncclCommInitRank runs on a helper thread bound to the caller's device and is waited for; after timeout_s
 * seconds without all `world` ranks NRF_ERR_HIP is returned (a peer that never started, or an id of another launch) and the caller should exit.  timeout_s <= 0 waits for
 * ever on the calling thread.  nrf_comm_create itself uses NRF_COMM_TIMEOUT_S from the environment (default 300; only a well-formed number is taken, 0 = wait for ever).
 * A non-blocking communicator handed over with nrf_comm_wrap is supported too: nrf_allgather_tiles waits (bounded) until its group has been enqueued before it returns. */
NRF_API int nrf_comm_create_timeout(const void *id, int world, int rank, double timeout_s, nrf_comm **out);
NRF_API int nrf_comm_wrap(void *nccl_comm, nrf_comm **out);
NRF_API void nrf_comm_destroy(nrf_comm *c);
NRF_API int nrf_comm_world(const nrf_comm *c);
NRF_API int nrf_comm_rank(const nrf_comm *c);
/* d_tiles: this rank's [frames, rows_rank, w, c] fp32 tiles of `frames` images (rows_rank from nrf_tile_partition; may be NULL on a rank that owns no rows, h < world);
 * d_frames: [frames, h, w, c] on every rank.  One fused launch on `stream` (ncclAllGather per frame when h % world == 0, grouped
 * ncclBroadcast per tile otherwise); asynchronous like every other call.  d_tiles and d_frames must not overlap. */
NRF_API int nrf_allgather_tiles(const nrf_comm *c, const float *d_tiles, int frames, int h, int w, int c_channels, float *d_frames, void *stream);
/* The data-parallel TRAINING step's exchange (no reference counterpart: the reference trains on one device, NeRFExecutor.h:862-995): the n_grads fp32
 * gradient buffers (hash table, network blob; counts[i] elements each) become their MEAN over the ranks, in place -- ncclAllReduce(sum) in slices of bucket_bytes
 * (0: 32 MiB) as one group launch, then a multiply by 1 / world, all on `stream`.  overflow >= 0 first makes the fp16 backward's per-rank overflow report collective
 * (all-reduce max of one word + one host read-back): *skip_out = 1 on every rank iff any rank passed a non-zero overflow, and no gradient is exchanged then (a peer's inf
 * is never summed in; every replica skips the same optimizer step).  overflow < 0: no agreement, nothing synchronises (skip_out may be NULL).  World of one: identity. */
NRF_API int nrf_allreduce_grads(const nrf_comm *c, float *const *d_grads, const int64_t *counts, int n_grads, int64_t bucket_bytes, int overflow, int *skip_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * LeRF render pass as library calls           LeRFRenderer (LeRFRenderer.h:56-132, LeRFRenderer.cpp:85-330)
 * ------------------------------------------------------------------------------------------- */
typedef struct nrf_lerf_renderer_desc {
    const nrf_hash *lang_embed;   /* LangEmbedFn: CuHashEmbedder L16 F8 (main.cpp:203-213) */
    const nrf_mlp *lerf;          /* Lerf: nrf_mlp_lerf_create; arithmetic of the fused passes: nrf_lerf_set_precision */
} nrf_lerf_renderer_desc;

typedef struct nrf_lerf_outputs {     /* LeRFRendererOutputs (LeRFRenderer.h:9-18); NULL = not wanted */
    float *d_embedding;        /* RenderedLangEmbedding [n, E] */
    float *d_disp;             /* DispMapLE [n] */
    float *d_acc;              /* AccMapLE [n] */
    float *d_depth;            /* DepthMapLE [n] */
    float *d_weights;          /* WeightsLE [n, n_samples + n_importance] */
    float *d_relevancy;        /* Relevancy [n, 2] (needs nrf_lerf_set_prompts) */
    /* intermediates for parity tests (optional) */
    float *d_z_coarse;         /* [n, n_samples] */
    float *d_weights_coarse;   /* [n, n_samples] */
    float *d_z_fine;           /* [n, n_samples + n_importance] */
} nrf_lerf_outputs;

typedef struct nrf_lerf_renderer nrf_lerf_renderer;
NRF_API int nrf_lerf_renderer_create(const nrf_lerf_renderer_desc *desc, nrf_lerf_renderer **out);
NRF_API void nrf_lerf_renderer_destroy(nrf_lerf_renderer *r);
/* The LeRF pass and nrf_render_params.overflow_policy: the compositing kernel of the fine pass looks at every sigma_le and the final normalise at every rendered embedding;
 * the pass has no fp32 single-call twin to render a flagged chunk again with, so AUTO / RERENDER / ERROR all end a call with one read-back and answer a non-finite value with
 * NRF_ERR_NONFINITE; DEFERRED reports at the next call (or here); IGNORE does not look.  flagged_calls: total since the renderer was created. */
NRF_API int nrf_lerf_renderer_nonfinite(const nrf_lerf_renderer *r, int64_t *flagged_calls);
/* Lanes of this renderer's Chunk loop, 1-4.  Default ONE: the LeRF kernels gain nothing from sharing the CUs (measured: 1 lane 140-143 ms per 800x800 frame, 2 lanes 146-147). */
NRF_API int nrf_lerf_renderer_set_lanes(nrf_lerf_renderer *r, int lanes);
/* LeRFRenderer::SetLeRFPrompts (LeRFRenderer.h:86): [n_pos, E] / [n_neg, E] fp32 phrase embeddings (host or device), copied; 0 / 0 clears them.  Synchronises `stream`. */
NRF_API int nrf_lerf_set_prompts(nrf_lerf_renderer *r, const float *positives, int n_pos, const float *negatives, int n_neg, int on_device, void *stream);

/* LeRFRenderer::RenderRays (LeRFRenderer.cpp:85-187) over one chunk of packed rays [n, 8 | 11], hierarchical (n_importance > 0), deterministic (ThinRay, Perturb = 0:
 * NRF_ERR_UNSUPPORTED otherwise), on the fused matrix-core path: every sample point is hash-encoded once and its density net evaluated once, raw_le [n, S, 769] is never
 * formed.  Of `p`: n_samples, n_importance (multiples of 32 in sum), lindisp, sum_vec, coarse_mode (NRF_COARSE_AUTO: sigma_le of the coarse pass in exact fp32 when the head
 * runs in NRF_PREC_F16_SPLIT, so that the fine sample set is the fp32 stage path's bit for bit; NRF_COARSE_FULL: the timed arithmetic).  d_t / d_u as nrf_render_rays. */
NRF_API size_t nrf_lerf_render_rays_workspace_bytes(const nrf_lerf_renderer *r, int64_t n, const nrf_render_params *p);
NRF_API int nrf_lerf_render_rays(const nrf_lerf_renderer *r, const float *d_rays, int ray_stride, int64_t n, const nrf_render_params *p, const float *d_t, const float *d_u,
                                 const nrf_lerf_outputs *out, void *d_workspace, size_t workspace_bytes, void *stream);
/* LeRFRenderer::BatchifyRays (LeRFRenderer.cpp:189-263): the Chunk loop inside the library, slices written in place, on the lanes of nrf_set_render_lanes /
 * nrf_lerf_renderer_set_lanes (one device and one caller at a time per renderer, as nrf_batchify_rays). */
NRF_API size_t nrf_lerf_batchify_rays_workspace_bytes(const nrf_lerf_renderer *r, int64_t n, int chunk, const nrf_render_params *p);
NRF_API int nrf_lerf_batchify_rays(const nrf_lerf_renderer *r, const float *d_rays, int ray_stride, int64_t n, int chunk, const nrf_render_params *p, const float *d_t,
                                   const float *d_u, const nrf_lerf_outputs *out, void *d_workspace, size_t workspace_bytes, void *stream);
/* LeRFRenderer::Render for a pose (LeRFRenderer.cpp:265-330), restricted to the row tile of `v`: rays + the Chunk loop + (with prompts) the relevancy in ONE call,
 * no synchronisation, no torch ops; out: buffers for the tile's rows*w rays; d_rays_out / d_near_far as nrf_render_rows. */
NRF_API size_t nrf_lerf_render_rows_workspace_bytes(const nrf_lerf_renderer *r, const nrf_view *v, const nrf_render_params *p);
NRF_API int nrf_lerf_render_rows(const nrf_lerf_renderer *r, const nrf_view *v, const nrf_render_params *p, const float *d_t, const float *d_u, const nrf_lerf_outputs *out,
                                 float *d_rays_out, float *d_near_far, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * LeRF relevancy in 3D (lerf_query.hip; no counterpart in the reference, which reads the language field through rendered images only)
 * ------------------------------------------------------------------------------------------- */
/* Per point x_i: d_relevancy[i] = Relevancy(normalize(le(x_i), eps 1e-8), positives[positive_id], negatives) -- the formula of nrf_lerf_relevancy: logits at temperature
 * 10, a pairwise softmax against each negative, the negative the positive does worst against (first on ties); n_neg = 0 gives (0, 0).  le = the head's 768-wide language
 * embedding (LeRFImpl::forward, LeRF.cpp:75-110).  The keep mask does not touch relevancy.  d_sigma [p] (NULL: not wanted) = sigma_le, equal in every precision to
 * nrf_mlp_forward(..., NRF_PREC_F32)[..., -1] bit for bit, with the keep mask (LeRFRenderer.cpp:17-18) in the point and grid entries.
 * precision:
 *   NRF_PREC_F32         the composed path: nrf_mlp_forward(F32) in chunks, normalise, relevancy.  Any LeRF head, any number of negatives.
 *   NRF_PREC_F16_SPLIT   one fused matrix-core kernel per slab from the sigma net's (sigma, geo32) output: LE0 -> a, ||W a||^2 = a^T (W^T W) a (the render pass's Gram
 *   NRF_PREC_F16_MFMA    layer), q . W a = (W^T q) . a for the 1 + n_neg prompts (U = W^T q built in fp64 into the workspace on every call), the relevancy in
 *                        registers; no 768-wide value exists.  SPLIT carries LE0 and the U tile as hi + lo fp16 pairs, MFMA as plain fp16.  The head must have
 *                        the matrix-core shape (in 128 / hidden 256 / 2+2 layers / geo 32 / embedding 768) and 1 + n_neg <= 32: NRF_ERR_UNSUPPORTED otherwise.
 * Results do not depend on p or slab_points, bit for bit; a lattice point gets the same bits from the grid entry as from the point entry.  Only the caller's workspace is
 * used; nothing the renderer owns is written (the feature view of nrf_lerf_renderer_last_features stays valid); prompts and weights are read anew on every call.
 * Errors: no prompts set, positive_id out of range, NULL d_relevancy: NRF_ERR_INVALID_ARG; workspace too small: NRF_ERR_WORKSPACE; p == 0: NRF_OK, nothing launched.
 * Non-finite network values are not detected (no overflow policy here): they reach the outputs. */
/* The head alone on fp32 feature rows d_x [p, 128] (16-byte aligned), explicit device prompts [n_pos, 768] / [n_neg, 768] as nrf_lerf_relevancy takes them.  In the fused
 * precisions the rows are split hi / lo for LE0 and sigma_le (when wanted) comes from the F32 network: rows are not fp16 numbers in general. */
NRF_API size_t nrf_lerf_head_relevancy_workspace_bytes(const nrf_mlp *m, int64_t p, int n_neg, int precision);
NRF_API int nrf_lerf_head_relevancy(const nrf_mlp *m, const float *d_x, int64_t p, const float *d_positives, int n_pos, const float *d_negatives, int n_neg,
                                    int positive_id, int precision, float *d_sigma, float *d_relevancy, void *d_ws, size_t ws_bytes, void *stream);
/* Points d_pts [p, 3] through the renderer's language grid and head, prompts from nrf_lerf_set_prompts.  Fused precisions: the level-major fp16 encode, sigma_le and the
 * geo planes from the exact-fp32 density pass (sigma_lerf_f32.hip), the fused kernel; slabs of slab_points points (<= 0: 2^22; at most 2^30) bound the workspace. */
NRF_API size_t nrf_lerf_point_relevancy_workspace_bytes(const nrf_lerf_renderer *r, int64_t p, int precision, int64_t slab_points);
NRF_API int nrf_lerf_point_relevancy(const nrf_lerf_renderer *r, const float *d_pts, int64_t p, int positive_id, int precision, float *d_sigma, float *d_relevancy,
                                     int64_t slab_points, void *d_ws, size_t ws_bytes, void *stream);
/* The lattice of nrf_density_grid (bbox[6] on the host, P = bmin + (float)i * step, x fastest): d_relevancy [nz][ny][nx][2], d_sigma [nz][ny][nx], in slabs as above. */
NRF_API size_t nrf_lerf_relevancy_grid_workspace_bytes(const nrf_lerf_renderer *r, int nx, int ny, int nz, int precision, int64_t slab_points);
NRF_API int nrf_lerf_relevancy_grid(const nrf_lerf_renderer *r, const float *bbox, int nx, int ny, int nz, int positive_id, int precision, float *d_sigma,
                                    float *d_relevancy, int64_t slab_points, void *d_ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * N1, LeRF branch of the optimisation step (NeRFExecutor.h:955-982): lang_loss and its backward into LeRFImpl and the language grid
 * ------------------------------------------------------------------------------------------- */
/* lang_loss = huber_loss(pred, target, reduction none, delta).sum(-1).nanmean() (NeRFExecutor.h:970-974; delta 1.25 there): d_loss [1]; d_grad [n, e] = d loss / d pred
 * (NULL: not wanted).  A row holding a NaN leaves the mean (count = the other rows); its gradient row is 0 except NaN at the NaN elements -- what LibTorch's backward
 * leaves there (golden train_lerf_nan).  With EVERY row NaN the loss is NaN and so is the whole gradient (1 / 0 rows times 0), as LibTorch's. */
NRF_API int nrf_huber_rows_nanmean(const float *d_pred, const float *d_target, int64_t n, int e, float delta, float *d_loss, float *d_grad, void *stream);
/* Backward of the FINE pass of LeRFRenderer::RenderRays (LeRFRenderer.cpp:141-172; the coarse pass carries none: z_samples are detached, :150) downstream of the language
 * grid: d_emb [n*s, in] = lang_embed_fn->forward(pts) -> LeRFImpl::forward (LeRF.cpp:86-108) -> sigma_le[~keep] = 0 (LeRFRenderer.cpp:37-38) -> RawToLEOutputs' weights
 * (:38-66; d_noise [n, s] / noise_std: the RawNoiseStd draws, NULL / 0 = none) -> RenderCLIPEmbedding (LeRFRenderer.h:45-54), given d_g_rendered [n, E] = d loss /
 * d RenderedLangEmbedding.  fp32; the forward is recomputed here (every layer input kept, chunks of whole rays).  d_g_params: the head's blob layout, ACCUMULATED into;
 * d_g_emb [n*s, in] written (NULL: not wanted); d_rendered [n, E] / d_weights [n, s]: the recomputed forward (NULL: not wanted).  d_dirs: rays_d, row stride d_stride. */
NRF_API size_t nrf_lerf_head_backward_workspace_bytes(const nrf_mlp *lerf, int64_t n, int s);
NRF_API int nrf_lerf_head_backward(const nrf_mlp *lerf, const float *d_emb, const uint8_t *d_keep, const float *d_z, const float *d_dirs, int d_stride, int64_t n, int s,
                                   const float *d_noise, float noise_std, const float *d_g_rendered, float *d_g_params, float *d_g_emb, float *d_rendered, float *d_weights,
                                   void *d_workspace, size_t workspace_bytes, void *stream);
/* ... with the language grid in front -- the backward of one LeRFRenderer::Render call on a ray batch in ONE library call: d_pts [n, s, 3] the fine pass's sample points
 * (o + d z, after TangentScatter / preconditioning where those are on) -> nrf_hash_encode -> the head's backward -> nrf_hash_backward_rays (CuHashEmbedderBackwardKernel's
 * gradient, CuHashEmbedder.cu:105-216).  d_g_lerf_params (head blob) and d_g_table (the grid's fp32 table layout) are ACCUMULATED into. */
NRF_API size_t nrf_lerf_backward_points_workspace_bytes(const nrf_lerf_renderer *r, int64_t n, int s);
NRF_API int nrf_lerf_backward_points(const nrf_lerf_renderer *r, const float *d_pts, const float *d_z, const float *d_dirs, int d_stride, int64_t n, int s, const float *d_noise,
                                     float noise_std, const float *d_g_rendered, float *d_g_lerf_params, float *d_g_table, void *d_workspace, size_t workspace_bytes, void *stream);
/* Where the most recent render call on this LeRF renderer left the language features of its fine depths (as nrf_renderer_last_features; a call that rendered exactly ONE
 * chunk): the level-major fp16 table [16][cols][8] (coarse columns first, the new samples' behind them), the keep mask by column, the merge map [n, sf].  They live in the
 * caller's workspace: valid until the next render call on this renderer or any other use of that workspace.  NRF_ERR_UNSUPPORTED when the last call left none (serial is set
 * either way).  nrf_lerf_backward_points_src: nrf_lerf_backward_points whose head backward reads those rows through the map instead of encoding d_pts again (the points must be
 * the ones that render encoded: thin rays, no preconditioning); d_pts still feeds the grid's gradient scatter. */
NRF_API int nrf_lerf_renderer_last_features(const nrf_lerf_renderer *r, const void **d_feats_lm, int64_t *cols, const uint8_t **d_keep_cols, const int32_t **d_src, int64_t *n, int *sf,
                                            uint64_t *serial /* optional */);
NRF_API int nrf_lerf_backward_points_src(const nrf_lerf_renderer *r, const void *d_feats_lm, int64_t cols, const uint8_t *d_keep_cols, const int32_t *d_src, const float *d_pts,
                                         const float *d_z, const float *d_dirs, int d_stride, int64_t n, int s, const float *d_noise, float noise_std, const float *d_g_rendered,
                                         float *d_g_lerf_params, float *d_g_table, void *d_workspace, size_t workspace_bytes, void *stream);

/* The library's short-lived device buffers (a layer product's split operand image, slice sums, reduction cells) come from blocks it keeps per (device, stream) and reuses
 * from call to call -- not from hipMallocAsync, whose pool proved unsafe inside a LibTorch host (scratch.hip).  nrf_scratch_trim gives the idle blocks back to the driver
 * (after a hipDeviceSynchronize of their devices) and returns the bytes freed; optional. */
NRF_API size_t nrf_scratch_trim(void);
/* Bytes of device memory the library holds right now: everything its handles own plus its scratch blocks, idle ones included.  Pinned host memory is not counted.
 * One counter for the process (all devices); every device allocation of the library goes through it. */
NRF_API int64_t nrf_device_bytes_in_use(void);

/* ---------------------------------------------------------------------------------------------
 * Instrumentation (bench / tests)
 * ------------------------------------------------------------------------------------------- */
/* When enabled, nrf_render_rays brackets its dominant kernels with HIP events on the caller's stream;
 * nrf_profile_read synchronises them and returns accumulated milliseconds and launch counts. */
/* NRF_PROF_MLP_COLOUR: the NeRFSmall kernel's colour-net-only launch of a hierarchical render's fine pass (its S coarse depths; see nrf_render_params.coarse_mode) --
 * a different amount of work per point than NRF_PROF_MLP's whole-network launches, so it has its own slot. */
enum { NRF_PROF_HASH = 0, NRF_PROF_MLP = 1, NRF_PROF_COMPOSITE = 2, NRF_PROF_SAMPLE = 3, NRF_PROF_OTHER = 4, NRF_PROF_SIGMA = 5, NRF_PROF_MLP_COLOUR = 6, NRF_PROF_COUNT = 7 };
/* The Chunk loop of nrf_batchify_rays / nrf_render_rows runs consecutive chunks on `lanes` internal streams (default 2, at most 4; forked from and joined to the
 * caller's stream) so that one chunk's gather-bound kernels overlap another's matrix-bound ones; results do not depend on it.  lanes = 1 restores the single-stream
 * loop (also: NRF_RENDER_LANES=1..4).  Process-wide setting, read at every call; the workspace query and the call must see the same value. */
NRF_API int nrf_set_render_lanes(int lanes);
NRF_API int nrf_get_render_lanes(void);
/* The fine pass of the default hierarchical HashNeRF render (NRF_PREC_F16_SPLIT with the exact coarse pass) evaluates the colour net at a coarse depth only where that
 * depth's density is positive: relu(sigma) = 0 gives alpha = 0 and a weight of exactly 0, so the colour there cannot change a bit of RGB, depth, disparity, acc or the
 * weights.  Renders that return Raw or add sigma noise evaluate every colour whatever the switch says.  on = 1 (the default; also NRF_LIVE_COLOUR=0 in the environment
 * turns it off) / 0: the colour net at every coarse depth.  Process-wide, read at every call; workspace sizes do not depend on it. */
NRF_API int nrf_set_live_colour(int on);
NRF_API int nrf_get_live_colour(void);
/* The compaction behind it, on its own: d_list [p] int32 receives the indices i with d_sigma[i] > 0.0f in ascending order (NaN, +-0 and negatives are not listed; entries
 * from *d_count on are left as they were), d_count [1] int32 their number, and -- unless NULL -- d_raw_rows [p, 4] (16-byte aligned) the row (0, 0, 0, d_sigma[i]) of
 * every index that is NOT listed, the sigma word copied bit for bit; rows of listed indices are not written.  1 <= p < 2^31.  Deterministic, no atomics, no host
 * synchronisation. */
NRF_API size_t nrf_live_points_workspace_bytes(int64_t p);
NRF_API int nrf_live_points(const float *d_sigma, int64_t p, int32_t *d_list, int32_t *d_count, float *d_raw_rows, void *d_workspace, size_t workspace_bytes, void *stream);
/* The default hierarchical HashNeRF render (the path of nrf_set_live_colour, sigma noise off, at most 256 + 256 samples) turns a chunk's exact coarse sigma into the fine
 * depths in ONE kernel -- coarse weights, SamplePDF, the stable merge and the per-ray masks of sigma > 0 from which the live list is made -- instead of one launch per
 * stage.  The same device functions in the same order: every output is bit for bit what the stage-wise chain gives.  on = 1 (the default; NRF_FUSED_RESAMPLE=0 in the
 * environment turns it off) / 0: one launch per stage.  Process-wide, read at every call; workspace sizes do not depend on it. */
NRF_API int nrf_set_fused_resample(int on);
NRF_API int nrf_get_fused_resample(void);
/* Debug entry, for tests: that kernel pair on its own.  d_sigma [n, s] -> d_z_fine [n, s + ns], d_src [n, s + ns], d_z_new [n, ns] as nrf_raw2weights (c = 1) followed by
 * nrf_fine_depths_merge give them; d_u: the shared table [ns] (u_stride 0), per-ray rows (u_stride ns) or NULL (draws generated from seed / ray_base as the renderer's
 * Perturb > 0 does); d_weights [n, s] or NULL: the coarse weights.  With d_counts (16-byte aligned, 4 ceil(n / 4) + ceil(n / 64) int32: every ray's number of
 * sigma > 0, then the list offsets of the groups of 64 rays) also d_list, d_count and d_raw_rows [n * s, 4] exactly as nrf_live_points writes them.  2 <= s <= 256, 1 <= ns <= 256, n (s + ns) < 2^31. */
NRF_API int nrf_dbg_resample(const float *d_sigma, const float *d_z, const float *d_dirs, int d_stride, int64_t n, int s, const float *d_u, int64_t u_stride, uint64_t seed,
                             int64_t ray_base, int ns, int sum_vec, float *d_z_fine, int32_t *d_src, float *d_z_new, float *d_weights, int32_t *d_counts, int32_t *d_list,
                             int32_t *d_count, float *d_raw_rows, void *stream);
/* ... per renderer: 1-4 lanes for this renderer's calls whatever the process-wide setting; 0 returns it to that setting (two renderers of one process need not share it). */
NRF_API int nrf_renderer_set_lanes(nrf_renderer *r, int lanes);
/* 1 when the fp32 layer products of the training paths (classic and LeRF backward, NeRFSmall's fp32 backward) run as rocBLAS GEMMs on the fp32 matrix cores (the library is
 * looked up with dlopen at first use, preferring the copy the process already maps), 0 when they run the hand-written FMA kernels (rocBLAS absent, or NRF_FP32_GEMM=0). */
NRF_API int nrf_fp32_gemm_available(void);
/* Arithmetic of the forward / back-propagation products of the classic-NeRF and LeRF training steps (gemm_bf16x3.hip; NRF_TRAIN_GEMM=auto | f32 | bf16x3 | f16x3 in the
 * environment selects the process-wide default):
 *  -1  (default, "auto") by network family: 2 for the classic NeRF and the LeRF head, 0 for NeRFSmall's fp32 backward (the hash path's parity chain; its fast chain is
 *      the fused fp16 backward, nrf_mlp_backward_f16).
 *   0  fp32 products (rocBLAS sgemm where present, else the FMA kernels).
 *   1  bf16x3: every operand as hi + lo bf16 (fp32's exponent range, 16 significant bits), three matrix-core products per fp32 accumulator, bias / ReLU / ReLU mask
 *      fused in the epilogue.  One product within 6e-6 of its largest entry; a whole chain's weight gradients within ~1e-3 of the fp32 chain's.
 *   2  f16x3: hi + lo fp16 (22 significant bits) of power-of-two scaled operands -- each row of A by its own largest entry, B by its largest entry, undone exactly in
 *      the epilogue; one product is closer to the float64 product than sgemm's (5e-7 against 8e-7 of the largest entry at K = 256), a classic step's weight gradients
 *      end 6e-5 (norm-wise) from the rocBLAS chain's -- rocBLAS and the FMA kernels are 2e-5 apart (ReLUs decided the other way by last-bit differences). */
NRF_API int nrf_get_train_gemm(void);
NRF_API int nrf_set_train_gemm(int mode);
/* The products themselves: C [m x n] (ldc) = A [m x k] (lda) . B [n x k]^T (ldb) (+ bias [n]) (ReLU), fp32 row-major in and out */
NRF_API int nrf_gemm_nt_bf16x3(const float *d_a, int lda, int64_t m, int k, const float *d_b, int ldb, int n, float *d_c, int ldc, const float *d_bias, int relu, void *stream);
/* dW [out x in] (ld in; columns col0 .. col0 + n) += G [p x out]^T (ldg) . X [p x n] (ldx), fp32 row-major: the weight-gradient product of a layer over p points
 * (bf16x3 arithmetic -- a per-point scale cannot be undone in a sum over points; deterministic: slices of the points summed in a fixed order) */
NRF_API int nrf_gemm_tn_bf16x3(const float *d_g, int ldg, int out, const float *d_x, int ldx, int n, int64_t p, float *d_dw, int in, int col0, void *stream);
/* One layer's weight gradient as the split-precision training modes compute it, with its bias gradient: dW += G^T X as above (out >= 32) or, for a head of fewer rows,
 * by fp32 FMAs four rows per pass over X; d_db (optional) [out] += the column sums of G, out of the same pass over G where out >= 32 */
NRF_API int nrf_layer_grad_split(const float *d_g, int ldg, int out, const float *d_x, int ldx, int n, int64_t p, float *d_dw, int in, int col0, float *d_db, void *stream);
NRF_API int nrf_gemm_nt_f16x3(const float *d_a, int lda, int64_t m, int k, const float *d_b, int ldb, int n, float *d_c, int ldc, const float *d_bias, int relu, void *stream);
NRF_API int nrf_profile_enable(int on);
/* 1 while the event bracketing is on.  A throughput measurement must run with it off: an event pair around every kernel of every lane costs host time per launch and
 * separates the kernels on the device (bench.py asserts 0 before its timed region; the per-kernel times come from a separate pass).  Events are pooled: none is created on
 * a launch path after the first profiled frame. */
NRF_API int nrf_profile_is_enabled(void);
NRF_API int nrf_profile_read(double *ms /*[NRF_PROF_COUNT]*/, int64_t *launches /*[NRF_PROF_COUNT]*/, int reset);

#ifdef __cplusplus
}
#endif
#endif /* NERFPP_HIP_H */
