"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C ABI, against
  (a) the committed golden vectors of the reference's LibTorch CPU path (tests/golden), and
  (b) the C oracle on the same seeded inputs.
Bars: bit-exact for indices / integer outputs and for every stage made of + - * / floor / compare;
float tolerance stated per test otherwise (pixels: 1e-4, BASELINE north_star)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from split_fine_pass_check import check_default_split_fine_pass
from nerfpp_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from nerfpp_amd import _lib, modules, renderer, scene
    _lib.lib()          # fail loudly if libnerfpp_hip.so is missing
    return type("Api", (), dict(L=_lib, M=modules, R=renderer, S=scene))


@pytest.fixture(scope="module")
def O():
    from oracle import capi
    return capi


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def assert_exact(a, b, what=""):
    a = np.asarray(a).reshape(-1); b = np.asarray(b).reshape(-1)
    assert a.size == b.size, (what, a.size, b.size)
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} differ, first at {bad[:5]}: {a[bad[:3]]} vs {b[bad[:3]]}"


def assert_close(a, b, rtol, atol, what=""):
    np.testing.assert_allclose(np.asarray(a).reshape(-1), np.asarray(b).reshape(-1), rtol=rtol, atol=atol, err_msg=what)


# ------------------------------------------------------------------------------------------- rays
def test_get_rays_bit_exact(api):
    g = load_golden("rays")
    h, w = (int(v) for v in g["hw"])
    o, d, cone = api.R.GetRays(h, w, g["k"], g["c2w"])
    assert_exact(host(o), g["o"], "rays_o"); assert_exact(host(d), g["d"], "rays_d"); assert_exact(cone.numpy(), g["cone"], "cone")
    ot, dt, _ = api.R.GetRays(h, w, g["k"], g["c2w"], row0=2, rows=3)           # row tile == slice of the image
    assert_exact(host(ot), g["o"][2:5]); assert_exact(host(dt), g["d"][2:5])


def test_ndc_rays_bit_exact(api):
    g = load_golden("rays")
    h, w = (int(v) for v in g["hw"])
    oo, od, _ = api.R.NDCRays(h, w, float(g["k"][0, 0]), 1.0, dev(g["o"]), dev(g["d"]))
    assert_exact(host(oo), g["ndc_o"]); assert_exact(host(od), g["ndc_d"])


def test_aabb_bit_exact(api):
    g = load_golden("aabb")
    nr, fr = api.R.IntersectWithAABB(dev(g["o"]), dev(g["d"]), g["bbox"])
    assert_exact(host(nr), g["near"]); assert_exact(host(fr), g["far"])


def test_linspace_helper_matches_aten(api):
    import ctypes as C
    g = load_golden("sample_pdf")
    for n, key in ((64, "aux_t64"), (128, "aux_u_128"), (192, "aux_t192"), (5, "aux_u_5")):
        out = np.empty(n, np.float32)
        api.L.check(api.L.lib().nrf_linspace(C.c_float(0), C.c_float(1), n, out.ctypes.data_as(C.c_void_p)))
        assert_exact(out, g[key], f"linspace {n}")
        assert_exact(torch.linspace(0, 1, n).numpy(), g[key], "torch.linspace on this host")


# --------------------------------------------------------------------------------------- encoders
@pytest.mark.parametrize("nf", [10, 4, 2])
def test_pe(api, nf):
    g = load_golden("pe")
    out, mask = api.M.Embedder("pe", nf).forward(dev(g["x"]))
    assert mask is None
    out = host(out)
    assert_exact(out[:, :3], g[f"out_{nf}"][:, :3])
    assert_close(out, g[f"out_{nf}"], rtol=0, atol=5e-7, what="sin/cos: nrf_math vs SLEEF, arguments up to 2^9*1.5")
    from oracle import capi as O
    assert_exact(out, O.pe(g["x"], nf), "PE == oracle bit for bit (shared portable sin/cos)")


@pytest.mark.parametrize("deg", [1, 2, 3, 4, 5])
def test_sh_libtorch_bit_exact(api, deg):
    g = load_golden("sh")
    out, _ = api.M.SHEncoder("sh", 3, deg).forward(dev(g["dirs"]))
    assert_exact(host(out), g[f"out_{deg}"])


@pytest.mark.parametrize("deg", [1, 2, 3, 4, 5, 6, 7, 8])
def test_sh_cuda_variant_bit_exact_vs_oracle(api, O, deg):
    g = load_golden("sh")
    out, _ = api.M.CuSHEncoder("sh", 3, deg).forward(dev(g["dirs"]))
    assert_exact(host(out), O.sh_cu(g["dirs"], deg))


@pytest.mark.parametrize("tag", ["hash_small", "hash_f4", "hash_f8", "hash_full", "hash_full1024"])
def test_hash_ngp_bit_exact_vs_reference(api, tag, manifest):
    g = load_golden(tag)
    Lv, F, T, base, fine = (int(v) for v in g["cfg"])
    e = api.M.HashEmbedder("embedder", g["bbox"], Lv, F, T, base, fine)
    e.set_table(synth.blob_from_manifest(manifest[tag]))
    emb, mask = e.forward(dev(g["x"]))
    assert_exact(host(mask), g["mask"], "keep_mask"); assert_exact(host(emb), g["emb"], "embedding")


@pytest.mark.parametrize("cfg", [(16, 2, 19, 16, 512), (16, 2, 19, 16, 1024), (4, 2, 10, 4, 32), (16, 8, 12, 16, 128), (3, 4, 8, 2, 20)])
def test_hash_cu_bit_exact_vs_oracle(api, O, cfg):
    Lv, F, T, base, fine = cfg
    bbox = api.S.LEGO_BBOX
    e = api.M.CuHashEmbedder("embedder", bbox, Lv, F, T, base, fine)
    table = synth.synth_sym(77, (Lv * (1 << T) * F,), np.float32(0.5))
    primes = np.array(api.S.CU_PRIMES[:3 * Lv], np.int32)
    e.set_table(table); e.set_primes(primes)
    x = synth.synth_sym(78, (4096, 3), np.float32(1.6))
    x[0] = [1.5, 1.5, 1.5]; x[1] = [-1.5, -1.5, -1.5]; x[2] = 0.0; x[3] = [2.0, 0.1, 0.2]
    emb, mask = e.forward(dev(x))
    ls = ((1 << T) >> 4) << 4
    ref, rmask = O.hash_cu(x, O.f32_to_f16(table), primes, np.arange(Lv, dtype=np.int32) * ls, np.full(Lv, ls, np.int32), np.zeros((Lv, 3), np.float32),
                           bbox, O.hash_cu_scales(Lv, base, fine), Lv, F)
    assert_exact(host(mask), rmask, "keep_mask"); assert_exact(host(emb), ref, "embedding (fp16-rounded)")
    assert (~rmask).sum() > 0


@pytest.mark.parametrize("tag", ["hash_small", "hash_f8"])
def test_cu_hash_kernel_reproduces_the_reference_pinned_hash_embedder_level_by_level(api, tag, manifest):
    """GPU twin of tests/test_oracle_golden.py::test_cu_hash_restatement_reproduces_...: the HIP CuHashEmbedder path (nrf_hash_encode, NRF_HASH_CU) with the level scales
    set to HashEmbedder's integer resolutions (nrf_hash_set_level_scales), primes (1, 2654435761, 805459861) and H1's level-l table placed where level l's view starts
    (ELEMENT l * local_size: the overlap quirk forbids loading all levels at once) must reproduce the REFERENCE's golden embedding of level l up to H2's two fp16
    roundings -- hash, corner order and trilinear weights of CuHashEmbedder.cu:66-100 against NeRF.cpp:230-298."""
    from test_oracle_golden import cu_level_vs_ngp_golden, NGP_PRIMES_AS_INT32
    g = load_golden(tag)
    L, F, T, base, fine = (int(v) for v in g["cfg"])
    e = api.M.CuHashEmbedder("embedder", g["bbox"], L, F, T, base, fine)
    e.set_primes(np.tile(NGP_PRIMES_AS_INT32, L))
    from oracle import capi as O
    e.set_level_scales(O.hash_ngp_resolutions(L, base, fine))
    ls = ((1 << T) >> 4) << 4
    assert ls == 1 << T

    def encode_level(l, table_l, res_l, T_, F_, x):
        full = np.zeros(L * (1 << T) * F, np.float32)
        full[l * ls:l * ls + table_l.size] = table_l.reshape(-1)
        e.set_table(full)
        emb, _ = e.forward(dev(x))
        return host(emb)[:, l * F:(l + 1) * F]
    assert cu_level_vs_ngp_golden(tag, manifest, encode_level) <= 1.0


@pytest.mark.parametrize("deg", [6, 7, 8])
def test_sh_cuda_variant_vs_an_independent_float64_recurrence(api, deg):
    """GPU twin of the S1 anchor at the degrees the LibTorch twin does not reach: CuSHEncoder's HIP kernel against real spherical harmonics from the Legendre recurrence in
    float64 (tests/test_oracle_golden.py::real_sh_f64) on unit vectors."""
    from test_oracle_golden import real_sh_f64
    g = load_golden("sh")
    d = g["dirs"].astype(np.float64)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    out, _ = api.M.CuSHEncoder("sh", 3, deg).forward(dev(d))
    assert_close(host(out), real_sh_f64(d, deg), rtol=0, atol=1.5e-6 if deg <= 7 else 3e-6, what=f"CuSHEncoder kernel, degree {deg}")


def test_hash_cu_known_answers(api):
    """Restatement pin for the CUDA-only unit: hand-computable cases.
    table[i] = i as fp16 over ONE level pair so that corner hits return table rows and the level-offset quirk
    (level l starts l*2^T ELEMENTS in, rows are F wide: CuHashEmbedder.cu:54 vs :96) is visible."""
    Lv, F, T = 2, 2, 4
    bbox = np.array([0, 0, 0, 1, 1, 1], np.float32)
    e = api.M.CuHashEmbedder("e", bbox, Lv, F, T, 2, 4)          # mul_0 = 2, mul_1 = 4 exactly
    table = np.arange(Lv * 16 * F, dtype=np.float32)
    e.set_table(table); e.set_primes(np.array([1, 1, 1, 1, 1, 1], np.int32))
    # x = 0 -> pos = 0, weights (1,0,..): hash(0,0,0) = 0 -> row 0 of each level's view
    emb, _ = e.forward(dev(np.zeros((1, 3), np.float32)))
    emb = host(emb)[0]
    assert emb[0] == 0.0 and emb[1] == 1.0                       # level 0: elements 0,1
    assert emb[2] == 16.0 and emb[3] == 17.0                     # level 1 starts at ELEMENT 16 (not 32): the overlap quirk
    # x = (0.5,0,0): level 0 pos = (1,0,0), a = 0 -> hash = 1 -> elements 2,3
    emb, _ = e.forward(dev(np.array([[0.5, 0, 0]], np.float32)))
    assert host(emb)[0, 0] == 2.0 and host(emb)[0, 1] == 3.0
    # partition of unity: constant table -> constant output
    e.set_table(np.full(Lv * 16 * F, 0.25, np.float32))
    emb, _ = e.forward(dev(synth.synth_sym(5, (64, 3), np.float32(0.5), 0.5)))
    assert_close(host(emb), 0.25 * np.ones((64, Lv * F)), rtol=0, atol=2e-4, what="fp16 rounding of a sum of 8 weights * 0.25")


# ------------------------------------------------------------------------------------------- MLPs
SMALL = [("mlp_small_c4", dict(in_ch=32, in_views=16, n_layers_c=4)), ("mlp_small_c3", dict(in_ch=32, in_views=16, n_layers_c=3)),
         ("mlp_small_v64", dict(in_ch=32, in_views=64, n_layers_c=3))]


@pytest.mark.parametrize("tag,kw", SMALL)
def test_mlp_small_f32_bit_exact_vs_oracle(api, O, tag, kw, manifest):
    g = load_golden(tag)
    blob = synth.blob_from_manifest(manifest[tag])
    m = api.M.NeRFSmall(3, 64, 15, kw["n_layers_c"], 64, False, 3, 64, kw["in_ch"], kw["in_views"], "model", params=blob)
    y = host(m.forward(dev(g["x"]), api.L.NRF_PREC_F32))
    assert_exact(y, O.mlp_small(blob, g["x"], **kw), "fp32 FMA chain == oracle")
    assert_close(y, g["y"], rtol=1e-4, atol=1e-5, what="vs reference (MKL sgemm order)")


@pytest.mark.parametrize("tag,kw", SMALL)
def test_mlp_small_f16_mfma(api, tag, kw, manifest):
    g = load_golden(tag)
    blob = synth.blob_from_manifest(manifest[tag])
    m = api.M.NeRFSmall(3, 64, 15, kw["n_layers_c"], 64, False, 3, 64, kw["in_ch"], kw["in_views"], "model", params=blob)
    x = np.tile(g["x"], (5, 1))[:333]                  # ragged count: exercises the tail guard of the 256-point blocks
    y = host(m.forward(dev(x), api.L.NRF_PREC_F16_MFMA))
    ref = np.tile(g["y"], (5, 1))[:333]
    # fp16 operands (11-bit significand), fp32 accumulate, 7 layers: ~1e-3 of the activation scale
    scale = np.abs(ref).max()
    assert_close(y, ref, rtol=0, atol=4e-3 * scale, what="fp16 MFMA vs reference")
    assert np.abs(y - ref).mean() < 6e-4 * scale


def test_mlp_nerf_f32_bit_exact_vs_oracle(api, O, manifest):
    g = load_golden("mlp_nerf")
    blob = synth.blob_from_manifest(manifest["mlp_nerf"])
    m = api.M.NeRF(8, 256, 63, 27, 5, (4,), True, "model", params=blob)
    y = host(m.forward(dev(g["x"])))
    assert_exact(y, O.mlp_nerf(blob, g["x"], out_ch=5))
    assert_close(y, g["y"], rtol=1e-4, atol=1e-5)
    g = load_golden("mlp_nerf_noview")
    blob = synth.blob_from_manifest(manifest["mlp_nerf_noview"])
    m = api.M.NeRF(8, 256, 63, 0, 4, (4,), False, "model", params=blob)
    y = host(m.forward(dev(g["x"])))
    assert_exact(y, O.mlp_nerf(blob, g["x"], in_views=0, out_ch=4, use_viewdirs=False))
    assert_close(y, g["y"], rtol=1e-4, atol=1e-5)


def test_lerf_head_f32(api, O, manifest):
    g = load_golden("lerf")
    blob = synth.blob_from_manifest(manifest["lerf"])
    m = api.M.LeRF(32, 2, 256, 768, 128, "lang_model", params=blob)
    y = host(m.forward(dev(g["x"])))
    assert_close(y, O.lerf(blob, g["x"]), rtol=2e-6, atol=1e-8, what="vs oracle (norm in double on both)")
    assert_close(y, g["y"], rtol=1e-3, atol=2e-7, what="vs reference")


# ------------------------------------------------------------------------------------ compositing
@pytest.mark.parametrize("S", [64, 192])
@pytest.mark.parametrize("bg", ["black", "white"])
def test_raw2outputs(api, O, S, bg):
    g = load_golden(f"raw2out_{S}")
    e = api.M.Embedder("e", 2)
    m = api.M.NeRF(2, 8, 15, 15, 4, (), True, "model", params=np.zeros(api.M.NeRF(2, 8, 15, 15, 4, (), True).n_params, np.float32))
    r = api.R.NeRFRenderer(e, api.M.Embedder("ed", 2), m)
    o = r.RawToOutputs(dev(g["raw"]), None, dev(g["z"]), dev(g["d"]), 0.0, bg == "white")
    ref = O.raw2outputs(g["raw"], g["z"], g["d"], bg == "white")
    for k, v in (("rgb", o.RGBMap), ("disp", o.DispMap), ("acc", o.AccMap), ("weights", o.Weights), ("depth", o.DepthMap)):
        assert_close(host(v), g[f"{bg}_{k}"], rtol=4e-6, atol=4e-7, what=f"{k} vs reference")
        assert_exact(host(v), ref[k], f"{k} == oracle bit for bit (double scans/sums + shared exp/log)")


# ---------------------------------------------------------------------------------------- sampler
@pytest.mark.parametrize("ns", [128, 192, 5])
def test_sample_pdf_indices_bit_exact_vs_reference(api, ns):
    g = load_golden("sample_pdf")
    s, inds = api.R.SamplePDF(dev(g["bins"]), dev(g["weights"]), ns, True, return_inds=True)
    assert_exact(host(inds), g[f"aux_inds_{ns}"], "searchsorted indices")
    assert_exact(host(s), g[f"samples_{ns}"], "samples")


@pytest.mark.parametrize("tag", ["render_hash", "render_classic", "render_hash_lindisp"])
def test_fine_depths_bit_exact_from_reference_coarse_pass(api, tag):
    """Stage-chained: the reference's own coarse z / weights in, the reference's fine z (sorted, sample indices implied) out."""
    import ctypes as C
    g = load_golden(tag)
    z = dev(g["coarse_z"]); w = dev(g["coarse_weights"])
    n = z.shape[0]
    u = torch.linspace(0, 1, 128).cuda()
    zf = torch.empty((n, 192), device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    api.L.check(api.L.lib().nrf_fine_depths(P(z), P(w), C.c_int64(n), 64, P(u), 128, 8, P(zf), None))
    torch.cuda.synchronize()
    assert_exact(host(zf), g["fine_z"], "sort(cat(z, SamplePDF(...)))")


def test_fine_depths_fallback_sort_on_unsorted_input(api, O):
    """A non-monotone z row must still come out sorted (exhaustive-rank path)."""
    import ctypes as C
    rng = np.random.RandomState(3)
    z = np.sort(rng.rand(8, 64).astype(np.float32) * 4 + 2, axis=1)
    z[3, 10], z[3, 11] = z[3, 11], z[3, 10]
    w = rng.rand(8, 64).astype(np.float32)
    zf = torch.empty((8, 192), device="cuda")
    u = torch.linspace(0, 1, 128).cuda()
    P = lambda t: C.c_void_p(t.data_ptr())
    zd, wd = dev(z), dev(w)
    api.L.check(api.L.lib().nrf_fine_depths(P(zd), P(wd), C.c_int64(8), 64, P(u), 128, 8, P(zf), None))
    out = host(zf)
    assert (np.diff(out, axis=1) >= 0).all()
    samples, _, _ = O.sample_pdf(O.z_mid(z), w[:, 1:-1], O.linspace(0, 1, 128))
    assert_exact(out, O.merge_sorted(z, samples))


# ------------------------------------------------------------------------------------- end to end
def _golden_hash_scene(api, manifest, mode_cls=None):
    ent = manifest["render_hash"]
    bbox = load_golden("render_hash")["bbox"]
    e = api.M.HashEmbedder("embedder", bbox, 16, 2, 19, 16, 512)
    e.set_table(synth.blob_from_manifest([x for x in ent if "embeddings" in x[0]]))
    blob = synth.blob_from_manifest([x for x in ent if "embeddings" not in x[0]])
    m = api.M.NeRFSmall(3, 64, 15, 4, 64, False, 3, 64, 32, 16, "model", params=blob)
    return api.R.NeRFRenderer(e, api.M.SHEncoder("embeddirs", 3, 4), m), blob


def _params(api, bbox, chunk, **kw):
    return api.R.NeRFRenderParams(NSamples=64, NImportance=128, Chunk=chunk, ReturnRaw=True, LinDisp=False, Perturb=0.0, WhiteBkgr=True,
                                  RawNoiseStd=0.0, Ndc=False, UseViewdirs=True, ReturnWeights=True, ThinRay=True, BoundingBox=bbox,
                                  KeepIntermediates=True, **kw)


def test_render_hash_vs_reference(api, O, manifest):
    g = load_golden("render_hash")
    r, blob = _golden_hash_scene(api, manifest)
    res = r.Render(8, 8, g["k"], _params(api, g["bbox"], 64), c2w=g["c2w"])
    ex = {k: host(v) for k, v in res.Extras.items()}
    # ray batch: o, d, near, far exact; viewdirs = d/||d|| to 2 ulp of torch::norm's order
    assert_exact(ex["rays_flat"][:, :8], g["rays_flat"][:, :8], "rays_flat[o,d,near,far]")
    assert_close(ex["rays_flat"][:, 8:], g["rays_flat"][:, 8:], rtol=3e-7, atol=0)
    assert_exact(ex["z_coarse"], g["coarse_z"], "coarse z_vals")
    scale = np.abs(g["coarse_raw"]).max()
    assert_close(ex["raw_coarse"], g["coarse_raw"], rtol=0, atol=1e-4 * scale, what="coarse raw")
    assert (ex["z_fine"] == g["fine_z"]).mean() > 0.85        # discontinuous in the coarse weights (see CPU test)
    assert_close(host(res.Outputs.RGBMap), g["out_rgb"], rtol=0, atol=1e-4, what="pixels within 1e-4 of the reference")
    assert_close(host(res.Outputs.AccMap), g["out_acc"], rtol=0, atol=1e-4)
    assert_close(host(res.Outputs.DepthMap), g["out_depth"], rtol=0, atol=3e-4)
    assert abs(res.Near - g["near_far"][0]) == 0 and abs(res.Far - g["near_far"][1]) == 0
    assert api.S.psnr(host(res.Outputs.RGBMap), g["out_rgb"]) > 80
    # ---- stage-chained parity against the oracle on the GPU's OWN intermediates ----
    mid = O.z_mid(ex["z_coarse"])
    samples, _, _ = O.sample_pdf(mid, ex["weights_coarse"][:, 1:-1], O.linspace(0, 1, 128))
    assert_exact(ex["z_fine"], O.merge_sorted(ex["z_coarse"], samples), "fine depths given the GPU's coarse weights: bit-exact sample indices")
    wc = O.raw2outputs(ex["raw_coarse"], ex["z_coarse"], ex["rays_flat"][:, 3:6], True)["weights"]
    assert_exact(ex["weights_coarse"], wc, "coarse weights == oracle on the GPU's raw")
    fin = O.raw2outputs(host(res.Raw), ex["z_fine"], ex["rays_flat"][:, 3:6], True)
    assert_exact(host(res.Outputs.RGBMap).reshape(-1, 3), fin["rgb"], "pixels == oracle compositing of the GPU's raw")
    # fp32 parity mode: the network output equals the oracle's bit for bit on the same points
    model = O.Model(0, blob, bbox=g["bbox"], table_f32=synth.blob_from_manifest([x for x in manifest["render_hash"] if "embeddings" in x[0]]))
    oc = O.render_rays(model, ex["rays_flat"], 64, 128, O.linspace(0, 1, 64), O.linspace(0, 1, 128), white_bkgr=True, want_intermediates=True)
    assert_exact(ex["rays_flat"], O.pack_rays(ex["rays_flat"][:, :3], ex["rays_flat"][:, 3:6], g["bbox"]), "packed rays == oracle")
    assert_exact(ex["raw_coarse"], oc["raw_coarse"], "NRF_PREC_F32 coarse raw == oracle")
    assert_exact(ex["z_fine"], oc["z_fine"], "END-TO-END sample set == oracle (indices bit-exact through both passes)")
    assert_exact(host(res.Raw), oc["raw_fine"], "fine raw == oracle")
    assert_exact(host(res.Outputs.RGBMap).reshape(-1, 3), oc["rgb"], "END-TO-END pixels == oracle bit for bit")
    assert_exact(host(res.Outputs.DepthMap).reshape(-1), oc["depth"]); assert_exact(host(res.Outputs.AccMap), oc["acc"])


def test_render_hash_chunk_invariance_and_ray_batch(api, manifest):
    g = load_golden("render_hash")
    r, _ = _golden_hash_scene(api, manifest)
    a = r.Render(8, 8, g["k"], _params(api, g["bbox"], 64), c2w=g["c2w"])
    b = r.Render(8, 8, g["k"], _params(api, g["bbox"], 24), c2w=g["c2w"])
    assert_exact(host(a.Outputs.RGBMap), host(b.Outputs.RGBMap), "Chunk does not affect results")
    assert_close(host(b.Outputs.RGBMap), g["chunk24_rgb"], rtol=0, atol=1e-4)
    # explicit ray batch + LinDisp + black background (training-style call)
    gl = load_golden("render_hash_lindisp")
    o, d, cone = api.R.GetRays(8, 8, g["k"], g["c2w"])
    p = _params(api, g["bbox"], 64); p.LinDisp = True; p.WhiteBkgr = False
    res = r.Render(0, 0, None, p, rays=(o.reshape(-1, 3)[:40], d.reshape(-1, 3)[:40], cone))
    assert_exact(host(res.Extras["z_coarse"]), gl["coarse_z"], "lindisp z_vals")
    assert_close(host(res.Outputs.RGBMap), gl["out_rgb"], rtol=0, atol=1e-4)


def test_render_classic_vs_reference(api, O, manifest):
    g = load_golden("render_classic")
    blob = synth.blob_from_manifest(manifest["render_classic"])
    m = api.M.NeRF(8, 256, 63, 27, 5, (4,), True, "model", params=blob)
    r = api.R.NeRFRenderer(api.M.Embedder("embedder", 10), api.M.Embedder("embeddirs", 4), m)
    res = r.Render(8, 8, g["k"], _params(api, g["bbox"], 64), c2w=g["c2w"])
    assert_exact(host(res.Extras["z_coarse"]), g["coarse_z"])
    scale = np.abs(g["coarse_raw"]).max()
    assert_close(host(res.Extras["raw_coarse"]), g["coarse_raw"], rtol=0, atol=2e-4 * scale)
    assert_close(host(res.Outputs.RGBMap), g["out_rgb"], rtol=0, atol=2e-4, what="classic pixels (PE sin/cos + 10-layer fp32 MLP)")
    assert api.S.psnr(host(res.Outputs.RGBMap), g["out_rgb"]) > 75
    model = O.Model(1, blob, bbox=g["bbox"])
    rays = host(res.Extras["rays_flat"])
    oc = O.render_rays(model, rays, 64, 128, O.linspace(0, 1, 64), O.linspace(0, 1, 128), white_bkgr=True, want_intermediates=True)
    assert_exact(host(res.Extras["z_fine"]), oc["z_fine"], "classic: end-to-end sample set == oracle")
    assert_exact(host(res.Outputs.RGBMap).reshape(-1, 3), oc["rgb"], "classic: end-to-end pixels == oracle bit for bit")
    # coarse only (N_importance = 0): the reference returns undefined maps; here the coarse maps, equal to RawToOutputs of the coarse pass
    gc = load_golden("render_classic_coarse")
    p = _params(api, g["bbox"], 1024); p.NImportance = 0
    rc = r.Render(8, 8, g["k"], p, c2w=g["c2w"])
    assert_close(host(rc.Outputs.RGBMap).reshape(-1, 3), gc["out_rgb"], rtol=0, atol=1e-4)


def test_render_hash_f16_mfma_pixels(api, manifest):
    g = load_golden("render_hash")
    r, _ = _golden_hash_scene(api, manifest)
    res = r.Render(8, 8, g["k"], _params(api, g["bbox"], 64, Precision=api.L.NRF_PREC_F16_MFMA), c2w=g["c2w"])
    rgb = host(res.Outputs.RGBMap)
    err = np.abs(rgb - g["out_rgb"]).max()
    # fp16 matrix-core MLP: reported, bounded loosely here; the headline tolerance applies to NRF_PREC_F32
    assert err < 2e-2 and api.S.psnr(rgb, g["out_rgb"]) > 40, err


# ------------------------------------------------------------------ full-size, size-independent properties
def test_full_size_row_tile_properties(api, O):
    """BASELINE config 3 shape (1-based, as BASELINE.md / SURVEY 8 count them): 800x800 camera, 64+128, HashNeRF (CuHash mode), one 16-row tile (12 800 rays, 3.3 M points).
    Properties: finite, acc in [0,1], rgb in [0,1+eps], depth within [near, far]; tile == slice-of-image by construction of
    the ray index; permuting rays permutes pixels (ray independence); a random 64-ray sample equals the oracle."""
    sc = api.S.make_hash_scene(mode="cu")
    K = api.S.lego_K(800, 800); c2w = api.S.pose_spherical(30.0, -30.0, 4.0)
    rp = api.S.lego_render_params(sc["bbox"], chunk=4096, ReturnWeights=False)
    res = sc["renderer"].Render(800, 800, K, rp, c2w=c2w, row0=392, rows=16)
    rgb = host(res.Outputs.RGBMap).reshape(-1, 3); acc = host(res.Outputs.AccMap); dep = host(res.Outputs.DepthMap).reshape(-1)
    rays = host(res.Extras["rays_flat"])
    assert np.isfinite(rgb).all() and np.isfinite(dep).all()
    assert acc.min() >= 0 and acc.max() <= 1 + 1e-5 and rgb.min() >= -1e-5 and rgb.max() <= 1 + 1e-5
    hit = acc > 1e-3
    assert hit.mean() > 0.5
    assert (dep[hit] >= rays[hit, 6] - 1e-4).all() and (dep[hit] <= rays[hit, 7] + 1e-4).all()
    # ray independence: a permuted explicit batch gives the permuted pixels, bit for bit
    perm = np.random.RandomState(0).permutation(rays.shape[0])[:4096]
    sub = sc["renderer"].Render(0, 0, None, rp, rays=(dev(rays[perm, 0:3]), dev(rays[perm, 3:6]), None))
    assert_exact(host(sub.Outputs.RGBMap), rgb[perm], "ray order independence")
    # sample against the oracle (CuHash restatement + CuSH + NeRFSmall), fp32 parity mode
    idx = perm[:64]
    cfg = sc["cfg"]
    ls = ((1 << cfg["log2_t"]) >> 4) << 4
    model = O.Model(2, sc["mlp_blob"], bbox=sc["bbox"], table_f16=O.f32_to_f16(sc["table"]), primes=sc["primes"],
                    local_idx=np.arange(16, dtype=np.int32) * ls, local_size=np.full(16, ls, np.int32), bias=np.zeros((16, 3), np.float32),
                    mul=O.hash_cu_scales(16, 16, 512))
    ref = O.render_rays(model, rays[idx], 64, 128, O.linspace(0, 1, 64), O.linspace(0, 1, 128), white_bkgr=True)
    assert_exact(rgb[idx], ref["rgb"], "800x800 sample == oracle bit for bit (CuHash mode, fp32 parity precision)")


# ------------------------------------------------------------------ fused fast path (NRF_PREC_F16_MFMA)
def test_fast_path_equals_stagewise_f16(api):
    """The renderer's fused path (level-major fp16 hash features -> fused MFMA MLP, CuHash mode) must produce the same raw
    network outputs, bit for bit, as composing the public stage functions on the same points:
    CuHashEmbedder.forward -> CuSHEncoder.forward -> cat -> NeRFSmall.forward(NRF_PREC_F16_MFMA) -> sigma mask."""
    sc = api.S.make_hash_scene(mode="cu")
    K = api.S.lego_K(800, 800); c2w = api.S.pose_spherical(30.0, -30.0, 4.0)
    rp = api.S.lego_render_params(sc["bbox"], chunk=1000, precision=api.L.NRF_PREC_F16_MFMA, ReturnRaw=True, KeepIntermediates=True)
    res = sc["renderer"].Render(800, 800, K, rp, c2w=c2w, row0=400, rows=2)          # 1600 rays, two ragged chunks
    rays = res.Extras["rays_flat"]; zc = res.Extras["z_coarse"]; zf = res.Extras["z_fine"]
    for z, raw in ((zc, res.Extras["raw_coarse"]), (zf, res.Raw)):
        n, s = z.shape
        pts = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]).reshape(-1, 3)
        # o + d*z must be formed with the same two roundings as the kernel (mul, add): torch does exactly that
        emb, keep = sc["embedder"].forward(pts)
        dirs, _ = sc["embeddirs"].forward(rays[:, 8:11].contiguous())
        x = torch.cat([emb, dirs[:, None, :].expand(n, s, dirs.shape[1]).reshape(n * s, -1)], 1).contiguous()
        ref = sc["mlp"].forward(x, api.L.NRF_PREC_F16_MFMA)
        ref[~keep, 3] = 0
        assert_exact(host(raw).reshape(-1, 4), host(ref), "fused fast path raw == stage-wise F16 raw")
    assert np.isfinite(host(res.Outputs.RGBMap)).all()


def test_fast_path_pixels_close_to_parity_mode(api):
    sc = api.S.make_hash_scene(mode="cu", sigma_scale=4.0)      # a smoother density field than the adversarial default
    K = api.S.lego_K(800, 800); c2w = api.S.pose_spherical(30.0, -30.0, 4.0)
    a = sc["renderer"].Render(800, 800, K, api.S.lego_render_params(sc["bbox"], chunk=4096, precision=api.L.NRF_PREC_F16_MFMA), c2w=c2w, row0=396, rows=8)
    b = sc["renderer"].Render(800, 800, K, api.S.lego_render_params(sc["bbox"], chunk=4096, precision=api.L.NRF_PREC_F32), c2w=c2w, row0=396, rows=8)
    ps = api.S.psnr(host(a.Outputs.RGBMap), host(b.Outputs.RGBMap))
    assert ps > 45, ps


def test_mlp_nerf_f16_mfma(api, manifest):
    g = load_golden("mlp_nerf")
    blob = synth.blob_from_manifest(manifest["mlp_nerf"])
    m = api.M.NeRF(8, 256, 63, 27, 5, (4,), True, "model", params=blob)
    x = np.tile(g["x"], (12, 1))[:700]                 # 700 points: two full 256-point blocks + a ragged one
    y = host(m.forward(dev(x), api.L.NRF_PREC_F16_MFMA))
    ref = np.tile(g["y"], (12, 1))[:700]
    scale = np.abs(ref).max()
    assert_close(y, ref, rtol=0, atol=4e-3 * scale, what="classic NeRF fp16 MFMA vs reference")
    assert np.abs(y - ref).mean() < 6e-4 * scale
    f32 = host(m.forward(dev(x), api.L.NRF_PREC_F32))
    assert np.abs(y - f32).mean() < 6e-4 * scale


def test_render_classic_f16_mfma_pixels(api, manifest):
    g = load_golden("render_classic")
    blob = synth.blob_from_manifest(manifest["render_classic"])
    m = api.M.NeRF(8, 256, 63, 27, 5, (4,), True, "model", params=blob)
    r = api.R.NeRFRenderer(api.M.Embedder("embedder", 10), api.M.Embedder("embeddirs", 4), m)
    res = r.Render(8, 8, g["k"], _params(api, g["bbox"], 64, Precision=api.L.NRF_PREC_F16_MFMA), c2w=g["c2w"])
    rgb = host(res.Outputs.RGBMap)
    assert np.isfinite(rgb).all() and api.S.psnr(rgb, g["out_rgb"]) > 35


def test_libtorch_adapter_drop_in_inside_reference_renderer(tmp_path):
    """oracle/_ref/adapter_check (compiled where /root/reference exists, travels as a binary): the C++ LibTorch adapter
    classes of include/nerfpp_torch.h driven by the reference's own NeRFRenderer::Render / BatchifyRays, compared with the
    reference CPU renderer on the same weights; plus the MODULE STATE of the drop-in embedders: HipHashEmbedder(CU) built from
    scratch draws its primes as CuHashEmbedder.cpp:28-51 does and registers the reference's four buffers, the NGP mode carries
    `embedder_embeddings_<i>.weight`, the reference-written checkpoint fixtures torch::load into the adapters, and the files the
    adapters torch::save load into the REFERENCE's modules (ref_driver ckpt_load)."""
    import json, os, shutil, subprocess
    from conftest import ROOT, GOLDEN
    exe = os.path.join(ROOT, "oracle", "_ref", "adapter_check")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/adapter_check not built (needs /root/reference at build time)")
    outd = str(tmp_path / "adapter_ckpt"); os.makedirs(outd)
    env = dict(os.environ, NRF_ADAPTER_CKPT_DIR=os.path.join(GOLDEN, "ckpt"), NRF_ADAPTER_OUT_DIR=outd)
    out = subprocess.run([exe, "16", "16"], capture_output=True, text=True, timeout=600, env=env)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert lines, out.stdout + out.stderr
    r = json.loads(lines[-1])
    ms = json.loads(lines[-2])
    assert out.returncode == 0 and r["ok"], (r, ms)
    assert r["hash_embedding_bit_exact"] and r["sh_bit_exact"] and r["shapes_near_far_equal"]
    assert r["pixels_within_1e-4"] >= 0.90 and r["psnr_db"] > 55, r
    assert r["split_pixels_within_1e-4"] >= 0.90 and r["split_psnr_db"] > 55, r      # the matrix-core fast path behind the reference's own Render()
    assert r["split_vs_own_f32_max_abs_err"] < 1e-4, r                                # strict: every pixel of the split render within 1e-4 of the adapter's parity render
    assert r["render_tile_equals_slice"] and r["render_sharded_world1_equals_render"], r     # multi-GPU surface: RenderTile / RenderSharded over a TileComm (world of one)
    lr = json.loads(lines[-3])                                                        # the LeRF pass: HipLeRFPass (what HipLeRFRenderer forwards to) vs the reference's LeRF module
    assert lr["lerf_pass_ok"] and lr["lerf_fused"], lr
    assert lr["lerf_single_library_call_equals_host_loop"] and lr["lerf_relevancy_ok"], lr            # nrf_lerf_render_rays / _render_rows behind HipLeRFPass; Relevancy filled
    assert lr["lerf_split_cos_min_vs_reference_head"] > 1 - 2e-6 and lr["lerf_split_weights_max_abs_err"] < 1e-5, lr
    # module state of the drop-in
    assert ms["module_state_ok"] and ms["parameter_names_equal_reference"] and ms["cu_from_scratch_primes_table_buffers_ok"] and ms["zero_primes_rejected"], ms
    assert ms["torch_load_cu_fixture"] and ms["torch_load_ngp_fixture_forward_bit_exact"] and ms["adapter_checkpoints_saved"], ms
    assert ms["chunk_loop_library_equals_reference_batchify"] and ms["ndc_viewdirs_ok"] and ms["staticcam_ok"], ms
    drv = os.path.join(ROOT, "oracle", "_ref", "ref_driver")
    if os.path.exists(drv):
        # the adapter-saved embedder files next to the reference-written model / start files -> the reference's own torch::load into ITS modules
        for f in ("model_checkpoint.pt", "start_checkpoint.pt"):
            shutil.copy(os.path.join(GOLDEN, "ckpt", f), outd)
        dump = str(tmp_path / "dump"); os.makedirs(dump)
        subprocess.check_call([drv, "ckpt_load", outd, dump], stdout=subprocess.DEVNULL)
        ref_dump = str(tmp_path / "ref_dump"); os.makedirs(ref_dump)
        subprocess.check_call([drv, "ckpt_load", os.path.join(GOLDEN, "ckpt"), ref_dump], stdout=subprocess.DEVNULL)
        names = [f for f in os.listdir(ref_dump) if f.startswith(("e.", "cu."))]
        assert len(names) >= 4 + 5
        for f in names:        # the adapters had loaded the fixtures, so what they saved must restore the same numbers
            np.testing.assert_array_equal(np.load(os.path.join(dump, f)), np.load(os.path.join(ref_dump, f)), err_msg=f)


def test_classic_fused_path_equals_stagewise_f16(api):
    """Classic NeRF fast path (points + PE formed inside the 8x256 matrix-core kernel) == Embedder.forward -> cat -> NeRF.forward(F16)."""
    sc = api.S.make_classic_scene()
    K = api.S.lego_K(800, 800); c2w = api.S.pose_spherical(30.0, -30.0, 4.0)
    rp = api.S.lego_render_params(sc["bbox"], chunk=700, precision=api.L.NRF_PREC_F16_MFMA, ReturnRaw=True, KeepIntermediates=True)
    res = sc["renderer"].Render(800, 800, K, rp, c2w=c2w, row0=400, rows=1)           # 800 rays, two ragged chunks
    rays = res.Extras["rays_flat"]
    for z, raw in ((res.Extras["z_coarse"], res.Extras["raw_coarse"]), (res.Extras["z_fine"], res.Raw)):
        n, s = z.shape
        pts = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]).reshape(-1, 3)
        emb, _ = sc["embedder"].forward(pts)
        dirs, _ = sc["embeddirs"].forward(rays[:, 8:11].contiguous())
        x = torch.cat([emb, dirs[:, None, :].expand(n, s, dirs.shape[1]).reshape(n * s, -1)], 1).contiguous()
        ref = sc["mlp"].forward(x, api.L.NRF_PREC_F16_MFMA)
        assert_exact(host(raw).reshape(-1, 4), host(ref), "fused classic raw == stage-wise F16 raw")


# ------------------------------------------------------------------ edge cases
def test_edge_cases_empty_ragged_and_limits(api):
    import ctypes as C
    sc = api.S.make_hash_scene(mode="cu", log2_t=14)
    r = sc["renderer"]
    K = api.S.lego_K(64, 64); c2w = api.S.pose_spherical(10.0, -30.0, 4.0)
    o, d, cone = api.R.GetRays(64, 64, K, c2w)
    o = o.reshape(-1, 3); d = d.reshape(-1, 3)
    ragged = {}
    for prec in (api.L.NRF_PREC_F32, api.L.NRF_PREC_F16_MFMA, api.L.NRF_PREC_F16_SPLIT):
        # ragged sample counts (not multiples of 64), n = 1 ray, n = 0 rays
        p = api.S.lego_render_params(sc["bbox"], n_samples=37, n_importance=53, chunk=97, precision=prec, ReturnWeights=True)
        full = r.Render(0, 0, None, p, rays=(o[:301], d[:301], None))
        assert host(full.Outputs.Weights).shape == (301, 90) and np.isfinite(host(full.Outputs.RGBMap)).all()
        ragged[prec] = full
        one = r.Render(0, 0, None, p, rays=(o[5:6], d[5:6], None))
        assert_exact(host(one.Outputs.RGBMap), host(full.Outputs.RGBMap)[5:6], "a single ray renders like the same ray inside a batch")
        # coarse only
        p0 = api.S.lego_render_params(sc["bbox"], n_samples=64, n_importance=0, chunk=128, precision=prec, ReturnWeights=True)
        c = r.Render(0, 0, None, p0, rays=(o[:200], d[:200], None))
        assert host(c.Outputs.Weights).shape == (200, 64)
    # the default split mode at ragged sizes (exact coarse pass with the geo hand-over, colour net alone at the 37 coarse depths, partial 64-point blocks everywhere)
    assert_close(host(ragged[api.L.NRF_PREC_F16_SPLIT].Outputs.RGBMap), host(ragged[api.L.NRF_PREC_F32].Outputs.RGBMap), rtol=0, atol=1e-4, what="ragged split render vs fp32")
    assert_close(host(ragged[api.L.NRF_PREC_F16_SPLIT].Outputs.Weights), host(ragged[api.L.NRF_PREC_F32].Outputs.Weights), rtol=0, atol=2e-5, what="ragged split weights vs fp32")
    empty = r.RenderRays(torch.empty((0, 11), device="cuda"), None, 64, n_importance=128)
    assert empty.Outputs.RGBMap.shape == (0, 3)
    # limits are reported, not silently mis-rendered
    with pytest.raises(api.L.NrfError, match="outside the built range"):
        r.RenderRays(torch.zeros((4, 11), device="cuda"), None, 300, n_importance=128)
    with pytest.raises(api.L.NrfError, match="bbox required"):
        r.RenderRays(torch.zeros((4, 11), device="cuda"), None, 64, n_importance=128, stochastic_preconditioning_alpha=0.01)
    # degenerate stochastic inputs: zero-length rays with a cone, all-zero weights with random u -> finite results
    deg = r.RenderRays(torch.zeros((4, 11), device="cuda"), torch.tensor(0.001), 64, n_importance=128, perturb=1.0)
    assert np.isfinite(host(deg.Outputs.RGBMap)).all()
    smp = api.R.SamplePDF(torch.zeros((2, 63), device="cuda"), torch.zeros((2, 62), device="cuda"), 128, det=False, seed=3)
    assert smp.shape == (2, 128) and np.isfinite(host(smp)).all()
    # rays that miss the box entirely: transparent, white background, finite depth
    far_o = torch.tensor([[10.0, 10.0, 10.0]], device="cuda").repeat(8, 1); away = torch.tensor([[1.0, 0.2, 0.1]], device="cuda").repeat(8, 1)
    miss = r.Render(0, 0, None, api.S.lego_render_params(sc["bbox"], chunk=8), rays=(far_o, away, None))
    assert_exact(host(miss.Outputs.AccMap), np.zeros(8, np.float32)); assert_exact(host(miss.Outputs.RGBMap), np.ones((8, 3), np.float32))


def test_hash_fast_path_fallbacks_bit_exact(api, O):
    """Dense pyramid off (budget 0), a partial bake (50 MB) and the default all-dense image give identical features on the default scene.  (Biased grids -- which disable
    the dense image -- and the other shapes the dispatch distinguishes are tests/test_hash_shapes_gpu.py's.)"""
    import ctypes as C
    lib = api.L.lib()
    sc = api.S.make_hash_scene(mode="cu")
    e = sc["embedder"]
    x = synth.synth_sym(99, (20000, 3), np.float32(1.6))
    xd = dev(x)
    P = lambda t: C.c_void_p(t.data_ptr())
    feats = torch.empty((16, x.shape[0], 2), device="cuda", dtype=torch.float16); keep = torch.empty((x.shape[0],), device="cuda", dtype=torch.uint8)
    ref, _ = e.forward(xd)                                             # generic hashed kernel
    outs = []
    for budget in (1 << 34, 50 << 20, 0):
        e.set_dense_budget(budget)
        api.L.check(lib.nrf_dbg_hash_lm(e._h, P(xd), C.c_int64(x.shape[0]), 0, 0, -1, P(feats), P(keep), None))
        outs.append(host(feats.permute(1, 0, 2).reshape(x.shape[0], 32).float()))
        assert_exact(outs[-1], host(ref), f"dense budget {budget}")
    e.set_dense_budget(1 << 34)


def test_hash_baked_lookup_on_faces_lattice_points_and_outside(api):
    """The baked-level lookup takes its cell index by a truncating conversion, its fraction by v_fract_f32 and its loads / stores through buffer resources
    (hash_fast.h): against the generic hashed kernel on the inputs where those forms could differ -- coordinates ON the box faces (q = 0 and q = mul exactly),
    points on the lattice of the coarsest and of the finest level (fraction exactly 0), points outside the box (clamped, keep mask false) and 10^6 random ones."""
    import ctypes as C
    lib = api.L.lib()
    sc = api.S.make_hash_scene(mode="cu"); e = sc["embedder"]
    n = 1_000_000
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    base = torch.rand((n, 3), device="cuda", generator=g) * 3.0 - 1.5
    sets = {"random": base}
    b = base.clone(); ax = torch.randint(0, 3, (n,), device="cuda", generator=g); sgn = torch.randint(0, 2, (n,), device="cuda", generator=g).float() * 3.0 - 1.5
    b[torch.arange(n, device="cuda"), ax] = sgn; sets["one coordinate on a box face"] = b
    sets["outside the box"] = base * 1.3
    sets["level-0 lattice"] = torch.round((base + 1.5) / 3.0 * 16.0) / 16.0 * 3.0 - 1.5
    sets["level-15 lattice"] = torch.round((base + 1.5) / 3.0 * 512.0) / 512.0 * 3.0 - 1.5
    P = lambda t: C.c_void_p(t.data_ptr())
    for name, pts in sets.items():
        pts = pts.contiguous()
        x = torch.empty((16, n, 2), device="cuda", dtype=torch.float16); k = torch.empty((n,), device="cuda", dtype=torch.uint8)
        api.L.check(lib.nrf_hash_encode_lm_f16(e._h, P(pts), C.c_int64(n), P(x), P(k), None))
        emb, keep = e.forward(pts)                                              # generic hashed kernel, fp32 rows (the values are fp16 numbers)
        ref = emb.reshape(-1, 16, 2).permute(1, 0, 2).to(torch.float16)
        assert int((ref != x).sum()) == 0, name
        assert int((keep.to(torch.uint8) != k).sum()) == 0, name


def test_hash_encode_beside_matrix_core_kernels_on_another_stream(api):
    """The encode's blend is inline asm (v_fma_mix_f32) fed by compiler-generated vector instructions.  A build in which those were PACKED fp32 instructions was bit-identical
    on every single-stream check and wrong while matrix-core kernels ran on another stream (packed fp32 shares the matrix data path, its result latency
    depends on other waves, and the compiler's hazard padding does not see the asm consumer).  The two-lane Chunk loop makes that the normal situation: the encode entry,
    repeated while the split-precision MLP runs on a second stream, must reproduce its solo features every time."""
    import ctypes as C
    lib = api.L.lib()
    sc = api.S.make_hash_scene(mode="cu"); e = sc["embedder"]
    n = 2_000_000
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    pts = (torch.rand((n, 3), device="cuda", generator=g) * 3.0 - 1.5).contiguous()
    P = lambda t: C.c_void_p(t.data_ptr())
    ref = torch.empty((16, n, 2), device="cuda", dtype=torch.float16); k = torch.empty((n,), device="cuda", dtype=torch.uint8)
    api.L.check(lib.nrf_hash_encode_lm_f16(e._h, P(pts), C.c_int64(n), P(ref), P(k), None)); torch.cuda.synchronize()
    xin = torch.randn((1_000_000, 48), device="cuda") * 0.1
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    with torch.cuda.stream(sa):
        for _ in range(24): sc["mlp"].forward(xin, api.L.NRF_PREC_F16_SPLIT)
    with torch.cuda.stream(sb):
        for _ in range(10):
            x = torch.empty((16, n, 2), device="cuda", dtype=torch.float16)
            api.L.check(lib.nrf_hash_encode_lm_f16(e._h, P(pts), C.c_int64(n), P(x), P(k), C.c_void_p(sb.cuda_stream)))
            outs.append(x)
    torch.cuda.synchronize()
    assert [int((o != ref).sum()) for o in outs] == [0] * 10


def test_raw2weights_gather_equals_gathered_rows(api):
    """nrf_raw2weights_gather (the LeRF fine pass composes sigma_le through the merge map) == nrf_raw2weights of the gathered rows, bit for bit."""
    import ctypes as C
    lib = api.L.lib()
    n, s = 300, 96
    rs = np.random.RandomState(11)
    sig = dev((rs.rand(n * s).astype(np.float32) * 8.0) * (rs.rand(n * s) > 0.3))
    src = dev(np.stack([rs.permutation(s) + i * s for i in range(n)]).astype(np.int32))
    z = dev(np.sort(rs.rand(n, s).astype(np.float32) * 4.0 + 2.0, axis=1)); d = dev(rs.randn(n, 3).astype(np.float32))
    P = lambda t: C.c_void_p(t.data_ptr())
    outs = []
    for mode in (0, 1):
        w = torch.empty((n, s), device="cuda"); dep = torch.empty((n,), device="cuda"); dsp = torch.empty((n,), device="cuda"); acc = torch.empty((n,), device="cuda")
        if mode == 0:
            api.L.check(lib.nrf_raw2weights_gather(P(sig), 1, 0, P(src), P(z), P(d), 3, C.c_int64(n), s, P(w), P(dep), P(dsp), P(acc), None))
        else:
            g = sig[src.reshape(-1).long()].contiguous()
            api.L.check(lib.nrf_raw2weights(P(g), 1, 0, P(z), P(d), 3, C.c_int64(n), s, P(w), P(dep), P(dsp), P(acc), None))
        torch.cuda.synchronize()
        outs.append([host(w), host(dep), host(dsp), host(acc)])
    for a_, b_, nm in zip(outs[0], outs[1], ("weights", "depth", "disp", "acc")):
        assert_exact(a_, b_, "raw2weights through the map == gathered rows: " + nm)


# ------------------------------------------------------------------ LeRF (BASELINE config 5)
def test_lerf_render_pass_vs_oracle(api, O, manifest):
    """LeRFRenderer::RenderRays minus the external Relevancy: CuHashEmbedder(F=8) -> LeRF head -> sigma_le weights ->
    RenderCLIPEmbedding, against the oracle composed stage by stage on the same rays."""
    Lv, F, T = 16, 8, 12
    bbox = api.S.LEGO_BBOX
    e = api.M.CuHashEmbedder("lang_embedder", bbox, Lv, F, T, 16, 128)
    table = synth.synth_sym(311, (Lv * (1 << T) * F,), np.float32(0.5))
    primes = np.array(api.S.CU_PRIMES[:3 * Lv], np.int32)
    e.set_table(table); e.set_primes(primes)
    blob = synth.blob_from_manifest(manifest["lerf"])
    blob = blob.copy(); blob[128 * 256:128 * 256 + 256] *= 20.0            # row 0 of sigma_le_net_1: a density that is not ~0
    lerf = api.M.LeRF(32, 2, 256, 768, 128, "lang_model", params=blob)
    r = api.R.LeRFRenderer(e, lerf)
    K = api.S.lego_K(6, 6); c2w = api.S.pose_spherical(40.0, -30.0, 4.0)
    p = api.R.NeRFRenderParams(NSamples=16, NImportance=16, Chunk=20, ReturnRaw=True, Perturb=0.0, Ndc=False, UseViewdirs=True, ReturnWeights=True,
                               ThinRay=True, BoundingBox=bbox)
    res = r.Render(6, 6, K, p, c2w=c2w)
    rays = host(res.Extras["rays_flat"])
    # oracle, stage by stage
    ls = ((1 << T) >> 4) << 4
    def net(pts):
        emb, keep = O.hash_cu(pts.reshape(-1, 3), O.f32_to_f16(table), primes, np.arange(Lv, dtype=np.int32) * ls, np.full(Lv, ls, np.int32),
                              np.zeros((Lv, 3), np.float32), bbox, O.hash_cu_scales(Lv, 16, 128), Lv, F)
        o = O.lerf(blob, emb)
        o[~keep, -1] = 0
        return o.reshape(pts.shape[0], pts.shape[1], -1)
    z = O.z_vals(rays[:, 6], rays[:, 7], O.linspace(0, 1, 16))
    raw = net(O.points(rays[:, :3], rays[:, 3:6], z))
    w1 = O.raw2weights(raw, 768, z, rays[:, 3:6])["weights"]
    samples, _, _ = O.sample_pdf(O.z_mid(z), w1[:, 1:-1], O.linspace(0, 1, 16))
    zf = O.merge_sorted(z, samples)
    rawf = net(O.points(rays[:, :3], rays[:, 3:6], zf))
    fin = O.raw2weights(rawf, 768, zf, rays[:, 3:6])
    emb_ref = O.render_clip_embedding(rawf, 768, fin["weights"])
    assert fin["acc"].max() > 0.05, "fixture must have non-trivial language density"
    assert_close(host(res.Outputs.WeightsLE), fin["weights"], rtol=2e-4, atol=2e-6, what="WeightsLE")
    assert_close(host(res.Outputs.DepthMapLE), fin["depth"], rtol=2e-4, atol=2e-5)
    hit = fin["acc"] > 1e-3
    assert_close(host(res.Outputs.RenderedLangEmbedding)[hit], emb_ref[hit], rtol=0, atol=2e-4, what="rendered CLIP embedding")
    assert_close(np.linalg.norm(host(res.Outputs.RenderedLangEmbedding)[hit], axis=1), np.ones(hit.sum()), rtol=1e-5, atol=0)
    # the stage functions on the oracle's own inputs are exact
    w_gpu = api.R.LeRFRenderer.RawToLEOutputs(r, dev(rawf), dev(zf), dev(rays[:, 3:6]), 768)
    assert_exact(host(w_gpu.WeightsLE), fin["weights"], "nrf_raw2weights == oracle")
    assert_close(host(w_gpu.RenderedLangEmbedding)[hit], emb_ref[hit], rtol=1e-6, atol=1e-7, what="nrf_render_clip_embedding")


# ------------------------------------------------------------------ stochastic branches (R6 jitter, R7 TangentScatter, det=false, noise)
def test_counter_rng_matches_oracle(api, O):
    for stream, normal in ((api.L.NRF_RNG_T_RAND, False), (api.L.NRF_RNG_U_PDF, False), (api.L.NRF_RNG_PRECOND, True)):
        got = host(api.R.RngFill(1234567, stream, 1000003, 70001, normal=normal))
        ref = O.rng_normal(1234567, stream, 1000003, 70001) if normal else O.rng_uniform(1234567, stream, 1000003, 70001)
        assert_exact(got, ref, f"nrf_rng_fill stream {stream}")
    big = host(api.R.RngFill(5, 2, (1 << 40) + 17, 4096))               # 64-bit element indices
    assert_exact(big, O.rng_uniform(5, 2, (1 << 40) + 17, 4096))


@pytest.mark.parametrize("tag", ["render_stoch", "render_stoch_train"])
def test_stochastic_stages_with_reference_draws(api, O, tag):
    """Every stochastic stage fed the reference's inputs and its replayed torch::rand / randn draws: == oracle bit for bit, and within
    the sin/cos ulp of the reference's LibTorch values."""
    g = load_golden(tag)
    train = tag.endswith("train")
    rays, bbox, cone = g["rays_flat"], load_golden("render_hash")["bbox"], float(g["cone_angle"][0])
    ns, ni = 32, 48
    z0 = O.z_vals(rays[:, 6], rays[:, 7], O.linspace(0, 1, ns))
    zj = host(api.R.JitterZ(dev(z0), dev(g["t_rand"])))
    assert_exact(zj, g["coarse_z"], "stratified jitter == reference")
    p0 = O.points(rays[:, :3], rays[:, 3:6], zj)
    pts = host(api.R.TangentScatter(dev(p0), dev(zj), cone, dev(rays[:, 3:6]), bbox, dev(g["u_r1"]), dev(g["u_theta1"])))
    assert_exact(pts, O.tangent_scatter(p0, zj, cone, rays[:, 3:6], g["u_r1"], g["u_theta1"], bbox), "TangentScatter == oracle")
    assert_close(pts, g["coarse_pts"], rtol=0, atol=2e-7, what="TangentScatter vs reference")
    samples, inds = api.R.SamplePDF(dev(O.z_mid(g["coarse_z"])), dev(g["coarse_weights"][:, 1:-1]), ni, det=False, return_inds=True, u=dev(g["u_pdf"]))
    s_ref, i_ref = O.sample_pdf_rand(O.z_mid(g["coarse_z"]), g["coarse_weights"][:, 1:-1], g["u_pdf"])
    assert_exact(host(inds), i_ref, "det=false searchsorted indices"); assert_exact(host(samples), s_ref)
    import ctypes as C
    zf = torch.empty((rays.shape[0], ns + ni), device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    zc, wc, up = dev(g["coarse_z"]), dev(g["coarse_weights"]), dev(g["u_pdf"])
    api.L.check(api.L.lib().nrf_fine_depths_rand(P(zc), P(wc), C.c_int64(rays.shape[0]), ns, P(up), ni, 8, P(zf), None))
    assert_exact(host(zf), g["fine_z"], "fine depth set (unsorted draws -> sort) == reference")
    pf = O.points(rays[:, :3], rays[:, 3:6], g["fine_z"])
    if train:
        pre = host(api.R.StochasticPrecondition(dev(pf), dev(g["precond"]), 0.01, bbox))
        assert_exact(pre, O.precondition(pf, g["precond"], 0.01, bbox), "preconditioning + ReflectBoundary == oracle")
        pf = pre
    pf2 = host(api.R.TangentScatter(dev(pf), dev(g["fine_z"]), cone, dev(rays[:, 3:6]), bbox, dev(g["u_r2"]), dev(g["u_theta2"])))
    assert_close(pf2, g["fine_pts"], rtol=0, atol=5e-7, what="fine points vs reference")
    if train:
        r = api.R.NeRFRenderer.RawToOutputs(None, dev(g["fine_raw"]), None, dev(g["fine_z"]), dev(rays[:, 3:6]), 0.5, True, noise=dev(g["noise2"]))
        ref = O.raw2outputs_noise(g["fine_raw"], g["fine_z"], rays[:, 3:6], g["noise2"], 0.5, True)
        assert_exact(host(r.RGBMap), ref["rgb"], "RawToOutputs(raw_noise_std) == oracle"); assert_exact(host(r.Weights), ref["weights"])
        assert_close(host(r.RGBMap), g["out_rgb"], rtol=0, atol=2e-6, what="vs reference")


@pytest.mark.parametrize("train", [False, True])
def test_stochastic_render_bit_exact_vs_oracle_and_chunk_independent(api, O, manifest, train):
    """nrf_render_rays with its in-kernel counter RNG == the oracle generating the same draws; Chunk does not matter."""
    g = load_golden("render_hash")
    bbox = g["bbox"]
    r, blob = _golden_hash_scene(api, manifest)
    kw = dict(RawNoiseStd=0.5, StochasticPreconditioningAlpha=0.01) if train else {}
    def params(chunk):
        p = _params(api, bbox, chunk, Seed=4242, **{k: v for k, v in kw.items() if k != "RawNoiseStd"})
        p.NSamples, p.NImportance, p.ThinRay, p.Perturb = 32, 48, False, 1.0
        p.RawNoiseStd = kw.get("RawNoiseStd", 0.0)
        return p
    a = r.Render(8, 8, g["k"], params(64), c2w=g["c2w"])
    b = r.Render(8, 8, g["k"], params(24), c2w=g["c2w"])
    assert_exact(host(a.Outputs.RGBMap), host(b.Outputs.RGBMap), "stochastic render independent of Chunk")
    _, _, cone = api.R.GetRays(8, 8, g["k"], g["c2w"])
    model = O.Model(0, blob, bbox=bbox, table_f32=synth.blob_from_manifest([x for x in manifest["render_hash"] if "embeddings" in x[0]]))
    st = dict(perturb=1.0, cone_angle=float(cone), seed=4242, raw_noise_std=kw.get("RawNoiseStd", 0.0), precond_alpha=kw.get("StochasticPreconditioningAlpha", 0.0))
    oc = O.render_rays(model, host(a.Extras["rays_flat"]), 32, 48, O.linspace(0, 1, 32), None, white_bkgr=True, want_intermediates=True, stoch=st)
    assert_exact(host(a.Extras["z_coarse"]), oc["z_coarse"], "jittered depths"); assert_exact(host(a.Extras["z_fine"]), oc["z_fine"], "fine sample set")
    assert_exact(host(a.Raw), oc["raw_fine"], "fine raw (scattered points through the network)")
    assert_exact(host(a.Outputs.RGBMap).reshape(-1, 3), oc["rgb"], "stochastic pixels == oracle bit for bit")
    # a different seed is a different sample of the estimator; the same seed reproduces
    p2 = params(64); p2.Seed = 4243
    c = r.Render(8, 8, g["k"], p2, c2w=g["c2w"])
    assert np.abs(host(c.Outputs.RGBMap) - host(a.Outputs.RGBMap)).max() > 1e-3
    assert_exact(host(r.Render(8, 8, g["k"], params(64), c2w=g["c2w"]).Outputs.RGBMap), host(a.Outputs.RGBMap), "same seed reproduces")
    # row-tile sharding (multi-GPU) draws the same numbers as the whole image
    t = r.Render(8, 8, g["k"], params(64), c2w=g["c2w"], row0=3, rows=2)
    assert_exact(host(t.Outputs.RGBMap), host(a.Outputs.RGBMap)[3:5], "row tile == slice of the full stochastic render")


def test_stochastic_fast_paths_use_same_points(api, manifest):
    """The matrix-core fast paths (CuHash + NeRFSmall, PE + NeRF) take the scattered points as explicit inputs: cone renders in F16 mode
    stay close to the F32 mode (same draws; the sample set differs where fp16 weights move a random u across a CDF bin)."""
    bbox = api.S.LEGO_BBOX
    for make, chunk, floor in ((api.S.make_hash_scene, 4096, 35.0), (api.S.make_classic_scene, 2048, 35.0)):
        r = make()["renderer"]
        K = api.S.lego_K(24, 24); c2w = api.S.pose_spherical(30.0, -30.0, 4.0)
        outs = {}
        for prec in (api.L.NRF_PREC_F32, api.L.NRF_PREC_F16_MFMA):
            p = api.R.NeRFRenderParams(NSamples=64, NImportance=128, Chunk=chunk, Perturb=1.0, WhiteBkgr=True, Ndc=False, UseViewdirs=True, ThinRay=False,
                                       BoundingBox=bbox, Precision=prec, Seed=11)
            outs[prec] = host(r.Render(24, 24, K, p, c2w=c2w).Outputs.RGBMap)
        assert api.S.psnr(outs[api.L.NRF_PREC_F16_MFMA], outs[api.L.NRF_PREC_F32]) > floor


# ------------------------------------------------------------------ NRF_PREC_F16_SPLIT: matrix cores at fp32-grade accuracy
def test_mlp_small_split_precision_vs_oracle(api, O, manifest):
    """hi + lo fp16 operand pairs (three MFMAs per product): the NeRFSmall output agrees with the fp32 oracle to ~1e-6 of its scale,
    three orders of magnitude tighter than the plain fp16 mode."""
    ent = [x for x in manifest["render_hash"] if "embeddings" not in x[0]]
    blob = synth.blob_from_manifest(ent)
    m = api.M.NeRFSmall(3, 64, 15, 4, 64, False, 3, 64, 32, 16, "model", params=blob)
    rng = np.random.RandomState(3)
    x = np.concatenate([rng.uniform(-1, 1, (3000, 32)), rng.uniform(-1, 1, (3000, 16))], 1).astype(np.float32)
    x[:, :32] = x[:, :32].astype(np.float16).astype(np.float32) * rng.choice([1.0, 1e-2, 1e-4], (3000, 1))     # incl. tiny (freshly initialised) features
    ref = O.mlp_small(blob, x, 32, 16)
    scale = np.abs(ref).max()
    y3 = host(m.forward(dev(x), api.L.NRF_PREC_F16_SPLIT))
    y1 = host(m.forward(dev(x), api.L.NRF_PREC_F16_MFMA))
    e3, e1 = np.abs(y3 - ref).max() / scale, np.abs(y1 - ref).max() / scale
    assert e3 < 3e-6, (e3, e1)
    assert e1 > 50 * e3, "the plain fp16 mode is the loose one"


def test_split_precision_render_matches_parity_mode(api, O):
    """BASELINE config 3 shape, CuHash fast path in NRF_PREC_F16_SPLIT vs the bit-exact NRF_PREC_F32 mode on the adversarial scene.  The default coarse pass
    (sigma net in exact fp32) reproduces the parity mode's sample set, so EVERY pixel value is within 1e-4; with the whole network forced onto the coarse pass
    in split precision (NRF_COARSE_FULL, what round 1 timed) ~1e-6 weight differences move a few samples across CDF plateaus and only the statistical bound holds."""
    sc = api.S.make_hash_scene(mode="cu")
    K = api.S.lego_K(800, 800); c2w = api.S.pose_spherical(30.0, -30.0, 4.0)
    out = {}
    for name, prec, kw in (("f32", api.L.NRF_PREC_F32, {}), ("split", api.L.NRF_PREC_F16_SPLIT, {}), ("split_full", api.L.NRF_PREC_F16_SPLIT, dict(CoarseMode=api.L.NRF_COARSE_FULL)),
                           ("f16", api.L.NRF_PREC_F16_MFMA, {})):
        rp = api.S.lego_render_params(sc["bbox"], chunk=4096, precision=prec, KeepIntermediates=(True if name in ("f32", "split_full") else "depths"), ReturnRaw=True, **kw)
        out[name] = sc["renderer"].Render(800, 800, K, rp, c2w=c2w, row0=396, rows=8)
    a, b, bf, c = (out[k] for k in ("f32", "split", "split_full", "f16"))
    raw_scale = np.abs(host(a.Extras["raw_coarse"])).max()
    assert_close(host(bf.Extras["raw_coarse"]), host(a.Extras["raw_coarse"]), rtol=0, atol=3e-6 * raw_scale, what="coarse raw, same points")
    rgb_a, rgb_b = host(a.Outputs.RGBMap).reshape(-1, 3), host(b.Outputs.RGBMap).reshape(-1, 3)
    assert_exact(host(b.Extras["z_fine"]), host(a.Extras["z_fine"]), "default coarse pass: the parity mode's sample set")
    d = np.abs(rgb_b - rgb_a)
    assert d.max() < 1e-4 and np.median(d) < 1e-5, (d.max(), np.median(d))                      # strict: north_star's pixel bar
    assert np.abs(host(b.Raw) - host(a.Raw)).max() < 1e-5 * np.abs(host(a.Raw)).max()           # fine raw on identical points: 22-bit operands
    df = np.abs(host(bf.Outputs.RGBMap).reshape(-1, 3) - rgb_a)
    assert (df < 1e-4).mean() > 0.98 and np.median(df) < 1e-5 and df.max() < 2e-2, ((df < 1e-4).mean(), np.median(df), df.max())
    ps_split, ps_f16 = api.S.psnr(rgb_b, rgb_a), api.S.psnr(host(c.Outputs.RGBMap).reshape(-1, 3), rgb_a)
    assert ps_split > 95 and ps_split > ps_f16 + 20, (ps_split, ps_f16)


@pytest.mark.parametrize("mode", ["cu", "ngp"])
def test_exact_coarse_sigma_pass_reproduces_the_parity_sample_set(api, mode):
    """The timed precision (NRF_PREC_F16_SPLIT, coarse pass = sigma net alone in exact fp32 on the matrix cores, sigma_small_f32.hip) against
    the bit-exact NRF_PREC_F32 mode on a 16-row tile of the 800x800 frame (12 800 rays, 3.3 M network evaluations):
    coarse weights and the fine sample set z_fine are IDENTICAL (bit for bit), and every pixel value is within the north star's 1e-4 --
    strictly, not for a fraction of them."""
    sc = api.S.make_hash_scene(mode=mode)
    K = api.S.lego_K(800, 800); c2w = api.S.pose_spherical(30.0, -30.0, 4.0)
    def render(prec, keep, **kw):
        rp = api.S.lego_render_params(sc["bbox"], chunk=4096, precision=prec, KeepIntermediates=keep, **kw)
        return sc["renderer"].Render(800, 800, K, rp, c2w=c2w, row0=392, rows=16)
    a = render(api.L.NRF_PREC_F32, True)
    b = render(api.L.NRF_PREC_F16_SPLIT, "depths")
    assert "raw_coarse" not in b.Extras
    assert_exact(host(b.Extras["z_coarse"]), host(a.Extras["z_coarse"]), "z_coarse")
    assert_exact(host(b.Extras["weights_coarse"]), host(a.Extras["weights_coarse"]), "coarse weights: fp32 MFMA sigma == NRF_PREC_F32")
    assert_exact(host(b.Extras["z_fine"]), host(a.Extras["z_fine"]), "fine sample set")
    rgb_a, rgb_b = host(a.Outputs.RGBMap).reshape(-1, 3), host(b.Outputs.RGBMap).reshape(-1, 3)
    d = np.abs(rgb_b - rgb_a)
    assert d.max() < 1e-4 and np.median(d) < 1e-5, (d.max(), np.median(d))
    for k in ("DepthMap", "AccMap"):
        dd = np.abs(host(getattr(b.Outputs, k)).reshape(-1) - host(getattr(a.Outputs, k)).reshape(-1))
        assert dd.max() < 1e-4, (k, dd.max())
    # the plain fp16 mode can ask for the same coarse pass
    c = render(api.L.NRF_PREC_F16_MFMA, "depths", CoarseMode=api.L.NRF_COARSE_SIGMA_F32)
    assert_exact(host(c.Extras["z_fine"]), host(a.Extras["z_fine"]), "fine sample set, fp16 fine pass")
    # NRF_COARSE_FULL is the whole network in the chosen precision (what a caller asking for raw_coarse gets): close, not identical
    e = render(api.L.NRF_PREC_F16_SPLIT, "depths", CoarseMode=api.L.NRF_COARSE_FULL)
    we, wa = host(e.Extras["weights_coarse"]), host(a.Extras["weights_coarse"])
    assert np.abs(we - wa).max() < 1e-4 and (we != wa).any()
    # stochastic branches (jitter + SamplePDF(det=false), cone rays, sigma noise, preconditioning) go through the same coarse pass
    kw = dict(Perturb=1.0, RawNoiseStd=0.5, ThinRay=False, StochasticPreconditioningAlpha=0.01, Seed=77)
    sa = render(api.L.NRF_PREC_F32, True, **kw)
    sb = render(api.L.NRF_PREC_F16_SPLIT, "depths", **kw)
    assert_exact(host(sb.Extras["weights_coarse"]), host(sa.Extras["weights_coarse"]), "stochastic: coarse weights")
    assert_exact(host(sb.Extras["z_fine"]), host(sa.Extras["z_fine"]), "stochastic: fine sample set")


def test_sigma_f32_kernel_shapes_and_ragged_sizes(api):
    """sigma_small_f32.hip over every built shape (2 or 3 sigma layers; fp16 / fp32 features) and ragged point counts (1 ray, a non-multiple of the
    512-point block, one block + 1): coarse weights == NRF_PREC_F32, bit for bit."""
    for mode, nl in (("cu", 3), ("cu", 2), ("ngp", 2), ("ngp", 3)):
        sc = api.S.make_hash_scene(mode=mode, log2_t=14, num_layers=nl)
        K = api.S.lego_K(40, 40); c2w = api.S.pose_spherical(10.0, -30.0, 4.0)
        for rows, cols, ns in ((1, 1, 64), (3, 7, 64), (1, 9, 57), (5, 40, 64)):
            out = {}
            for prec in (api.L.NRF_PREC_F32, api.L.NRF_PREC_F16_SPLIT):
                rp = api.S.lego_render_params(sc["bbox"], ns, 32, 4096, prec, KeepIntermediates="depths" if prec else True)
                o, d, _ = api.R.GetRays(40, 40, K, c2w, row0=17, rows=rows)
                out[prec] = sc["renderer"].Render(0, 0, None, rp, rays=(o.reshape(-1, 3)[:rows * cols].contiguous(), d.reshape(-1, 3)[:rows * cols].contiguous(), None))
            a, b = out[api.L.NRF_PREC_F32], out[api.L.NRF_PREC_F16_SPLIT]
            assert host(a.Extras["weights_coarse"]).max() > 0
            assert_exact(host(b.Extras["weights_coarse"]), host(a.Extras["weights_coarse"]), f"{mode} nl={nl} n={rows * cols} s={ns}")
            assert_exact(host(b.Extras["z_fine"]), host(a.Extras["z_fine"]), f"{mode} nl={nl} n={rows * cols} s={ns} z_fine")


def test_image_post_bit_exact_vs_reference(api, O):
    """N4: the 8-bit buffers RenderPath hands to cv::imwrite (NeRFExecutor.h:690-700)."""
    g = load_golden("post")
    dn = api.R.NormalizeDepth(dev(g["depth"]), float(g["near_far"][0]), float(g["near_far"][1]))
    assert_exact(host(dn), g["depth_norm"])
    for k in ("rgb", "disp", "edge"):
        assert_exact(host(api.R.TorchTensorToCVMat(dev(g[k]))), g[k + "_u8"], k)
    assert_exact(host(api.R.TorchTensorToCVMat(dn)), g["depth_u8"])
    big = np.random.RandomState(0).uniform(-0.2, 1.3, 1000003).astype(np.float32)         # ragged length, unaligned tail
    assert_exact(host(api.R.TorchTensorToCVMat(dev(big))), O.to_u8(big))


# ------------------------------------------------------------------ N1: training step (backward + huber + Adam)
def _train_golden(api, manifest):
    g = load_golden("train_hash")
    ent = manifest["train_hash"]
    table = synth.blob_from_manifest([e for e in ent if "embeddings" in e[0]])
    blob = synth.blob_from_manifest([e for e in ent if "embeddings" not in e[0]])
    e = api.M.HashEmbedder("embedder", g["bbox"], 4, 2, 12, 16, 128)
    m = api.M.NeRFSmall(3, 64, 15, 3, 64, False, 3, 64, 8, 16, "model", params=blob)
    return g, table, blob, e, api.M.SHEncoder("embeddirs", 3, 4), m


def _mlp_names():
    return ["sigma_net_0", "sigma_net_1", "sigma_net_2", "color_net_0", "color_net_1", "color_net_2"]


def test_training_backward_stages_vs_reference_autograd(api, O, manifest):
    import ctypes as C
    P = lambda t: C.c_void_p(t.data_ptr())
    g, table, blob, e, ed, m = _train_golden(api, manifest)
    e.set_table(table)
    lib = api.L.lib()
    # huber / mse and d huber / d rgb
    rgb, tgt = dev(g["s1_rgb"]), dev(g["target"])
    lm = torch.empty(2, device="cuda"); g_rgb = torch.empty_like(rgb)
    api.L.check(lib.nrf_huber_loss(P(rgb), P(tgt), C.c_int64(rgb.numel()), P(lm), P(g_rgb), None))
    assert abs(host(lm)[0] - g["s1_loss"][0]) < 2e-7 and abs(host(lm)[1] - g["s1_mse"][0]) < 2e-7
    ol, om, og = O.huber_loss(g["s1_rgb"], g["target"])
    assert_exact(host(g_rgb), og, "d huber / d rgb == oracle")
    # RawToOutputs backward on the reference's fine raw / z
    rays = O.pack_rays(g["rays_o"], g["rays_d"], g["bbox"])
    raw, z, d = dev(g["s1_fine_raw"]), dev(g["s1_fine_z"]), dev(rays[:, 3:6])
    g_raw = torch.empty_like(raw)
    api.L.check(lib.nrf_raw2outputs_backward(P(raw), P(z), P(d), 3, C.c_int64(64), 64, 4, 0, P(g_rgb), P(g_raw), None))
    ref = g["s1_grad_fine_raw"]
    assert_close(host(g_raw), ref, rtol=2e-4, atol=1e-5 * np.abs(ref).max(), what="RawToOutputs backward vs autograd")
    assert_close(host(g_raw), O.raw2outputs_backward(g["s1_fine_raw"], g["s1_fine_z"], rays[:, 3:6], og), rtol=1e-5, atol=1e-7 * np.abs(ref).max(), what="vs oracle")
    # network backward on the reference's points
    pts = dev(g["s1_fine_pts"].reshape(-1, 3))
    emb, keep = e.forward(pts)
    dirs, _ = ed.forward(dev(rays[:, 8:11]))
    x = torch.cat([emb, dirs[:, None, :].expand(64, 64, 16).reshape(4096, 16)], 1).contiguous()
    gr = dev(ref.reshape(-1, 4).copy())
    ku8 = keep.to(torch.uint8)
    api.L.check(lib.nrf_mask_sigma_grad(P(ku8), C.c_int64(4096), 4, P(gr), None))
    g_blob = torch.zeros(blob.size, device="cuda"); g_x = torch.empty((4096, 8), device="cuda")
    nb = lib.nrf_mlp_backward_workspace_bytes(m._m, C.c_int64(4096))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    api.L.check(lib.nrf_mlp_backward(m._m, P(x), P(gr), C.c_int64(4096), P(g_blob), P(g_x), P(ws), C.c_size_t(nb), None))
    refb = np.concatenate([g[f"s1_grad_model_{n}.weight"].reshape(-1) for n in _mlp_names()])
    assert_close(host(g_blob), refb, rtol=1e-3, atol=2e-5 * np.abs(refb).max(), what="NeRFSmall weight gradients vs autograd")
    gp_o, gx_o = O.mlp_small_backward(blob, host(x), host(gr), 8, 16, 3, 64, 15, 3, 64)
    assert_close(host(g_x), gx_o, rtol=1e-4, atol=1e-6 * np.abs(gx_o).max(), what="d loss / d features vs oracle")
    g_table = torch.zeros(table.size, device="cuda")
    api.L.check(lib.nrf_hash_backward(e._h, P(pts), C.c_int64(4096), P(g_x), P(g_table), None))
    reft = np.stack([g[f"s1_grad_embedder_embeddings_{l}.weight"] for l in range(4)]).reshape(-1)
    assert_close(host(g_table), reft, rtol=1e-3, atol=2e-5 * np.abs(reft).max(), what="hash table gradients vs autograd")
    # Adam on the reference's gradients -> the reference's parameters after step 1
    p = dev(blob.copy()); mm = torch.zeros_like(p); vv = torch.zeros_like(p); gg = dev(refb)
    api.L.check(lib.nrf_adam_step(P(p), P(gg), P(mm), P(vv), C.c_int64(p.numel()), C.c_float(float(g["lr"][0])), C.c_float(0.9), C.c_float(0.99), C.c_float(1e-15), 1, None))
    ref1 = np.concatenate([g[f"s1_param_model_{n}.weight"].reshape(-1) for n in _mlp_names()])
    assert_close(host(p), ref1, rtol=0, atol=2e-7, what="Adam step 1")


def _small_backward_both(api, nl, nlc, blob, x_h, gr_h):
    import ctypes as C
    P = lambda t: C.c_void_p(t.data_ptr())
    p = x_h.shape[0]
    m = api.M.NeRFSmall(nl, 64, 15, nlc, 64, False, 3, 64, 32, 16, "model", params=blob)
    x, gr = dev(x_h), dev(gr_h)
    lib = api.L.lib()
    out = {}
    for name, fn, wsfn in (("f32", lib.nrf_mlp_backward, lib.nrf_mlp_backward_workspace_bytes), ("f16", lib.nrf_mlp_backward_f16, lib.nrf_mlp_backward_f16_workspace_bytes)):
        nb = wsfn(m._m, C.c_int64(p))
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        g_blob = torch.zeros(blob.size, device="cuda"); g_x = torch.zeros((p, 32), device="cuda")
        api.L.check(fn(m._m, P(x), P(gr), C.c_int64(p), P(g_blob), P(g_x), P(ws), C.c_size_t(nb), None))
        torch.cuda.synchronize()
        out[name] = (host(g_blob), host(g_x))
    return out["f32"], out["f16"]


def _small_dims(nl, nlc):
    return [(32, 64)] + [(64, 64)] * (nl - 2) + [(64, 16)] + [(31, 64)] + [(64, 64)] * (nlc - 2) + [(64, 3)]


@pytest.mark.parametrize("nl,nlc,p", [(3, 4, 1000), (3, 3, 333), (2, 4, 128), (2, 3, 4100)])
def test_mlp_backward_matrix_core_exact_on_integer_network(api, nl, nlc, p):
    """nrf_mlp_backward_f16 (one fused MFMA kernel: forward, gradient chain through W^T images, weight gradients through MFMA transposition)
    against the fp32 backward, which test_training_backward_stages_vs_reference_autograd pins to the reference's autograd.  Sparse -1/0/+1
    weights and small-integer inputs / output gradients: every activation and every chained gradient is an integer fp16 holds exactly
    (checked below in float64), no pre-activation sits next to the ReLU kink, so the two paths may differ by fp32 summation order only --
    any wrong fragment index, mask bit or blob offset shows up at full size."""
    rng = np.random.default_rng(100 * nl + nlc)
    dims = _small_dims(nl, nlc)
    mats = []
    for (i, o) in dims:
        w = np.zeros((o, i), np.float32)
        nz = rng.random((o, i)) < 3.0 / i
        w[nz] = rng.choice([-1.0, 1.0], size=int(nz.sum()))
        mats.append(w)
    blob = np.concatenate([w.reshape(-1) for w in mats])
    x = np.concatenate([rng.integers(-2, 3, (p, 32)), rng.integers(-1, 2, (p, 16))], 1).astype(np.float32)
    gk = rng.integers(-2, 3, (p, 4)).astype(np.float64)
    gk[0, 0] = 2.0                                              # the device picks the loss scale from max |g_out|
    gr = (gk * 2.0 ** -22).astype(np.float32)
    # float64 model of the pass: every value the kernel rounds to fp16 must be an integer below 2048 (in units of the scaled gradient)
    h, acts = x[:, :32].astype(np.float64), []
    for l in range(nl):
        acts.append(h); h = h @ mats[l].T.astype(np.float64)
        if l < nl - 1: h = np.maximum(h, 0)
    sig = h
    c = np.concatenate([x[:, 32:].astype(np.float64), sig[:, 1:]], 1)
    for l in range(nlc - 1):
        acts.append(c); c = np.maximum(c @ mats[nl + l].T.astype(np.float64), 0)
    acts.append(c)
    assert max(np.abs(a).max() for a in acts) < 2048 and np.abs(sig).max() < 2048
    g = gk[:, :3] @ mats[-1].astype(np.float64); gmax = 0.0
    for l in range(nlc - 1, 0, -1):
        g = g * (acts[nl + l] > 0); gmax = max(gmax, np.abs(g).max()); g = g @ mats[nl + l - 1].astype(np.float64)
    g = np.concatenate([gk[:, 3:4], g[:, 16:]], 1)
    for l in range(nl - 1, 0, -1):
        gmax = max(gmax, np.abs(g).max()); g = (g @ mats[l].astype(np.float64)) * (acts[l] > 0)
    assert max(gmax, np.abs(g).max()) < 256                     # x 8 (the loss scale puts max |g_out| = 2 at 16) < 2048
    (gb32, gx32), (gb16, gx16) = _small_backward_both(api, nl, nlc, blob, x, gr)
    off = 0
    for li, (i, o) in enumerate(dims):
        a, b = gb16[off:off + i * o], gb32[off:off + i * o]
        assert np.abs(b).max() > 0
        assert_close(a, b, rtol=1e-5, atol=1e-6 * np.abs(b).max(), what=f"dW of layer {li}")
        off += i * o
    assert_close(gx16, gx32, rtol=1e-5, atol=1e-6 * np.abs(gx32).max(), what="d loss / d features")
    assert np.abs(gx32).max() > 0


def test_mlp_backward_matrix_core_level_major_input(api):
    """nrf_mlp_backward_f16_lm (level-major fp16 hash features of nrf_hash_encode_lm_f16 + one fp16 direction row per ray) against nrf_mlp_backward_f16 on the
    [p, 48] fp32 rows built from the same encoders: the operand fragments are the same fp16 values, so the gradients agree to summation order.
    p is not a multiple of the kernel's 128-point block and s does not divide it."""
    import ctypes as C
    P = lambda t: C.c_void_p(t.data_ptr())
    sc = api.S.make_hash_scene(mode="cu", log2_t=14, seed=31, table_amp=0.4)
    e, ed, m = sc["embedder"], sc["embeddirs"], sc["mlp"]
    rng = np.random.default_rng(8)
    n, s = 37, 24
    p = n * s
    bb = api.S.LEGO_BBOX
    pts = dev(rng.uniform(bb[:3] - 0.1, bb[3:] + 0.1, (p, 3)).astype(np.float32))            # a few outside the box (keep == false)
    vd = rng.standard_normal((n, 3)); vd /= np.linalg.norm(vd, axis=1, keepdims=True)
    dirs, _ = ed.forward(dev(vd.astype(np.float32)))
    emb, keep = e.forward(pts)
    x = torch.cat([emb, dirs[:, None, :].expand(n, s, 16).reshape(p, 16)], 1).contiguous()
    gr = dev((rng.standard_normal((p, 4)) * 1e-4).astype(np.float32))
    lib = api.L.lib()
    feats = torch.empty((16, p, 2), device="cuda", dtype=torch.float16); k8 = torch.empty((p,), device="cuda", dtype=torch.uint8)
    api.L.check(lib.nrf_hash_encode_lm_f16(e._h, P(pts), C.c_int64(p), P(feats), P(k8), None))
    assert_exact(host(feats).astype(np.float32).transpose(1, 0, 2).reshape(p, 32), host(emb), "level-major fp16 features == CuHashEmbedder.forward")
    assert_exact(host(k8).astype(bool), host(keep), "keep mask")
    assert (~host(keep)).sum() > 0
    d16 = dirs.to(torch.float16).contiguous()
    nb = lib.nrf_mlp_backward_f16_workspace_bytes(m._m, C.c_int64(p)); ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    ga = torch.zeros(m.n_params, device="cuda"); gxa = torch.zeros((p, 32), device="cuda")
    gb = torch.zeros(m.n_params, device="cuda"); gxb = torch.zeros((p, 32), device="cuda")
    api.L.check(lib.nrf_mlp_backward_f16(m._m, P(x), P(gr), C.c_int64(p), P(ga), P(gxa), P(ws), C.c_size_t(nb), None))
    api.L.check(lib.nrf_mlp_backward_f16_lm(m._m, P(feats), P(d16), s, P(gr), C.c_int64(p), P(gb), P(gxb), P(ws), C.c_size_t(nb), None))
    assert float(ga.abs().max()) > 0
    assert_exact(host(gxb), host(gxa), "d loss / d features: level-major input == row input")
    assert_close(host(gb), host(ga), rtol=1e-5, atol=1e-6 * float(ga.abs().max()), what="weight gradients (LDS float-atomic order only)")


@pytest.mark.parametrize("nl,nlc", [(3, 4), (2, 3)])
def test_mlp_set_params_on_the_device_equals_a_freshly_packed_handle(api, nl, nlc):
    """nrf_mlp_set_params of a NeRFSmall handle refreshes the blob and every derived image (fp16 / split / sigma-fp32 + geo / backward fragments, transposed fp32
    layers) ON THE DEVICE from gather maps decoded out of the host packers (mlp.hip build_weight_maps).  A handle created with blob A and moved to blob B must be
    indistinguishable, bit for bit, from one created with B: all forward precisions, both backward chains, and a rendered frame (exact coarse sigma pass + geo
    hand-over) after going A -> garbage -> A.  Reference: the optimizer step of NeRFExecutor::Train (NeRFExecutor.h:653-770) changes every weight each iteration."""
    import ctypes as C
    P = lambda t: C.c_void_p(t.data_ptr())
    lib = api.L.lib()
    a = api.S.make_hash_scene(mode="cu", log2_t=14, seed=77, num_layers=nl, num_layers_color=nlc)
    b = api.S.make_hash_scene(mode="cu", log2_t=14, seed=78, num_layers=nl, num_layers_color=nlc)
    ma, mb = a["mlp"], b["mlp"]
    assert lib.nrf_mlp_device_repack_images(ma._m) >= 5 + nl + nlc, "the packers' layouts must decode into gather maps (else set_params silently takes the host path)"
    rng = np.random.default_rng(5)
    p = 1000
    x = dev(rng.uniform(-1, 1, (p, 48)).astype(np.float32))
    gr = dev((rng.standard_normal((p, 4)) * 1e-3).astype(np.float32))
    K = api.S.lego_K(40, 40); c2w = api.S.pose_spherical(30.0, -30.0, 4.0)
    rp = api.S.lego_render_params(a["bbox"], 16, 32, 4096, api.L.NRF_PREC_F16_SPLIT)
    frame_a = host(a["renderer"].Render(40, 40, K, rp, c2w=c2w).Outputs.RGBMap)

    blob_b = dev(b["mlp_blob"])
    api.L.check(lib.nrf_mlp_set_params(ma._m, P(blob_b), 1, None))                      # device source
    for prec, name in ((api.L.NRF_PREC_F32, "fp32"), (api.L.NRF_PREC_F16_MFMA, "fp16"), (api.L.NRF_PREC_F16_SPLIT, "split")):
        assert_exact(host(ma.forward(x, prec)), host(mb.forward(x, prec)), f"forward {name}: updated handle == fresh handle")
    for entry, wsb in ((lib.nrf_mlp_backward, lib.nrf_mlp_backward_workspace_bytes), (lib.nrf_mlp_backward_f16, lib.nrf_mlp_backward_f16_workspace_bytes)):
        res = []
        for m in (ma, mb):
            nb = wsb(m._m, C.c_int64(p)); ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
            g = torch.zeros(m.n_params, device="cuda"); gx = torch.zeros((p, 32), device="cuda")
            api.L.check(entry(m._m, P(x), P(gr), C.c_int64(p), P(g), P(gx), P(ws), C.c_size_t(nb), None))
            res.append((host(g), host(gx)))
        assert np.abs(res[1][1]).max() > 0
        assert_exact(res[0][1], res[1][1], "d loss / d features: updated handle == fresh handle")
        assert_close(res[0][0], res[1][0], rtol=1e-5, atol=1e-6 * np.abs(res[1][0]).max(), what="weight gradients (float-atomic order only)")

    frame_b = host(a["renderer"].Render(40, 40, K, rp, c2w=c2w).Outputs.RGBMap)
    assert np.abs(frame_b - frame_a).max() > 1e-3                                       # the frame really depends on the weights
    api.L.check(lib.nrf_mlp_set_params(ma._m, C.c_void_p(a["mlp_blob"].ctypes.data), 0, None))      # host source
    assert_exact(host(a["renderer"].Render(40, 40, K, rp, c2w=c2w).Outputs.RGBMap), frame_a, "frame after A -> B -> A")


def test_mlp_backward_matrix_core_edges(api):
    """Boundary behaviour of nrf_mlp_backward_f16: empty batch, optional d_g_x, all-zero output gradient (loss scale of nothing), accumulation into a
    non-zero gradient blob, a workspace that is too small, a NeRFSmall shape outside the built family, more points than one 2^22-point pass."""
    import ctypes as C
    P = lambda t: C.c_void_p(t.data_ptr())
    rng = np.random.default_rng(3)
    dims = _small_dims(3, 4)
    blob = (rng.standard_normal(sum(i * o for i, o in dims)) * 0.2).astype(np.float32)
    m = api.M.NeRFSmall(3, 64, 15, 4, 64, False, 3, 64, 32, 16, "model", params=blob)
    lib = api.L.lib()
    p = 777
    x = dev(rng.uniform(-1, 1, (p, 48)).astype(np.float32)); gr = dev((rng.standard_normal((p, 4)) * 1e-3).astype(np.float32))
    nb = lib.nrf_mlp_backward_f16_workspace_bytes(m._m, C.c_int64(p))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    g0 = torch.zeros(blob.size, device="cuda"); gx = torch.zeros((p, 32), device="cuda")
    api.L.check(lib.nrf_mlp_backward_f16(m._m, P(x), P(gr), C.c_int64(0), P(g0), P(gx), P(ws), C.c_size_t(nb), None))          # p = 0
    assert float(g0.abs().max()) == 0.0
    api.L.check(lib.nrf_mlp_backward_f16(m._m, P(x), P(gr), C.c_int64(p), P(g0), P(gx), P(ws), C.c_size_t(nb), None))
    g1 = torch.full((blob.size,), 0.5, device="cuda")
    api.L.check(lib.nrf_mlp_backward_f16(m._m, P(x), P(gr), C.c_int64(p), P(g1), None, P(ws), C.c_size_t(nb), None))            # no d_g_x; accumulates
    assert_close(host(g1) - 0.5, host(g0), rtol=1e-4, atol=1e-6 * float(g0.abs().max()), what="accumulation into a non-zero blob")
    # overflow report (nrf_mlp_backward_f16_flags): clean after a normal call; an inf / NaN in the incoming gradient or a non-finite accumulated gradient is flagged
    fl = (C.c_uint32 * 2)()
    api.L.check(lib.nrf_mlp_backward_f16_flags(P(ws), fl, None))
    assert (fl[0], fl[1]) == (0, 0)
    gr_bad = gr.clone(); gr_bad[5, 2] = float("inf"); gr_bad[9, 0] = float("nan")
    g2 = torch.zeros(blob.size, device="cuda")
    api.L.check(lib.nrf_mlp_backward_f16(m._m, P(x), P(gr_bad), C.c_int64(p), P(g2), None, P(ws), C.c_size_t(nb), None))
    api.L.check(lib.nrf_mlp_backward_f16_flags(P(ws), fl, None))
    assert fl[0] == 1 and fl[1] == 1, (fl[0], fl[1])
    g3 = torch.zeros(blob.size, device="cuda"); g3[7] = float("inf")                         # a poisoned accumulator is reported too
    api.L.check(lib.nrf_mlp_backward_f16(m._m, P(x), P(gr), C.c_int64(p), P(g3), None, P(ws), C.c_size_t(nb), None))
    api.L.check(lib.nrf_mlp_backward_f16_flags(P(ws), fl, None))
    assert fl[0] == 0 and fl[1] == 1
    gz = torch.zeros_like(gr); g2 = torch.zeros(blob.size, device="cuda"); gx2 = torch.ones((p, 32), device="cuda")
    api.L.check(lib.nrf_mlp_backward_f16(m._m, P(x), P(gz), C.c_int64(p), P(g2), P(gx2), P(ws), C.c_size_t(nb), None))          # zero gradient in
    assert float(g2.abs().max()) == 0.0 and float(gx2.abs().max()) == 0.0
    with pytest.raises(api.L.NrfError):
        api.L.check(lib.nrf_mlp_backward_f16(m._m, P(x), P(gr), C.c_int64(p), P(g0), P(gx), P(ws), C.c_size_t(1024), None))
    m8 = api.M.NeRFSmall(3, 64, 15, 3, 64, False, 3, 64, 8, 16, "model", params=(rng.standard_normal(8 * 64 + 64 * 64 + 64 * 16 + 31 * 64 + 64 * 64 + 64 * 3) * 0.1).astype(np.float32))
    x8 = torch.zeros((p, 24), device="cuda")
    with pytest.raises(api.L.NrfError):
        api.L.check(lib.nrf_mlp_backward_f16(m8._m, P(x8), P(gr), C.c_int64(p), P(g0), P(gx), P(ws), C.c_size_t(nb), None))
    # two passes (2^22 points each): the second pass's points must land in the same gradient
    pbig = (1 << 22) + 1000
    xb = x[:1].expand(pbig, 48).contiguous(); gb = gr[:1].expand(pbig, 4).contiguous()
    nbb = lib.nrf_mlp_backward_f16_workspace_bytes(m._m, C.c_int64(pbig))
    wsb = torch.empty(nbb, dtype=torch.uint8, device="cuda")
    g3 = torch.zeros(blob.size, device="cuda"); g4 = torch.zeros(blob.size, device="cuda")
    api.L.check(lib.nrf_mlp_backward_f16(m._m, P(xb), P(gb), C.c_int64(pbig), P(g3), None, P(wsb), C.c_size_t(nbb), None))
    api.L.check(lib.nrf_mlp_backward_f16(m._m, P(xb), P(gb), C.c_int64(1000), P(g4), None, P(wsb), C.c_size_t(nbb), None))
    assert_close(host(g3), host(g4) * (pbig / 1000.0), rtol=2e-3, atol=1e-5 * float(g3.abs().max()), what="identical points: gradient scales with their count")


@pytest.mark.parametrize("nl,nlc,p", [(3, 4, 50000), (3, 3, 20001)])
def test_mlp_backward_matrix_core_vs_fp32_random_network(api, nl, nlc, p):
    """Same comparison on a dense random network.  The fused kernel's own forward is fp16, so a pre-activation within ~1e-3 of zero can land on
    the other side of the ReLU than in the fp32 pass and that point's gradient through that neuron flips on/off: a handful of points differ at
    full size, everything else by fp16 rounding.  With this test's random-SIGN output gradients signal and flip noise both grow as sqrt(points)
    (relative error ~ sqrt(share of flipped units), ~1 %); a training batch's coherent gradient grows as `points`.  Hence statistical bounds."""
    rng = np.random.default_rng(nl * 10 + nlc)
    dims = _small_dims(nl, nlc)
    blob = (rng.standard_normal(sum(i * o for i, o in dims)) * 0.18).astype(np.float32)
    x = rng.uniform(-1, 1, (p, 48)).astype(np.float32)
    gr = (rng.standard_normal((p, 4)) * 3e-6).astype(np.float32)
    gr[rng.random(p) < 0.2, 3] = 0.0                        # masked sigma gradients (keep == false)
    (gb32, gx32), (gb16, gx16) = _small_backward_both(api, nl, nlc, blob, x, gr)
    assert np.isfinite(gb16).all() and np.isfinite(gx16).all()
    off = 0
    for li, (i, o) in enumerate(dims):
        a, b = gb16[off:off + i * o], gb32[off:off + i * o]
        scale = np.abs(b).max()
        assert np.corrcoef(a, b)[0, 1] > 0.998, (li, np.corrcoef(a, b)[0, 1])
        assert np.sqrt(np.mean((a - b) ** 2)) < 2e-2 * scale, (li, np.sqrt(np.mean((a - b) ** 2)) / scale)
        assert np.abs(a - b).max() < 0.12 * scale, (li, np.abs(a - b).max() / scale)
        off += i * o
    sx = np.abs(gx32).max()
    row_err = np.abs(gx16 - gx32).max(1) / sx
    assert np.median(row_err) < 2e-3, np.median(row_err)
    assert np.mean(row_err > 2e-2) < 0.05, np.mean(row_err > 2e-2)
    assert np.sqrt(np.mean((gx16 - gx32) ** 2)) < 1e-2 * sx


def test_trainer_two_steps_vs_reference(api, manifest):
    from nerfpp_amd.train import Trainer
    g, table, blob, e, ed, m = _train_golden(api, manifest)
    lr = float(g["lr"][0])
    tr = Trainer(e, ed, m, table, blob, learning_rate=lr)
    rp = api.R.NeRFRenderParams(NSamples=32, NImportance=32, Chunk=64, Perturb=0.0, WhiteBkgr=False, Ndc=False, UseViewdirs=True, ThinRay=True,
                                BoundingBox=g["bbox"], Precision=api.L.NRF_PREC_F32)
    o, d, tgt = dev(g["rays_o"]), dev(g["rays_d"]), dev(g["target"])
    lm1, _ = tr.step(o, d, tgt, rp)
    # end to end the loss inherits the render's own distance to the reference (a few fine samples in other CDF bins, 64 rays only)
    assert abs(host(lm1)[0] - g["s1_loss"][0]) < 2e-4 and abs(host(lm1)[1] - g["s1_mse"][0]) < 4e-4, (host(lm1), g["s1_loss"], g["s1_mse"])
    ref1 = np.concatenate([g[f"s1_param_model_{n}.weight"].reshape(-1) for n in _mlp_names()])
    # Adam's first step is lr * sign(g) (m/sqrt(v) = g/|g|, eps 1e-15): a weight whose gradient is rounding-level noise moves by +-lr either
    # way, so the comparison bounds the SHARE of such weights, not their distance
    d1 = np.abs(host(tr.blob) - ref1) / lr
    assert d1.mean() < 0.02 and (d1 > 0.05).mean() < 0.03, (d1.mean(), (d1 > 0.05).mean())
    # second step from the REFERENCE's state after step 1 (its parameters; moments rebuilt from its step-1 gradients), so that the
    # comparison is not dominated by the sign-descent noise of step 1
    g1b = np.concatenate([g[f"s1_grad_model_{n}.weight"].reshape(-1) for n in _mlp_names()])
    g1t = np.stack([g[f"s1_grad_embedder_embeddings_{l}.weight"] for l in range(4)]).reshape(-1)
    tr.blob.copy_(dev(ref1)); tr.table.copy_(dev(np.stack([g[f"s1_param_embedder_embeddings_{l}.weight"] for l in range(4)]).reshape(-1)))
    tr.m_blob.copy_(dev(0.1 * g1b)); tr.v_blob.copy_(dev(np.float32(0.01) * g1b * g1b))
    tr.m_table.copy_(dev(0.1 * g1t)); tr.v_table.copy_(dev(np.float32(0.01) * g1t * g1t))
    tr._push_params()
    lm2, _ = tr.step(o, d, tgt, rp)
    assert abs(host(lm2)[0] - g["s2_loss"][0]) < 2e-4, (host(lm2), g["s2_loss"])
    ref2 = np.concatenate([g[f"s2_param_model_{n}.weight"].reshape(-1) for n in _mlp_names()])
    d2 = np.abs(host(tr.blob) - ref2) / lr
    assert d2.mean() < 5e-3 and (d2 > 0.05).mean() < 0.03, (d2.mean(), (d2 > 0.05).mean())
    reft2 = np.stack([g[f"s2_param_embedder_embeddings_{l}.weight"] for l in range(4)]).reshape(-1)
    dt = np.abs(host(tr.table) - reft2) / lr
    assert dt.mean() < 8e-3 and (dt > 0.05).mean() < 0.05, (dt.mean(), (dt > 0.05).mean())


def test_trainer_two_steps_vs_reference_classic_model(api, manifest):
    """The same loop body on the classic configuration -- Embedder(10) / Embedder(4) / NeRFImpl with a skip and the view-direction head (a legal TNeRF of NeRFExecutor::Train):
    Trainer (fused render in NRF_PREC_F32 -> huber -> RawToOutputs backward -> nrf_mlp_backward on NeRFImpl -> Adam) against the reference's CPU autograd over the compiled
    NeRF.cpp, golden train_classic: loss and mse of both steps, the step-1 gradient of every parameter, and the parameters after the steps at the sign-descent bounds of
    test_trainer_two_steps_vs_reference."""
    from nerfpp_amd.train import Trainer
    g = load_golden("train_classic")
    ent = manifest["train_classic"]
    blob = synth.blob_from_manifest(ent)
    e, ed = api.M.Embedder("embedder", 10), api.M.Embedder("embeddirs", 4)
    m = api.M.NeRF(4, 64, 63, 27, 5, {1}, True, "model", params=blob)
    lr = float(g["lr"][0])
    tr = Trainer(e, ed, m, None, blob, learning_rate=lr)
    rp = api.R.NeRFRenderParams(NSamples=16, NImportance=16, Chunk=64, Perturb=0.0, WhiteBkgr=False, Ndc=False, UseViewdirs=True, ThinRay=True,
                                BoundingBox=g["bbox"], Precision=api.L.NRF_PREC_F32)
    o, d, tgt = dev(g["rays_o"]), dev(g["rays_d"]), dev(g["target"])
    names = [n for n, _, _, _ in ent]
    lm1, _ = tr.step(o, d, tgt, rp)
    assert abs(host(lm1)[0] - g["s1_loss"][0]) < 2e-4 and abs(host(lm1)[1] - g["s1_mse"][0]) < 4e-4, (host(lm1), g["s1_loss"], g["s1_mse"])
    g1 = np.concatenate([g["s1_grad_" + n].reshape(-1) for n in names])
    got = host(tr.g_blob)
    # the few rays whose fine sample set differs from the CPU render's contribute their whole difference: a norm-wise bound
    assert np.linalg.norm(got - g1) < 0.05 * np.linalg.norm(g1), (np.linalg.norm(got - g1), np.linalg.norm(g1))
    ref1 = np.concatenate([g["s1_param_" + n].reshape(-1) for n in names])
    d1 = np.abs(host(tr.blob) - ref1) / lr
    assert d1.mean() < 0.03 and (d1 > 0.05).mean() < 0.04, (d1.mean(), (d1 > 0.05).mean())
    # second step from the REFERENCE's state after step 1 (its parameters; moments rebuilt from its step-1 gradients)
    tr.blob.copy_(dev(ref1))
    tr.m_blob.copy_(dev(0.1 * g1)); tr.v_blob.copy_(dev(np.float32(0.01) * g1 * g1))
    tr._push_params()
    lm2, _ = tr.step(o, d, tgt, rp)
    assert abs(host(lm2)[0] - g["s2_loss"][0]) < 2e-4, (host(lm2), g["s2_loss"])
    ref2 = np.concatenate([g["s2_param_" + n].reshape(-1) for n in names])
    d2 = np.abs(host(tr.blob) - ref2) / lr
    assert d2.mean() < 8e-3 and (d2 > 0.05).mean() < 0.04, (d2.mean(), (d2 > 0.05).mean())
    assert g["s2_loss"][0] < g["s1_loss"][0] and host(lm2)[0] < host(lm1)[0]
    # the checkpoint layout of the classic model: the reference's parameter names in its registration order
    _, lay = tr._param_layout()
    assert [n for n, _, _ in lay] == names


def test_raw_and_training_step_without_importance_sampling(api):
    """N_importance = 0: the render's Raw is the coarse pass's raw (NeRFRenderer.h:421-423) -- also when the coarse intermediates are asked for in the same call (Raw was
    left unwritten then, and a training step differentiated garbage: tools/scratch/train_fuzz.py).  The step's gradients are non-zero and agree between the float-atomic,
    packed and binned table gradients and between the fp32 and matrix-core network backward."""
    from nerfpp_amd.train import Trainer
    K = api.S.lego_K(800, 800); c2w = api.S.pose_spherical(30.0, -30.0, 4.0)
    sc = api.S.make_hash_scene(mode="cu", log2_t=14, table_amp=1e-2, sigma_scale=4.0)
    rp = api.S.lego_render_params(sc["bbox"], 64, 0, 4096, api.L.NRF_PREC_F16_SPLIT, ReturnRaw=True, KeepIntermediates=True)
    res = sc["renderer"].Render(800, 800, K, rp, c2w=c2w, row0=400, rows=2)
    assert_exact(host(res.Raw), host(res.Extras["raw_coarse"]).reshape(host(res.Raw).shape), "Raw == the coarse raw when there is no fine pass")
    assert np.abs(host(res.Raw)).max() > 0
    o, d, _ = api.R.GetRays(800, 800, K, c2w)
    idx = torch.arange(0, 1000, device="cuda") * 640
    o = o.reshape(-1, 3)[idx].contiguous(); d = d.reshape(-1, 3)[idx].contiguous()
    tgt = torch.rand((1000, 3), generator=torch.Generator().manual_seed(3)).cuda()
    p = api.R.NeRFRenderParams(NSamples=64, NImportance=0, Chunk=1000, Perturb=0.0, WhiteBkgr=False, Ndc=False, UseViewdirs=True, ThinRay=True, BoundingBox=api.S.LEGO_BBOX,
                               Precision=api.L.NRF_PREC_F16_SPLIT)
    grads = {}
    for mb, hb in (("f32", "f32"), ("f32", "packed"), ("f32", "binned"), ("f16", "binned")):
        s2 = api.S.make_hash_scene(mode="cu", log2_t=14, table_amp=1e-2, sigma_scale=4.0)
        with Trainer(s2["embedder"], s2["embeddirs"], s2["mlp"], s2["table"], s2["mlp_blob"], mlp_backward=mb, hash_backward=hb) as tr:
            tr.step(o, d, tgt, p)
            grads[(mb, hb)] = (host(tr.g_table), host(tr.g_blob))
    gt, gb = grads[("f32", "f32")]
    assert np.abs(gt).max() > 0 and np.abs(gb).max() > 0
    assert_exact(grads[("f32", "binned")][0], grads[("f32", "packed")][0], "binned == packed table gradient")
    assert_close(grads[("f32", "packed")][0], gt, rtol=0, atol=2e-3 * np.abs(gt).max(), what="fixed-point table gradient vs float atomics")
    assert_close(grads[("f32", "packed")][1], gb, rtol=1e-5, atol=1e-6 * np.abs(gb).max(), what="network gradient: same backward, same raw")
    assert np.abs(grads[("f16", "binned")][1] - gb).max() < 5e-2 * np.abs(gb).max() and np.corrcoef(grads[("f16", "binned")][0], gt)[0, 1] > 0.99


def test_trainer_learns_a_teacher_scene(api):
    """Fit a freshly initialised CuHash + NeRFSmall student to the renders of a teacher: the loss must fall steadily
    (CuHashEmbedder backward, fp32 accumulation; the render the loss is computed on runs on the matrix cores)."""
    from nerfpp_amd.train import Trainer
    teacher = api.S.make_hash_scene(mode="cu", log2_t=14, sigma_scale=6.0)
    student = api.S.make_hash_scene(mode="cu", log2_t=14, seed=777, table_amp=1e-4, sigma_scale=1.0)
    K = api.S.lego_K(48, 48); bbox = api.S.LEGO_BBOX
    rp = api.R.NeRFRenderParams(NSamples=32, NImportance=32, Chunk=4096, Perturb=0.0, WhiteBkgr=False, Ndc=False, UseViewdirs=True, ThinRay=True,
                                BoundingBox=bbox, Precision=api.L.NRF_PREC_F16_SPLIT)
    views = []
    for th in (-120.0, -30.0, 60.0, 150.0):
        c2w = api.S.pose_spherical(th, -30.0, 4.0)
        o, d, _ = api.R.GetRays(48, 48, K, c2w)
        tgt = teacher["renderer"].Render(48, 48, K, rp, c2w=c2w).Outputs.RGBMap.reshape(-1, 3).clone()
        views.append((o.reshape(-1, 3), d.reshape(-1, 3), tgt))
    tr = Trainer(student["embedder"], student["embeddirs"], student["mlp"], student["table"], student["mlp_blob"], learning_rate=1e-2)
    losses = []
    for it in range(60):
        o, d, tgt = views[it % 4]
        lm, _ = tr.step(o, d, tgt, rp)
        losses.append(float(host(lm)[0]))
    first, last = np.mean(losses[:4]), np.mean(losses[-4:])
    assert np.isfinite(losses).all() and last < 0.5 * first, (first, last)


@pytest.mark.parametrize("F,T", [(2, 12), (8, 10)])
def test_hash_cu_backward_vs_oracle(api, O, F, T):
    """CuHashEmbedderBackwardKernel (CuHashEmbedder.cu:105-216): same corner set, same fp16-rounded contributions (x128 scaling), the
    overlap quirk of the level offsets included; fp32 accumulation vs the oracle's exact one."""
    import ctypes as C
    Lv = 6
    bbox = api.S.LEGO_BBOX
    e = api.M.CuHashEmbedder("embedder", bbox, Lv, F, T, 16, 256)
    primes = np.array(api.S.CU_PRIMES[:3 * Lv], np.int32)
    e.set_primes(primes); e.set_table(np.zeros(e.table_elems(), np.float32))
    rng = np.random.RandomState(5)
    x = rng.uniform(-1.6, 1.6, (5000, 3)).astype(np.float32)            # some points outside the box (clamped, like QueryPoints)
    g_emb = (rng.standard_normal((5000, Lv * F)) * rng.choice([1e-2, 1e-4, 0.0], (5000, 1))).astype(np.float32)
    gt = torch.zeros(e.table_elems(), device="cuda")
    xd, gd = dev(x), dev(g_emb)
    api.L.check(api.L.lib().nrf_hash_backward(e._h, C.c_void_p(xd.data_ptr()), C.c_int64(5000), C.c_void_p(gd.data_ptr()), C.c_void_p(gt.data_ptr()), None))
    ls = ((1 << T) >> 4) << 4
    ref = O.hash_cu_backward(x, primes, np.arange(Lv, dtype=np.int32) * ls, np.full(Lv, ls, np.int32), np.zeros((Lv, 3), np.float32), bbox,
                             O.hash_cu_scales(Lv, 16, 256), Lv, F, e.table_elems(), g_emb)
    assert (ref != 0).mean() > 0.05
    assert_close(host(gt), ref, rtol=2e-5, atol=1e-4 * np.abs(ref).max(), what="CuHash table gradient (fp32 atomics vs exact accumulation; a handful of entries differ by one fp16 ulp of a single contribution)")


@pytest.mark.parametrize("n_feat", [2, 4, 8])
@pytest.mark.parametrize("mode", ["ngp", "cu"])
def test_hash_backward_ray_coherent_equals_per_point(api, mode, n_feat):
    """nrf_hash_backward_rays (voxel-run pre-summation along each ray) == nrf_hash_backward up to fp32 summation order.  F = 4, 8 (LeRF's language grid) walk with one lane per
    feature (k_hash_bwd_ray_fl): rows whose gradient is zero in every feature are skipped by the whole group, rows with single zero features are not."""
    import ctypes as C
    sc = api.S.make_hash_scene(mode=mode, log2_t=15, n_feat=n_feat)
    e = sc["embedder"]
    n, s = 701, 37                                                        # ragged: s not a multiple of the segment length, n * segments not a multiple of the workgroup
    K = api.S.lego_K(64, 64); c2w = api.S.pose_spherical(20.0, -30.0, 4.0)
    o, d, _ = api.R.GetRays(64, 64, K, c2w)
    o = o.reshape(-1, 3)[:n]; d = d.reshape(-1, 3)[:n]
    z = torch.sort(torch.rand((n, s), device="cuda") * 3.0 + 2.0, dim=1).values
    z[:, 5:20] = z[:, 5:6] + torch.linspace(0, 0.01, 15, device="cuda")   # a dense cluster, as importance sampling produces
    pts = (o[:, None, :] + d[:, None, :] * z[..., None]).reshape(-1, 3).contiguous()
    g = (torch.randn((n * s, 16 * n_feat), device="cuda") * 1e-3).contiguous()
    g[::7] = 0.0                                                          # samples without gradient (masked / outside the box in a training step)
    g[3::5, 1::n_feat] = 0.0                                              # single zero features inside live rows
    a = torch.zeros(e.table_elems(), device="cuda"); b = torch.zeros_like(a)
    P = lambda t: C.c_void_p(t.data_ptr())
    api.L.check(api.L.lib().nrf_hash_backward(e._h, P(pts), C.c_int64(n * s), P(g), P(a), None))
    api.L.check(api.L.lib().nrf_hash_backward_rays(e._h, P(pts), C.c_int64(n), s, P(g), P(b), None))
    ha, hb = host(a), host(b)
    assert (ha != 0).mean() > 0.01
    assert_close(hb, ha, rtol=1e-4, atol=1e-4 * np.abs(ha).max())        # signed addends cancel: order-dependent to ~1e-7 of the sum of magnitudes


# ------------------------------------------------------------------ N2: ray-batch producer
def test_ray_batch_producer(api, O):
    from nerfpp_amd import dataset as D
    g = load_golden("rays")
    h, w = (int(v) for v in g["hw"])
    rng = np.random.RandomState(1)
    img = rng.rand(h, w, 3).astype(np.float32)
    v = D.View(H=h, W=w, K=g["k"], Pose=g["c2w"], Image=dev(img), Near=2.0, Far=6.0)
    ds = D.NeRFDataset([v], batch_size=500, precorp_iters=0, seed=11)
    ds.SetCurrentIter(5)
    b = ds.get_batch()
    rh, rw = host(b["rand_h"]), host(b["rand_w"])
    rh_o, rw_o = O.rand_pixels(11, 5, (0, h - 1, 0, w - 1), 500)
    assert_exact(rh, rh_o, "pixel rows == oracle"); assert_exact(rw, rw_o, "pixel columns == oracle")
    assert_exact(host(b["rays_d"]), g["d"][rh, rw], "rays_d == the reference's GetRays at those pixels")
    assert_exact(host(b["rays_o"]), g["o"][rh, rw]); assert_exact(host(b["target_s"]), img[rh, rw], "target colours")
    o_o, d_o, cone_o = O.ray_batch(g["k"], g["c2w"], rh, rw)
    assert float(b["cone_angle"]) == cone_o
    assert D.CalculateBounds(800, 800, 0, 500, 0.5) == (200, 599, 200, 599)
    # Blender bounds helpers on the reference's test orbit
    views = [D.View(H=800, W=800, K=api.S.lego_K(800, 800), Pose=api.S.pose_spherical(th, -30.0, 4.0), Near=2.0, Far=6.0) for th in (-180.0, -90.0, 0.0, 90.0)]
    near, far = D.GetBoundsForObj(views)
    assert 0 < near < far and abs(far / near - 4.0) < 1e-5
    bb = D.GetBbox3dForObj(views)
    assert (bb[:3] < -1.5).all() and (bb[3:] > 1.5).all(), "the frusta of four orbit cameras between Near and Far enclose the Lego box"


def test_lerf_fused_matrix_core_path(api, O, manifest):
    """The LeRF head fused with its render pass (mlp_lerf_mfma.hip: sigma net / LE net on the matrix cores, ||h|| pass + weighted-sum pass,
    raw_le never formed) against the stage-composed fp32 path and the oracle."""
    import ctypes as C
    Lv, F, T = 16, 8, 12
    bbox = api.S.LEGO_BBOX
    e = api.M.CuHashEmbedder("lang_embedder", bbox, Lv, F, T, 16, 128)
    table = synth.synth_sym(311, (Lv * (1 << T) * F,), np.float32(0.5))
    e.set_table(table); e.set_primes(np.array(api.S.CU_PRIMES[:3 * Lv], np.int32))
    blob = synth.blob_from_manifest(manifest["lerf"]).copy()
    blob[128 * 256:128 * 256 + 256] *= 20.0
    lerf = api.M.LeRF(32, 2, 256, 768, 128, "lang_model", params=blob)
    assert api.L.lib().nrf_lerf_mfma_available(lerf._m)
    fused = api.R.LeRFRenderer(e, lerf, precision=api.L.NRF_PREC_F16_MFMA); plain = api.R.LeRFRenderer(e, lerf, fused=False)
    assert fused.fused and not plain.fused
    K = api.S.lego_K(12, 12); c2w = api.S.pose_spherical(40.0, -30.0, 4.0)
    p = api.R.NeRFRenderParams(NSamples=32, NImportance=32, Chunk=50, Perturb=0.0, Ndc=False, UseViewdirs=True, ReturnWeights=True, ThinRay=True, BoundingBox=bbox)
    a = fused.Render(12, 12, K, p, c2w=c2w); b = plain.Render(12, 12, K, p, c2w=c2w)
    # stage check on identical points: sigma_le and the per-ray weighted sum of normalised embeddings vs the oracle
    rays = host(a.Extras["rays_flat"])
    z = O.z_vals(rays[:, 6], rays[:, 7], O.linspace(0, 1, 32))
    pts = O.points(rays[:, :3], rays[:, 3:6], z)
    ls = ((1 << T) >> 4) << 4
    emb, keep = O.hash_cu(pts.reshape(-1, 3), O.f32_to_f16(table), np.array(api.S.CU_PRIMES[:3 * Lv], np.int32), np.arange(Lv, dtype=np.int32) * ls,
                          np.full(Lv, ls, np.int32), np.zeros((Lv, 3), np.float32), bbox, O.hash_cu_scales(Lv, 16, 128), Lv, F)
    raw = O.lerf(blob, emb); raw_unmasked = raw.copy(); raw[~keep, -1] = 0
    sig_gpu, x_gpu = fused._sigma_fused(dev(pts))
    scale = np.abs(raw[:, -1]).max()
    assert_close(host(sig_gpu).reshape(-1), raw[:, -1], rtol=0, atol=3e-3 * scale, what="sigma_le, fp16 matrix-core sigma net")
    w = np.random.RandomState(0).rand(144, 32).astype(np.float32)
    acc = torch.empty((144, 768), device="cuda")
    wd = dev(w)
    assert fused.level_major and x_gpu.dtype == torch.float16 and tuple(x_gpu.shape) == (16, 144 * 32, 8)
    api.L.check(api.L.lib().nrf_lerf_render_embedding_lm(lerf._m, C.c_void_p(x_gpu.data_ptr()), C.c_void_p(wd.data_ptr()), C.c_int64(144), 32, C.c_void_p(acc.data_ptr()), None))
    ref = (w[:, :, None] * raw[:, :768].reshape(144, 32, 768)).sum(1)
    assert_close(host(acc), ref, rtol=0, atol=4e-3 * np.abs(ref).max(), what="sum_s w_s normalize(le_s)")
    # the level-major fp16 feature path against the fp32-row path: the same fp16 values reach the same kernels
    rowm = api.R.LeRFRenderer(e, lerf, precision=api.L.NRF_PREC_F16_MFMA); rowm.level_major = False
    sig_r, x_r = rowm._sigma_fused(dev(pts))
    assert x_r.dtype == torch.float32
    assert_exact(host(x_gpu).astype(np.float32).transpose(1, 0, 2).reshape(144 * 32, 128), host(x_r), "level-major fp16 features == row-major features")
    assert_exact(host(sig_gpu), host(sig_r), "sigma_le: level-major == row-major input")
    acc_r = torch.empty((144, 768), device="cuda")
    api.L.check(api.L.lib().nrf_lerf_render_embedding(lerf._m, C.c_void_p(x_r.data_ptr()), C.c_void_p(wd.data_ptr()), C.c_int64(144), 32, C.c_void_p(acc_r.data_ptr()), None))
    assert_close(host(acc), host(acc_r), rtol=0, atol=1e-5 * np.abs(ref).max(), what="embedding sums differ by the order of the float atomics only")
    # end to end: same rays, fused vs stage-composed fp32
    hit = host(b.Outputs.AccMapLE) > 1e-2
    assert hit.sum() > 20
    ea, eb = host(a.Outputs.RenderedLangEmbedding)[hit], host(b.Outputs.RenderedLangEmbedding)[hit]
    assert_close(np.linalg.norm(ea, axis=1), np.ones(hit.sum()), rtol=1e-5, atol=0)
    cos = (ea * eb).sum(1)
    # fp16 sigma moves a few fine samples across CDF plateaus; on this field (independent random embeddings per voxel) a moved sample turns
    # the mixture direction, so the end-to-end comparison is statistical -- the stage checks above are the tight ones
    assert np.median(cos) > 0.99999 and (cos > 0.999).mean() > 0.85 and cos.min() > 0.9, (np.median(cos), (cos > 0.999).mean(), cos.min())
    da = np.abs(host(a.Outputs.AccMapLE) - host(b.Outputs.AccMapLE))
    assert np.median(da) < 1e-3 and (da < 5e-3).mean() > 0.9, (np.median(da), (da < 5e-3).mean())


def test_raw2outputs_backward_with_noise_vs_oracle(api, O):
    import ctypes as C
    g = load_golden("train_hash")
    rays = O.pack_rays(g["rays_o"], g["rays_d"], g["bbox"])
    rng = np.random.RandomState(2)
    noise = rng.standard_normal((64, 64)).astype(np.float32); g_rgb = (rng.standard_normal((64, 3)) * 1e-2).astype(np.float32)
    raw, z, d, nz, gr = dev(g["s1_fine_raw"]), dev(g["s1_fine_z"]), dev(rays[:, 3:6]), dev(noise), dev(g_rgb)
    out = torch.empty_like(raw)
    P = lambda t: C.c_void_p(t.data_ptr())
    api.L.check(api.L.lib().nrf_raw2outputs_backward_noise(P(raw), P(z), P(d), 3, C.c_int64(64), 64, 4, 1, P(nz), C.c_float(0.7), P(gr), P(out), None))
    ref = O.raw2outputs_backward_noise(g["s1_fine_raw"], g["s1_fine_z"], rays[:, 3:6], g_rgb, noise, 0.7, white_bkgr=True)
    assert_close(host(out), ref, rtol=1e-5, atol=1e-7 * np.abs(ref).max())
    plain = O.raw2outputs_backward(g["s1_fine_raw"], g["s1_fine_z"], rays[:, 3:6], g_rgb, white_bkgr=True)
    assert np.abs(ref - plain).max() > 1e-3 * np.abs(plain).max(), "the noise must matter"


def test_trainer_with_stochastic_branches_sees_the_forwards_samples(api):
    """RawNoiseStd, stochastic preconditioning and cone rays during training (FillRenderParams, NeRFExecutor.h:405-411): the backward
    regenerates the forward's counter-based draws.  Check: the features recomputed for the backward reproduce the forward's raw output
    exactly (fp32 mode), and a few steps reduce the loss."""
    from nerfpp_amd.train import Trainer
    sc = api.S.make_hash_scene(mode="cu", log2_t=14, seed=777, table_amp=1e-2, sigma_scale=2.0)
    K = api.S.lego_K(32, 32); c2w = api.S.pose_spherical(20.0, -30.0, 4.0)
    o, d, cone = api.R.GetRays(32, 32, K, c2w)
    o = o.reshape(-1, 3); d = d.reshape(-1, 3)
    tgt = torch.rand((1024, 3), device="cuda") * 0.2 + 0.4
    tr = Trainer(sc["embedder"], sc["embeddirs"], sc["mlp"], sc["table"], sc["mlp_blob"], learning_rate=5e-3)
    rp = api.R.NeRFRenderParams(NSamples=32, NImportance=32, Chunk=400, Perturb=0.0, WhiteBkgr=False, Ndc=False, UseViewdirs=True, ThinRay=False, RawNoiseStd=0.5,
                                StochasticPreconditioningAlpha=0.01, BoundingBox=api.S.LEGO_BBOX, Precision=api.L.NRF_PREC_F32, Seed=123)
    rp.ReturnRaw, rp.KeepIntermediates = True, True
    res = tr.renderer.Render(0, 0, None, rp, rays=(o, d, cone))
    tr.backward(res, tgt, 64, False, params=rp, cone_angle=cone)
    raw_again = tr.mlp.forward(tr.last["x"], api.L.NRF_PREC_F32)
    keep = tr.embedder.forward(tr.last["pts"])[1]
    raw_again[~keep, 3] = 0
    assert_exact(host(raw_again), host(res.Raw).reshape(-1, 4), "backward's recomputed points/features == the forward's (cone + preconditioning draws regenerated)")
    losses = []
    for it in range(12):
        rp.Seed = 1000 + it
        lm, _ = tr.step(o, d, tgt, rp, cone_angle=cone)
        losses.append(float(host(lm)[0]))
    assert np.isfinite(losses).all() and np.mean(losses[-3:]) < 0.8 * np.mean(losses[:3]), losses


def test_render_from_reference_checkpoint(api, O, manifest):
    """N3 end to end: a checkpoint written by the reference's torch::save (tests/golden/ckpt) is loaded, its tensors handed to the C ABI in
    checkpoint order, and the render equals the oracle render of the same weights bit for bit (fp32 mode)."""
    import os
    from conftest import GOLDEN
    from nerfpp_amd import checkpoint as CK
    ck = CK.LoadCheckpoint(os.path.join(GOLDEN, "ckpt"))
    g = load_golden("train_hash")
    e = api.M.HashEmbedder("embedder", g["bbox"], 4, 2, 12, 16, 128)
    e.set_table(CK.blob(ck["embedder"]))
    m = api.M.NeRFSmall(3, 64, 15, 3, 64, False, 3, 64, 8, 16, "model", params=CK.blob(ck["model"]))
    r = api.R.NeRFRenderer(e, api.M.SHEncoder("embeddirs", 3, 4), m)
    rp = api.R.NeRFRenderParams(NSamples=32, NImportance=32, Chunk=64, Perturb=0.0, WhiteBkgr=False, Ndc=False, UseViewdirs=True, ThinRay=True,
                                BoundingBox=g["bbox"], Precision=api.L.NRF_PREC_F32)
    res = r.Render(0, 0, None, rp, rays=(dev(g["rays_o"]), dev(g["rays_d"]), None))
    dref = np.abs(host(res.Outputs.RGBMap) - g["s1_rgb"])      # vs the reference's own render of these weights (32+32 samples: a fine sample in another
    assert np.median(dref) < 1e-5 and (dref < 1e-4).mean() > 0.9, (np.median(dref), (dref < 1e-4).mean())      # CDF bin is worth a few 1e-2 of a pixel)
    model = O.Model(0, CK.blob(ck["model"]), bbox=g["bbox"], table_f32=CK.blob(ck["embedder"]), L=4, F=2, log2_t=12, base=16, finest=128, n_layers_c=3)
    oc = O.render_rays(model, host(res.Extras["rays_flat"]), 32, 32, O.linspace(0, 1, 32), O.linspace(0, 1, 32), white_bkgr=False)
    assert_exact(host(res.Outputs.RGBMap), oc["rgb"], "== oracle on the checkpoint's tensors")


def test_lerf_renderer_falls_back_when_samples_are_not_multiples_of_32(api, manifest):
    Lv, F, T = 16, 8, 12
    e = api.M.CuHashEmbedder("lang_embedder", api.S.LEGO_BBOX, Lv, F, T, 16, 128)
    e.set_table(synth.synth_sym(311, (Lv * (1 << T) * F,), np.float32(0.5))); e.set_primes(np.array(api.S.CU_PRIMES[:3 * Lv], np.int32))
    lerf = api.M.LeRF(32, 2, 256, 768, 128, "lang_model", params=synth.blob_from_manifest(manifest["lerf"]))
    r = api.R.LeRFRenderer(e, lerf)
    K = api.S.lego_K(6, 6); c2w = api.S.pose_spherical(40.0, -30.0, 4.0)
    p = api.R.NeRFRenderParams(NSamples=20, NImportance=17, Chunk=36, Perturb=0.0, Ndc=False, UseViewdirs=True, ReturnWeights=True, ThinRay=True, BoundingBox=api.S.LEGO_BBOX)
    res = r.Render(6, 6, K, p, c2w=c2w)               # 37 samples per ray: the stage-composed path
    assert host(res.Outputs.WeightsLE).shape == (36, 37) and np.isfinite(host(res.Outputs.RenderedLangEmbedding)).all()
    with pytest.raises(api.L.NrfError, match="multiple of 32"):
        import ctypes as C
        x = torch.zeros((37, 128), device="cuda"); w = torch.zeros((37,), device="cuda"); out = torch.zeros((1, 768), device="cuda")
        api.L.check(api.L.lib().nrf_lerf_render_embedding(lerf._m, C.c_void_p(x.data_ptr()), C.c_void_p(w.data_ptr()), C.c_int64(1), 37, C.c_void_p(out.data_ptr()), None))


# ------------------------------------------------------------------ HashEmbedder (LibTorch semantics) on the fast path
def test_ngp_fast_path_vs_reference_render(api, manifest):
    """The reference's own LibTorch CPU render (golden render_hash: HashEmbedder + SHEncoder + NeRFSmall) against the fast path -- dense fp32
    pyramid, level-major hi/lo fp16 features, split-precision matrix-core MLP: pixels within the north star's 1e-4."""
    g = load_golden("render_hash")
    r, _ = _golden_hash_scene(api, manifest)
    res = r.Render(8, 8, g["k"], _params(api, g["bbox"], 64, Precision=api.L.NRF_PREC_F16_SPLIT), c2w=g["c2w"])
    ref32 = r.Render(8, 8, g["k"], _params(api, g["bbox"], 64, Precision=api.L.NRF_PREC_F32), c2w=g["c2w"])
    rgb = host(res.Outputs.RGBMap)
    scale = np.abs(g["coarse_raw"]).max()
    # samples outside the box: sigma is masked in both; the colour the fast path reports there is the network's on ZERO features (k_hash_ngp_lm: the extrapolated
    # features of far-away points leave the fp16 range) -- weightless either way, compared inside the box only
    rays = res.Extras["rays_flat"]; zc = res.Extras["z_coarse"]
    _, keep = r.EmbedFn.forward((rays[:, None, 0:3] + rays[:, None, 3:6] * zc[..., None]).reshape(-1, 3))
    keep = host(keep).reshape(zc.shape)
    rc, rc32 = host(res.Extras["raw_coarse"]), host(ref32.Extras["raw_coarse"])
    assert_close(rc[..., 3], rc32[..., 3], rtol=0, atol=3e-6 * scale, what="coarse sigma: split fast path vs fp32 parity mode (every sample)")
    assert_close(rc[keep], rc32[keep], rtol=0, atol=3e-6 * scale, what="coarse raw inside the box: split fast path vs fp32 parity mode")
    assert np.isfinite(rc).all()
    assert_close(rgb, g["out_rgb"], rtol=0, atol=1e-4, what="fast path pixels within 1e-4 of the reference's LibTorch CPU render")
    assert api.S.psnr(rgb, g["out_rgb"]) > 80


def test_ngp_fast_path_features_equal_generic_encoder(api):
    """k_hash_ngp_lm (dense fp32 pyramid) == k_hash_ngp (hashed fp32 tables): hi plane = f16(feature), hi + lo = feature to 2^-22."""
    import ctypes as C
    sc = api.S.make_hash_scene(mode="ngp")
    K = api.S.lego_K(800, 800); c2w = api.S.pose_spherical(30.0, -30.0, 4.0)
    rp = api.S.lego_render_params(sc["bbox"], chunk=1000, precision=api.L.NRF_PREC_F16_SPLIT, ReturnRaw=True, KeepIntermediates=True)
    res = sc["renderer"].Render(800, 800, K, rp, c2w=c2w, row0=400, rows=2)
    rays = res.Extras["rays_flat"]; zf = res.Extras["z_fine"]
    n, s = zf.shape
    pts = (rays[:, None, 0:3] + rays[:, None, 3:6] * zf[..., None]).reshape(-1, 3)
    emb, keep = sc["embedder"].forward(pts)
    dirs, _ = sc["embeddirs"].forward(rays[:, 8:11].contiguous())
    emb[~keep] = 0                                                       # the fast path encodes a point outside the box as zeros (k_hash_ngp_lm): its sigma is masked anyway
    x = torch.cat([emb, dirs[:, None, :].expand(n, s, dirs.shape[1]).reshape(n * s, -1)], 1).contiguous()
    ref = sc["mlp"].forward(x, api.L.NRF_PREC_F16_SPLIT)                 # fp32 rows -> the kernel splits them itself: same hi/lo operands
    ref[~keep, 3] = 0
    assert_exact(host(res.Raw).reshape(-1, 4), host(ref), "fast path raw == stage-wise split raw (identical hi/lo operands, identical lookups)")
    # the default split render (sigma-only fp32 coarse pass; the fine pass keeps the coarse columns of both feature planes and encodes the new samples only)
    rp2 = api.S.lego_render_params(sc["bbox"], chunk=1000, precision=api.L.NRF_PREC_F16_SPLIT, ReturnRaw=True, KeepIntermediates="depths")
    res2 = sc["renderer"].Render(800, 800, K, rp2, c2w=c2w, row0=400, rows=2)
    check_default_split_fine_pass(api, sc, res2, rays, "HashEmbedder, default split render")
    f32 = sc["renderer"].Render(800, 800, K, api.S.lego_render_params(sc["bbox"], chunk=1000, precision=api.L.NRF_PREC_F32), c2w=c2w, row0=400, rows=2)
    assert api.S.psnr(host(res.Outputs.RGBMap), host(f32.Outputs.RGBMap)) > 85


@pytest.mark.parametrize("mode", ["ngp", "cu"])
def test_rays_that_miss_the_box_render_finite_background_in_every_precision(api, mode):
    """A ray that misses the bounding box keeps a degenerate depth interval (far = near + 1e-6, RayUtils.h:87-126) OUTSIDE the box: every sample has keep == false, sigma is
    forced to 0 (NeRFRenderer.h:187-188) and the pixel is the background.  HashEmbedder extrapolates such points with weights from the unclamped coordinate
    (NeRF.cpp:265-277) -- 1e5 at the finest levels half a scene away -- which leaves the fp16 range: the matrix-core precisions once returned 0 * NaN there.  All
    precisions: finite everywhere, the missing rays exactly white, everything else as close to NRF_PREC_F32 as the precision allows."""
    sc = api.S.make_hash_scene(mode=mode, log2_t=16)
    h, w = 120, 97
    K = api.S.lego_K(h, w); c2w = api.S.pose_spherical(40.0, -25.0, 4.0)
    outs = {}
    for prec in (api.L.NRF_PREC_F32, api.L.NRF_PREC_F16_MFMA, api.L.NRF_PREC_F16_SPLIT):
        rp = api.S.lego_render_params(sc["bbox"], 64, 128, 4000, prec, ReturnWeights=True, ReturnRaw=(prec != api.L.NRF_PREC_F32), KeepIntermediates=True)
        res = sc["renderer"].Render(h, w, K, rp, c2w=c2w)
        rays = host(res.Extras["rays_flat"])
        miss = (rays[:, 7] - rays[:, 6]) < 1e-5                         # near == far up to the 1e-6 floor
        assert miss.sum() >= 3, "the pose is chosen so that a few rays miss the box"
        rgb = host(res.Outputs.RGBMap).reshape(-1, 3)
        for f in ("RGBMap", "DepthMap", "AccMap", "DispMap", "Weights"):
            assert np.isfinite(host(getattr(res.Outputs, f))).all(), f"{f} finite, precision {prec}"
        if res.Raw is not None:
            assert np.isfinite(host(res.Raw)).all(), f"raw network outputs finite, precision {prec}"
        assert_exact(rgb[miss], np.ones_like(rgb[miss]), f"missing rays are white background, precision {prec}")
        assert_exact(host(res.Outputs.AccMap).reshape(-1)[miss], np.zeros(miss.sum(), np.float32), "... with zero opacity")
        outs[prec] = rgb
    # (with the intermediates kept the coarse pass of the split mode runs the whole network in split precision, not the exact sigma pass: a moved sample here and there)
    assert api.S.psnr(outs[api.L.NRF_PREC_F16_SPLIT], outs[api.L.NRF_PREC_F32]) > 70
    assert api.S.psnr(outs[api.L.NRF_PREC_F16_MFMA], outs[api.L.NRF_PREC_F32]) > 35


@pytest.mark.parametrize("mode", ["ngp", "cu"])
def test_few_importance_samples_fit_the_workspace(api, mode):
    """N_importance much smaller than N_samples (64 + 5): the feature-reuse layout of the hash fast paths (two feature planes per column + the fp32 plane of the coarse
    columns with the HashEmbedder) is then larger than the generic network scratch the workspace formula was sized by -- nrf_render_rays answered NRF_ERR_WORKSPACE
    (found by tools/scratch/render_fuzz.py).  Renders, chunk-invariant, close to NRF_PREC_F32."""
    sc = api.S.make_hash_scene(mode=mode, log2_t=15)
    K = api.S.lego_K(130, 44); c2w = api.S.pose_spherical(10.0, -30.0, 4.0)
    outs = []
    for chunk in (5564, 1000):
        rp = api.S.lego_render_params(sc["bbox"], 64, 5, chunk, api.L.NRF_PREC_F16_SPLIT)
        outs.append(host(sc["renderer"].Render(130, 44, K, rp, c2w=c2w).Outputs.RGBMap))
    assert_exact(outs[1], outs[0], "independent of Chunk")
    f32 = host(sc["renderer"].Render(130, 44, K, api.S.lego_render_params(sc["bbox"], 64, 5, 5564, api.L.NRF_PREC_F32), c2w=c2w).Outputs.RGBMap)
    assert api.S.psnr(outs[0], f32) > 90


def test_seeded_render_invariance_sweep(api):
    """A seeded sweep in the manner of tools/scratch/render_fuzz.py / lane_fuzz.py (which found four defects in round 4): random frame sizes, sample counts, chunk sizes,
    row tiles, lane counts, scenes and precisions -- a render does not depend on Chunk or on the number of lanes, a row tile equals the rows of the frame, everything is
    finite (rays that miss the box included)."""
    rng = np.random.default_rng(20261004)
    lib = api.L.lib()
    scenes = [api.S.make_hash_scene(mode="cu", log2_t=14), api.S.make_hash_scene(mode="ngp", log2_t=14), api.S.make_classic_scene()]
    eq = lambda a, b: a.shape == b.shape and torch.equal(a.nan_to_num(nan=4321.0), b.nan_to_num(nan=4321.0))
    try:
        for case in range(18):
            which = case % 3; sc = scenes[which]; r = sc["renderer"]
            h, w = (int(rng.integers(12, 40)), int(rng.integers(12, 40))) if which == 2 else (int(rng.integers(100, 300)), int(rng.integers(100, 300)))
            s = int(rng.choice([8, 17, 64])); ni = int(rng.choice([0, 5, 128]))
            prec = int(rng.choice([api.L.NRF_PREC_F32, api.L.NRF_PREC_F16_MFMA, api.L.NRF_PREC_F16_SPLIT])) if which != 2 or case % 2 else api.L.NRF_PREC_F16_SPLIT
            n = h * w
            K = api.S.lego_K(h, w); c2w = api.S.pose_spherical(float(rng.uniform(-180, 180)), float(rng.uniform(-60, -5)), float(rng.uniform(3.0, 4.6)))
            what = f"case {case}: scene {which} {h}x{w} s {s}+{ni} precision {prec}"
            def render(chunk, lanes, **kw):
                api.L.check(lib.nrf_set_render_lanes(lanes))
                o = r.Render(h, w, K, api.S.lego_render_params(sc["bbox"], s, ni, chunk, prec, ReturnWeights=True), c2w=c2w, **kw).Outputs
                return [o.RGBMap, o.DepthMap, o.AccMap, o.Weights]
            full = render(n, 1)
            assert all(bool(torch.isfinite(t).all()) for t in full), what + ": finite"
            for chunk, lanes in ((int(rng.integers(max(1, n // 6), n)), 2), (33001, 3), (int(rng.integers(max(1, n // 6), n)), 4)):
                assert all(eq(a, b) for a, b in zip(full, render(chunk, lanes))), what + f": chunk {chunk} on {lanes} lanes == one chunk on one stream"
            row0 = int(rng.integers(0, h)); rows = int(rng.integers(1, h - row0 + 1))
            t = render(int(rng.integers(max(1, n // 6), n)), 2, row0=row0, rows=rows)
            assert all(eq(a.reshape(b[row0:row0 + rows].shape), b[row0:row0 + rows]) for a, b in zip(t, [f.reshape(h, w, -1) for f in full])), what + f": tile {row0}+{rows} == rows of the frame"
    finally:
        api.L.check(lib.nrf_set_render_lanes(2))


def test_feature_reusing_fine_pass_equals_stagewise_cu(api):
    """Default split render of the CuHashEmbedder scene (see check_default_split_fine_pass) -- ragged chunk sizes included."""
    sc = api.S.make_hash_scene(mode="cu")
    K = api.S.lego_K(800, 800); c2w = api.S.pose_spherical(30.0, -30.0, 4.0)
    rp = api.S.lego_render_params(sc["bbox"], chunk=700, precision=api.L.NRF_PREC_F16_SPLIT, ReturnRaw=True, KeepIntermediates="depths")
    res = sc["renderer"].Render(800, 800, K, rp, c2w=c2w, row0=399, rows=2)
    assert res.Extras["z_fine"].shape[1] == 192
    check_default_split_fine_pass(api, sc, res, res.Extras["rays_flat"], "CuHashEmbedder, default split render")
    # without ReturnRaw the compositing kernel reads the column-ordered outputs through the merge map: same pixels as composing the gathered rows
    rp_n = api.S.lego_render_params(sc["bbox"], chunk=700, precision=api.L.NRF_PREC_F16_SPLIT)
    res_n = sc["renderer"].Render(800, 800, K, rp_n, c2w=c2w, row0=399, rows=2)
    for f in ("RGBMap", "DepthMap", "AccMap", "DispMap"):
        assert_exact(host(getattr(res_n.Outputs, f)), host(getattr(res.Outputs, f)), f"{f}: merge-map read in the compositing kernel == gathered rows")


@pytest.mark.parametrize("workload,coarse", [("hash", "full"), ("classic", "full"), ("classic", "exact")])
def test_composite_through_merge_map_equals_gathered_rows(api, workload, coarse):
    """Fine passes that keep the coarse pass's network outputs (NRF_COARSE_FULL of either network, the classic network's exact coarse pass): without ReturnRaw the
    compositing kernel reads each sample's row through the merge map (coarse rows | new-sample rows); with it the rows are first gathered into depth order.
    Same rows, same order of the per-ray scan: identical maps."""
    sc = api.S.make_hash_scene(mode="cu") if workload == "hash" else api.S.make_classic_scene()
    K = api.S.lego_K(800, 800); c2w = api.S.pose_spherical(30.0, -30.0, 4.0)
    kw = dict(CoarseMode=api.L.NRF_COARSE_FULL) if coarse == "full" else {}
    outs = []
    for raw in (False, True):
        rp = api.S.lego_render_params(sc["bbox"], chunk=900, precision=api.L.NRF_PREC_F16_SPLIT, ReturnRaw=raw, ReturnWeights=True, **kw)
        outs.append(sc["renderer"].Render(800, 800, K, rp, c2w=c2w, row0=401, rows=2))
    for f in ("RGBMap", "DepthMap", "AccMap", "DispMap", "Weights"):
        assert_exact(host(getattr(outs[0].Outputs, f)), host(getattr(outs[1].Outputs, f)), f"{workload}/{coarse} {f}")


def test_tv_loss_vs_oracle_and_reference(api, O, manifest):
    import ctypes as C
    g = load_golden("tv_loss")
    ent = manifest["tv_loss"]
    table = synth.blob_from_manifest(ent)
    e = api.M.HashEmbedder("embedder", api.S.LEGO_BBOX, 6, 2, 14, 16, 256)
    e.set_table(table)
    td = dev(table)
    for level in (0, 3, 5):
        mv = np.ascontiguousarray(g[f"l{level}_min_vertex"], np.int32); cube = int(g[f"l{level}_res_cube"][1])
        loss = torch.zeros(1, device="cuda"); gt = torch.zeros(table.size, device="cuda")
        api.L.check(api.L.lib().nrf_hash_tv_loss(e._h, C.c_void_p(td.data_ptr()), level, mv.ctypes.data_as(C.c_void_p), cube, C.c_float(1.0), C.c_void_p(loss.data_ptr()),
                                                 C.c_void_p(gt.data_ptr()), None))
        assert abs(float(loss) - g[f"l{level}_loss"][0]) < 2e-5 * g[f"l{level}_loss"][0]
        got = host(gt).reshape(6, 1 << 14, 2)
        ref = g[f"l{level}_grad"]
        assert_close(got[level], ref, rtol=1e-4, atol=1e-5 * np.abs(ref).max(), what=f"TV gradient, level {level}")
        assert np.abs(np.delete(got, level, axis=0)).max() == 0, "only the level's own table receives gradient"


@pytest.mark.parametrize("mode", ["cu", "ngp"])
def test_hash_backward_packed_fixed_point_vs_float_atomics(api, mode):
    """nrf_hash_backward_rays_packed (one 64-bit fixed-point atomic per entry) against nrf_hash_backward_rays (one float atomic per feature,
    pinned to the reference's autograd by test_training_backward_stages_vs_reference_autograd): same addends, so the difference is the
    round-to-nearest of each addend to (mass bound) * 2^-30, with the bound computed on the device.  Includes samples piled onto one voxel
    (the overflow-relevant case) and accumulation into a non-zero g_table."""
    import ctypes as C
    P = lambda t: C.c_void_p(t.data_ptr())
    sc = api.S.make_hash_scene(mode=mode, log2_t=14, seed=99, table_amp=0.3)
    e = sc["embedder"]
    rng = np.random.default_rng(5)
    n, s = 600, 48
    bb = api.S.LEGO_BBOX
    o = rng.uniform(bb[:3], bb[3:], (n, 1, 3)); dd = rng.standard_normal((n, 1, 3)) * 0.02
    pts = (o + dd * np.arange(s)[None, :, None]).astype(np.float32)
    pts[:50] = pts[0, 0]                                  # 2400 samples in one voxel of every level
    pts[50:60] += np.float32(3.0 if mode == "cu" else 2e-3)     # outside the box: the HashEmbedder's weights leave [0,1] there and the bound has to know (it grows with the distance)
    g = (rng.standard_normal((n * s, 32)) * 1e-4).astype(np.float32)
    g[:50 * s] = np.abs(g[:50 * s])                       # coherent: the pile adds up
    g[rng.random(n * s) < 0.1] = 0.0
    dp, dg = dev(pts.reshape(-1, 3)), dev(g)
    lib = api.L.lib()
    base = (rng.standard_normal(e.table_elems()) * 1e-3).astype(np.float32)
    gt_f, gt_q = dev(base.copy()), dev(base.copy())
    api.L.check(lib.nrf_hash_backward_rays(e._h, P(dp), C.c_int64(n), s, P(dg), P(gt_f), None))
    nb = lib.nrf_hash_backward_packed_workspace_bytes(e._h)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    for _ in range(2):                                    # second call: the workspace is reusable as is
        gt_q.copy_(dev(base))
        api.L.check(lib.nrf_hash_backward_rays_packed(e._h, P(dp), C.c_int64(n), s, P(dg), P(gt_q), P(ws), C.c_size_t(nb), None))
    a, b = host(gt_q) - base, host(gt_f) - base
    assert np.abs(b).max() > 1e-2                         # the pile
    unit = float(ws[768 + 4:768 + 8].view(torch.float32).cpu()[0])          # 1 / scale of the (only) pass, as the device chose it
    mass = np.abs(g).reshape(-1, 16, 2).max(2).sum(0)     # per level
    bound = (mass[:-1] + mass[1:]).max() if mode == "cu" else mass.max()
    assert unit >= bound * 2.0 ** -30                     # never finer than the rigorous bound allows ...
    if mode == "cu":
        assert unit <= bound * 1.01 * 2.0 ** -29          # ... and no coarser than the next power of two (the outside points only matter in ngp mode)
    # an entry collects at most n*s*8 addends (in practice tens, 2400 on the pile), each off by <= unit/2, plus the float path's own fp32 summation noise
    tol = 64 * unit + 3e-6 * np.abs(b)
    assert (np.abs(a - b) <= tol).all(), (np.abs(a - b).max(), unit)
    nz = b != 0
    assert np.sqrt(np.mean((a[nz] - b[nz]) ** 2)) < 4 * unit + 1e-6 * np.sqrt(np.mean(b[nz] ** 2))
    if mode == "cu":
        h4 = api.M.CuHashEmbedder("e4", bb, 8, 4, 14, 16, 256)
        h4.set_primes(np.array(api.S.CU_PRIMES[:24], np.int32))
        with pytest.raises(api.L.NrfError):
            api.L.check(lib.nrf_hash_backward_rays_packed(h4._h, P(dp), C.c_int64(n), s, P(dg), P(gt_q), P(ws), C.c_size_t(nb), None))


@pytest.mark.parametrize("mode,log2_t", [("cu", 14), ("ngp", 14), ("cu", 19)])
def test_hash_backward_binned_equals_packed_bit_for_bit(api, mode, log2_t):
    """nrf_hash_backward_rays_binned (records binned by table range, summed in LDS, added without atomics) against nrf_hash_backward_rays_packed (one 64-bit
    fixed-point atomic per contribution): same groups of points, same device-side scale, integer sums -- the gradient tables must be IDENTICAL.  Several groups
    (n * s > 2^18), a pile of samples on one voxel, points outside the box, zero gradients, accumulation into a non-zero table, workspace reuse."""
    import ctypes as C
    P = lambda t: C.c_void_p(t.data_ptr())
    sc = api.S.make_hash_scene(mode=mode, log2_t=log2_t, seed=77, table_amp=0.3)
    e = sc["embedder"]
    rng = np.random.default_rng(11)
    n, s = 3000, 192                                      # 576 000 points: three groups of <= 2^18
    bb = api.S.LEGO_BBOX
    o = rng.uniform(bb[:3], bb[3:], (n, 1, 3)); dd = rng.standard_normal((n, 1, 3)) * 0.004
    pts = (o + dd * np.arange(s)[None, :, None]).astype(np.float32)
    pts[:20] = pts[0, 0]                                  # 3 840 samples in one voxel of every level
    pts[20:30] += np.float32(3.0 if mode == "cu" else 2e-3)
    g = (rng.standard_normal((n * s, 32)) * 1e-4).astype(np.float32)
    g[rng.random(n * s) < 0.1] = 0.0
    # a few samples that dominate their pass (one in each of the three passes): their fixed-point addends exceed the 25-bit fields of the 8-byte records and
    # travel through the side list
    for row in (100, n * s // 2, n * s - 50):
        g[row] = rng.choice([-1.0, 1.0], 32).astype(np.float32) * np.float32(20.0)
    dp, dg = dev(pts.reshape(-1, 3)), dev(g)
    lib = api.L.lib()
    base = (rng.standard_normal(e.table_elems()) * 1e-3).astype(np.float32)
    gt_q, gt_b = dev(base.copy()), dev(base.copy())
    nb = lib.nrf_hash_backward_packed_workspace_bytes(e._h)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    api.L.check(lib.nrf_hash_backward_rays_packed(e._h, P(dp), C.c_int64(n), s, P(dg), P(gt_q), P(ws), C.c_size_t(nb), None))
    nbb = lib.nrf_hash_backward_binned_workspace_bytes(e._h, s)
    wsb = torch.empty(nbb, dtype=torch.uint8, device="cuda")
    with pytest.raises(api.L.NrfError):
        api.L.check(lib.nrf_hash_backward_rays_binned(e._h, P(dp), C.c_int64(n), s, P(dg), P(gt_b), P(wsb), C.c_size_t(nbb - 1), None))
    for _ in range(2):                                    # second call: the workspace is reusable as is
        gt_b.copy_(dev(base))
        api.L.check(lib.nrf_hash_backward_rays_binned(e._h, P(dp), C.c_int64(n), s, P(dg), P(gt_b), P(wsb), C.c_size_t(nbb), None))
    a, b = host(gt_b), host(gt_q)
    assert np.abs(b - base).max() > 0
    assert_exact(a, b, f"{mode} T=2^{log2_t}: binned table gradient == packed-atomic table gradient")
    side = int(host(wsb[65536:65540]).view(np.uint32)[0])       # entries of the LAST pass's side list (the workspace keeps the counter behind its 64-KB header)
    assert 0 < side <= 128 * 16, f"{mode}: the dominating sample's addends went through the side list ({side} entries)"
    # a workspace sized for THIS batch (records for n rays instead of a whole 2^18-point pass) serves the same call
    nbf = lib.nrf_hash_backward_binned_workspace_bytes_for(e._h, C.c_int64(n), s)
    assert 0 < nbf <= nbb
    wsf = torch.empty(nbf, dtype=torch.uint8, device="cuda")
    gt_f = dev(base.copy())
    api.L.check(lib.nrf_hash_backward_rays_binned(e._h, P(dp), C.c_int64(n), s, P(dg), P(gt_f), P(wsf), C.c_size_t(nbf), None))
    assert_exact(host(gt_f), b, "batch-sized workspace: same table gradient")


def test_trainer_matrix_core_backward_matches_fp32_trainer(api):
    """Trainer(mlp_backward="f16") vs the fp32 trainer on the same rendered batch of a HashNeRF scene: gradients of the MLP and of the hash table
    (which sees the MLP backward through d loss / d features), then three optimisation steps with the same loss trajectory."""
    from nerfpp_amd.train import Trainer
    sc = api.S.make_hash_scene(mode="cu", log2_t=15, seed=4242, table_amp=0.3, sigma_scale=3.0)
    K = api.S.lego_K(32, 32); c2w = api.S.pose_spherical(20.0, -30.0, 4.0)
    o, d, _ = api.R.GetRays(32, 32, K, c2w)
    o = o.reshape(-1, 3); d = d.reshape(-1, 3)
    tgt = torch.rand((1024, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    rp = api.R.NeRFRenderParams(NSamples=32, NImportance=32, Chunk=1024, Perturb=0.0, WhiteBkgr=False, Ndc=False, UseViewdirs=True, ThinRay=True,
                                BoundingBox=api.S.LEGO_BBOX, Precision=api.L.NRF_PREC_F16_SPLIT, ReturnRaw=True, KeepIntermediates=True)
    grads = {}
    for mode in ("f32", "f16"):
        tr = Trainer(sc["embedder"], sc["embeddirs"], sc["mlp"], sc["table"], sc["mlp_blob"], learning_rate=1e-3, mlp_backward=mode)
        res = tr.renderer.Render(0, 0, None, rp, rays=(o, d, None))
        lm = tr.backward(res, tgt, 64, False, rp)
        grads[mode] = (host(tr.g_blob).copy(), host(tr.g_table).copy(), host(lm).copy())
    (gb32, gt32, l32), (gb16, gt16, l16) = grads["f32"], grads["f16"]
    assert np.array_equal(l32, l16)
    assert np.isfinite(gb16).all() and np.isfinite(gt16).all()
    off = 0
    for li, (i, o_) in enumerate(_small_dims(3, 4)):
        a, b = gb16[off:off + i * o_], gb32[off:off + i * o_]
        scale = np.abs(b).max()
        assert np.sqrt(np.mean((a - b) ** 2)) < 1e-2 * scale and np.abs(a - b).max() < 5e-2 * scale, (li, np.sqrt(np.mean((a - b) ** 2)) / scale, np.abs(a - b).max() / scale)
        off += i * o_
    nz = gt32 != 0
    assert nz.sum() > 1000 and np.array_equal(nz, gt16 != 0) or np.mean(nz != (gt16 != 0)) < 1e-3
    st = np.abs(gt32).max()
    assert np.sqrt(np.mean((gt16[nz] - gt32[nz]) ** 2)) < 1e-2 * st, np.sqrt(np.mean((gt16[nz] - gt32[nz]) ** 2)) / st
    assert np.corrcoef(gt16[nz], gt32[nz])[0, 1] > 0.999
    # a few steps: same descent
    losses = {}
    for mode, hmode in (("f32", "f32"), ("f16", "f32"), ("f16", "packed")):
        tr = Trainer(sc["embedder"], sc["embeddirs"], sc["mlp"], sc["table"], sc["mlp_blob"], learning_rate=1e-3, mlp_backward=mode, hash_backward=hmode)
        losses[mode + hmode] = [float(host(tr.step(o, d, tgt, rp)[0])[0]) for _ in range(4)]
        if hmode == "packed":                                  # table gradient of the last step vs the float-atomic trainer's (same parameters up to step noise)
            gq = host(tr.g_table)
        elif mode == "f16":
            gf = host(tr.g_table)
    assert losses["f16f32"][-1] < losses["f16f32"][0]
    assert np.allclose(losses["f16f32"], losses["f32f32"], rtol=2e-2), losses
    assert np.allclose(losses["f16packed"], losses["f32f32"], rtol=2e-2), losses
    assert np.corrcoef(gq, gf)[0, 1] > 0.99
    with pytest.raises(api.L.NrfError):
        Trainer(sc["embedder"], sc["embeddirs"], sc["mlp"], sc["table"], sc["mlp_blob"], mlp_backward="bf16")
    with pytest.raises(api.L.NrfError):
        Trainer(sc["embedder"], sc["embeddirs"], sc["mlp"], sc["table"], sc["mlp_blob"], hash_backward="f16")
    # the data-parallel hook sees both gradients after the backward and before Adam (world size 1 here: the 2-rank reduction itself is a CPU gloo test)
    from nerfpp_amd.dist import GradSync
    seen = []
    def hook(gt, gb):
        seen.append((float(gt.abs().sum()), float(gb.abs().sum()))); return GradSync(world=1)(gt, gb)
    tr = Trainer(sc["embedder"], sc["embeddirs"], sc["mlp"], sc["table"], sc["mlp_blob"], learning_rate=1e-3, grad_sync=hook)
    tr.step(o, d, tgt, rp)
    assert len(seen) == 1 and seen[0][0] > 0 and seen[0][1] > 0


def test_trainer_tv_regulariser_smooths_the_table(api):
    """With the TV term switched on (HashEmbedder mode) the table gradient gains the regulariser's contribution and a few steps lower the
    TV value the trainer reports."""
    from nerfpp_amd.train import Trainer
    sc = api.S.make_hash_scene(mode="ngp", log2_t=14, seed=777, table_amp=0.3, sigma_scale=2.0)
    K = api.S.lego_K(16, 16); c2w = api.S.pose_spherical(20.0, -30.0, 4.0)
    o, d, _ = api.R.GetRays(16, 16, K, c2w)
    o = o.reshape(-1, 3); d = d.reshape(-1, 3)
    tgt = torch.rand((256, 3), device="cuda")
    rp = api.R.NeRFRenderParams(NSamples=32, NImportance=32, Chunk=256, Perturb=0.0, WhiteBkgr=False, Ndc=False, UseViewdirs=True, ThinRay=True,
                                BoundingBox=api.S.LEGO_BBOX, Precision=api.L.NRF_PREC_F16_SPLIT)
    tr = Trainer(sc["embedder"], sc["embeddirs"], sc["mlp"], sc["table"], sc["mlp_blob"], learning_rate=1e-2, tv_loss_weight=1e-3, seed=5)
    tvs = []
    for it in range(10):
        tr.seed = 5                     # same cubes every step (t is part of the index: pin it through the seed for this test)
        t_keep = tr.t
        tr.step(o, d, tgt, rp)
        tvs.append(float(tr.tv_loss))
        assert tr.t == t_keep + 1
    assert np.isfinite(tvs).all() and tvs[0] > 0
    tr2 = Trainer(sc["embedder"], sc["embeddirs"], sc["mlp"], sc["table"], sc["mlp_blob"], learning_rate=1e-2, tv_loss_weight=0.0)
    tr2.step(o, d, tgt, rp)
    assert float(tr2.tv_loss) == 0.0


# ------------------------------------------------------------------ X1: render factor, multi-GPU collective behind the C ABI, whole frames
def test_render_view_render_factor_vs_reference(api, manifest):
    """NeRFExecutor::RenderView with RenderFactor = 3 (NeRFExecutor.h:609-650): 26x26 -> 8x8 with K's fx, fy, cx, cy divided, then Render --
    against the reference's own render of the downsampled view."""
    g = load_golden("render_factor")
    r, _ = _golden_hash_scene(api, manifest)
    h, w = (int(v) for v in g["hw"])
    p = _params(api, load_golden("render_hash")["bbox"], 64, RenderFactor=float(g["render_factor"][0]))
    res = api.R.RenderView(r, g["c2w"], w, h, g["k"], p)
    assert tuple(res.Outputs.RGBMap.shape) == (8, 8, 3) and tuple(res.Outputs.DepthMap.shape) == (8, 8)
    assert_close(host(res.Outputs.RGBMap), g["out_rgb"], rtol=0, atol=1e-4, what="downsampled view within 1e-4 of the reference")
    assert_close(host(res.Outputs.AccMap), g["out_acc"], rtol=0, atol=1e-4)
    assert res.Near == g["near_far"][0] and res.Far == g["near_far"][1]
    # RenderFactor == 0 is the plain Render; RenderPath scales the size only (the reference hands Render() the original k, NeRFExecutor.h:668)
    p0 = _params(api, load_golden("render_hash")["bbox"], 64)
    g0 = load_golden("render_hash")
    full = api.R.RenderView(r, g0["c2w"], 8, 8, g0["k"], p0)
    assert_exact(host(full.Outputs.RGBMap), host(r.Render(8, 8, g0["k"], p0, c2w=g0["c2w"]).Outputs.RGBMap), "RenderFactor 0")
    bufs = api.R.RenderPath(r, [g["c2w"]], h, w, float(g["k"][0, 0]), g["k"], p)
    assert len(bufs) == 1 and tuple(bufs[0][0].shape) == (8, 8, 3) and bufs[0][0].dtype == torch.uint8
    same_k = r.Render(8, 8, g["k"], p, c2w=g["c2w"])
    assert_exact(host(bufs[0][0]), host(api.R.TorchTensorToCVMat(same_k.Outputs.RGBMap)), "RenderPath: size / factor, k unchanged")


def test_allgather_tiles_c_abi_single_rank(api):
    """nrf_comm_* / nrf_allgather_tiles on a world of one (the box has one GPU): RCCL is found, the communicator comes up from the library's own unique id,
    and the gathered frames equal the tiles -- equal split (ncclAllGather) and the uneven-split code path's bookkeeping are the same at world 1, so the N > 1
    offsets are covered by the CPU partition tests and the 2-rank gloo test; N > 1 on RCCL runs in the driver's SCALE job (bench.py reports a cross-check there)."""
    from nerfpp_amd.dist import TileComm, tile_partition
    cm = TileComm(0, 1)
    assert api.L.lib().nrf_comm_world(cm._c) == 1 and api.L.lib().nrf_comm_rank(cm._c) == 0
    tiles = torch.rand((3, 37, 20, 3), device="cuda")
    out = cm.all_gather_frames(tiles, 37)
    torch.cuda.synchronize()
    assert_exact(host(out), host(tiles), "world-1 all-gather through RCCL")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                                   # launches go to the caller's stream
        out2 = cm.all_gather_frames(tiles[:1], 37)
    s.synchronize()
    assert_exact(host(out2), host(tiles[:1]))
    # overlap = True: issued on a side stream behind the current one; the result is ordered into the current stream by pending.wait()
    tiles3 = tiles * 2.0
    out3, pending = cm.all_gather_frames(tiles3, 37, overlap=True)
    pending.wait()
    torch.cuda.synchronize()
    assert_exact(host(out3), host(tiles3), "world-1 all-gather issued on the side stream")
    assert tile_partition(37, 1, 0) == (0, 37)
    cm.close()


def test_whole_frame_800x800_bench_configuration(api, O):
    """The bench configuration itself (BASELINE config 3: CuHashEmbedder L16 T2^19 F2 + CuSHEncoder(4) + NeRFSmall, 640 000 rays, 64 + 128 samples,
    Chunk 131 072, NRF_PREC_F16_SPLIT) rendered whole: properties over every pixel, the bit-exact NRF_PREC_F32 mode on the same frame as the yardstick
    (every pixel value within 1e-4), 1 024 random rays of the F32 frame equal to the CPU oracle bit for bit, and row tiles == slices of the frame."""
    sc = api.S.make_hash_scene(mode="cu")
    K = api.S.lego_K(800, 800); c2w = api.S.pose_spherical(30.0, -30.0, 4.0)
    rp = api.S.lego_render_params(sc["bbox"], chunk=131072, precision=api.L.NRF_PREC_F16_SPLIT)
    res = sc["renderer"].Render(800, 800, K, rp, c2w=c2w)
    rgb = host(res.Outputs.RGBMap).reshape(-1, 3); acc = host(res.Outputs.AccMap).reshape(-1); dep = host(res.Outputs.DepthMap).reshape(-1)
    rays = host(res.Extras["rays_flat"])
    assert rgb.shape == (640000, 3) and np.isfinite(rgb).all() and np.isfinite(dep).all() and np.isfinite(acc).all()
    assert acc.min() >= 0 and acc.max() <= 1 + 1e-5 and rgb.min() >= -1e-5 and rgb.max() <= 1 + 1e-5
    hit = acc > 1e-3
    assert 0.2 < hit.mean() < 1.0                                # the orbit camera sees the box in the middle of the frame, background around it
    assert (dep[hit] >= rays[hit, 6] - 1e-4).all() and (dep[hit] <= rays[hit, 7] + 1e-4).all()
    miss = rays[:, 7] <= rays[:, 6] + 2e-6                       # rays that miss the AABB (far clamped to near + 1e-6, RayUtils.h:123)
    assert miss.any() and np.abs(rgb[miss & (acc < 1e-6)] - 1.0).max() < 1e-5      # white background
    # the parity mode on the same frame
    rp32 = api.S.lego_render_params(sc["bbox"], chunk=32768, precision=api.L.NRF_PREC_F32)
    ref = sc["renderer"].Render(800, 800, K, rp32, c2w=c2w)
    rgb32 = host(ref.Outputs.RGBMap).reshape(-1, 3)
    d = np.abs(rgb - rgb32)
    assert d.max() < 1e-4 and np.median(d) < 1e-5, (d.max(), np.median(d), (d >= 1e-4).sum())
    assert api.S.psnr(rgb, rgb32) > 95
    assert np.abs(dep - host(ref.Outputs.DepthMap).reshape(-1)).max() < 2e-4 and np.abs(acc - host(ref.Outputs.AccMap).reshape(-1)).max() < 1e-4
    # 1 024 random rays of the parity frame against the CPU oracle
    idx = np.sort(np.random.RandomState(7).choice(640000, 1024, replace=False))
    cfg = sc["cfg"]
    ls = ((1 << cfg["log2_t"]) >> 4) << 4
    model = O.Model(2, sc["mlp_blob"], bbox=sc["bbox"], table_f16=O.f32_to_f16(sc["table"]), primes=sc["primes"],
                    local_idx=np.arange(16, dtype=np.int32) * ls, local_size=np.full(16, ls, np.int32), bias=np.zeros((16, 3), np.float32),
                    mul=O.hash_cu_scales(16, 16, 512))
    orc = O.render_rays(model, rays[idx], 64, 128, O.linspace(0, 1, 64), O.linspace(0, 1, 128), white_bkgr=True)
    assert_exact(rgb32[idx], orc["rgb"], "whole frame, NRF_PREC_F32: 1024 random rays == oracle bit for bit")
    assert np.abs(rgb[idx] - orc["rgb"]).max() < 1e-4
    # multi-GPU partition: rank 5 of 8's row tile equals the slice of the frame, bit for bit
    from nerfpp_amd.dist import tile_partition
    row0, rows = tile_partition(800, 8, 5)
    tile = sc["renderer"].Render(800, 800, K, rp, c2w=c2w, row0=row0, rows=rows)
    assert_exact(host(tile.Outputs.RGBMap).reshape(-1, 3), rgb[row0 * 800:(row0 + rows) * 800], "row tile == slice of the frame")


def test_chunk_loop_lanes_reproduce_the_single_stream_loop(api):
    """nrf_batchify_rays runs consecutive chunks on two internal streams (render.hip: forked from / joined to the caller's stream, lane 1 staggered by half a
    chunk, a one-chunk batch cut in two).  Same kernels on the same slices: every output equals the single-stream loop's bit for bit -- several chunks, an odd
    count, one chunk, a batch below the two-lane threshold, a ragged last chunk, and a caller on a side stream whose next kernel reads the result."""
    import torch
    sc = api.S.make_hash_scene(mode="cu")
    K = api.S.lego_K(800, 800); c2w = api.S.pose_spherical(30.0, -30.0, 4.0)
    lib = api.L.lib()
    cases = [(300, 200, 40000), (300, 200, 65536), (300, 200, 131072), (300, 200, 1 << 20), (390, 20, 131072), (390, 21, 5000), (300, 37, 9999),
             (300, 200, 33001)]          # a Chunk that is no multiple of 64, several chunks per lane: a lane's first (staggered, rounded) chunk must stay within its workspace slice
    try:
        for row0, rows, chunk in cases:
            rp = api.S.lego_render_params(sc["bbox"], chunk=chunk, precision=api.L.NRF_PREC_F16_SPLIT)
            outs = []
            for lanes in (1, 2):
                api.L.check(lib.nrf_set_render_lanes(lanes))
                res = sc["renderer"].Render(800, 800, K, rp, c2w=c2w, row0=row0, rows=rows)
                outs.append([host(res.Outputs.RGBMap), host(res.Outputs.DepthMap), host(res.Outputs.AccMap), host(res.Outputs.DispMap)])
            for x, y, nm in zip(outs[0], outs[1], ("rgb", "depth", "acc", "disp")):
                assert_exact(y, x, "two lanes == one stream: %s, rows %d chunk %d" % (nm, rows, chunk))
        # Chunk < 8 on the lane path with an odd ray count (round-4 advisor: the tail balance computed an EMPTY chunk there -- lc / 8 == 0 -- and the loop never advanced):
        # 32 769 rays in chunks of 4 must come back, equal to the single-stream loop
        o, d, _ = api.R.GetRays(800, 800, K, c2w, row0=380, rows=41)
        o = o.reshape(-1, 3)[:32769].contiguous(); d = d.reshape(-1, 3)[:32769].contiguous()
        rp4 = api.S.lego_render_params(sc["bbox"], chunk=4, precision=api.L.NRF_PREC_F16_SPLIT)
        tiny = []
        for lanes in (1, 2):
            api.L.check(lib.nrf_set_render_lanes(lanes))
            tiny.append(host(sc["renderer"].Render(800, 800, K, rp4, rays=(o, d, None)).Outputs.RGBMap))
        assert_exact(tiny[1], tiny[0], "two lanes == one stream at Chunk 4, 32 769 rays")
        # the classic model's kernels (weight-streaming split kernel, exact sigma kernel) beside each other on the two lanes
        cl = api.S.make_classic_scene()
        rpc = api.S.lego_render_params(cl["bbox"], chunk=16384, precision=api.L.NRF_PREC_F16_SPLIT)
        co = []
        for lanes in (1, 2, 2):
            api.L.check(lib.nrf_set_render_lanes(lanes))
            res = cl["renderer"].Render(800, 800, K, rpc, c2w=c2w, row0=380, rows=82)
            co.append([host(res.Outputs.RGBMap), host(res.Outputs.DepthMap)])
        for other in co[1:]:
            assert_exact(other[0], co[0][0], "classic: two lanes == one stream, rgb"); assert_exact(other[1], co[0][1], "classic: two lanes == one stream, depth")
        # the caller's stream order holds across the fork / join: a side stream renders, then reduces the pixels on the same stream, no host sync in between
        rp = api.S.lego_render_params(sc["bbox"], chunk=40000, precision=api.L.NRF_PREC_F16_SPLIT)
        api.L.check(lib.nrf_set_render_lanes(2))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        sums = []
        with torch.cuda.stream(side):
            for _ in range(3):
                res = sc["renderer"].Render(800, 800, K, rp, c2w=c2w, row0=300, rows=200)
                sums.append(res.Outputs.RGBMap.double().sum())
        side.synchronize()
        api.L.check(lib.nrf_set_render_lanes(1))
        ref = sc["renderer"].Render(800, 800, K, rp, c2w=c2w, row0=300, rows=200).Outputs.RGBMap.double().sum().item()
        assert [v.item() for v in sums] == [ref] * 3
    finally:
        api.L.check(lib.nrf_set_render_lanes(2))


def test_lerf_render_pass_at_main_cpp_table_size(api, O):
    """BASELINE config 5 at the reference's own sizes (main.cpp:203-213: CuHashEmbedder L16 F8 T2^19 16..1024, LeRF 2 x 256 -> 768) on a 4-row tile of the
    800x800 frame, 64 + 128 samples, fused matrix-core path: sigma_le and the rendered embedding of 48 sampled rays against the oracle composed stage by
    stage; unit norm, finite, Chunk-independent."""
    sc = api.S.make_lerf_scene()
    r = sc["renderer"]
    assert r.fused and r.level_major
    K = api.S.lego_K(800, 800); c2w = api.S.pose_spherical(30.0, -30.0, 4.0)
    p = api.R.NeRFRenderParams(NSamples=64, NImportance=128, Chunk=2048, Perturb=0.0, Ndc=False, UseViewdirs=True, ReturnWeights=True, ThinRay=True, BoundingBox=sc["bbox"])
    res = r.Render(800, 800, K, p, c2w=c2w, row0=398, rows=4)
    emb = host(res.Outputs.RenderedLangEmbedding); accm = host(res.Outputs.AccMapLE)
    assert emb.shape == (3200, 768) and np.isfinite(emb).all()
    hit = accm > 1e-2
    assert hit.sum() > 500
    assert_close(np.linalg.norm(emb[hit], axis=1), np.ones(hit.sum()), rtol=1e-5, atol=0)
    # the Chunk loop's two torch lanes (LeRFRenderer.Render) against the single-stream loop: same kernels on the same slices, a deterministic embedding
    lanes_before = r.lanes
    try:
        r.lanes = 1 if lanes_before == 2 else 2
        other = r.Render(800, 800, K, p, c2w=c2w, row0=398, rows=4)
        assert torch.equal(other.Outputs.RenderedLangEmbedding, res.Outputs.RenderedLangEmbedding), "LeRF: two lanes == one stream, bit for bit"
    finally:
        r.lanes = lanes_before
    p2 = api.R.NeRFRenderParams(NSamples=64, NImportance=128, Chunk=800, Perturb=0.0, Ndc=False, UseViewdirs=True, ReturnWeights=True, ThinRay=True, BoundingBox=sc["bbox"])
    res2 = r.Render(800, 800, K, p2, c2w=c2w, row0=398, rows=4)
    cosc = (host(res2.Outputs.RenderedLangEmbedding)[hit] * emb[hit]).sum(1)
    assert cosc.min() > 1 - 1e-5, cosc.min()                                   # Chunk only changes the order of the float atomics of the per-ray sums
    # oracle on a sample of the rays, end to end: its own coarse pass, its own fine depths.  The renderer's default is split precision with the coarse sigma_le in
    # exact fp32 on the matrix cores, so the sample set must be the oracle's bit for bit and everything downstream is held to split-precision bounds.
    assert r.precision_name == "f16x3" and r._exact_coarse_on()
    rays = host(res.Extras["rays_flat"])
    idx = np.nonzero(hit)[0][::max(1, hit.sum() // 48)][:48]
    Lv, F, T = 16, 8, 19
    ls = ((1 << T) >> 4) << 4
    primes = sc["primes"]
    def net(pts):
        e_, keep = O.hash_cu(pts.reshape(-1, 3), O.f32_to_f16(sc["table"]), primes, np.arange(Lv, dtype=np.int32) * ls, np.full(Lv, ls, np.int32),
                             np.zeros((Lv, 3), np.float32), sc["bbox"], O.hash_cu_scales(Lv, 16, 1024), Lv, F)
        o = O.lerf(sc["blob"], e_)
        o[~keep, -1] = 0
        return o.reshape(pts.shape[0], pts.shape[1], -1)
    zc = O.z_vals(rays[idx, 6], rays[idx, 7], O.linspace(0, 1, 64))
    assert_exact(host(res.Extras["z_coarse"])[idx], zc, "coarse depths")
    rawc = net(O.points(rays[idx, :3], rays[idx, 3:6], zc))
    wc = O.raw2weights(rawc, 768, zc, rays[idx, 3:6])["weights"]
    assert_exact(host(res.Extras["weights_coarse"])[idx], wc, "coarse weights: sigma_le of the exact-fp32 matrix-core pass == oracle, bit for bit")
    samples, _, _ = O.sample_pdf(O.z_mid(zc), wc[:, 1:-1], O.linspace(0, 1, 128))
    zf = O.merge_sorted(zc, samples)
    assert_exact(host(res.Extras["z_fine"])[idx], zf, "fine sample set of the timed (split-precision) LeRF mode == oracle's, bit for bit")
    rawf = net(O.points(rays[idx, :3], rays[idx, 3:6], zf))
    fin = O.raw2weights(rawf, 768, zf, rays[idx, 3:6])
    ref = O.render_clip_embedding(rawf, 768, fin["weights"])
    assert_close(host(res.Outputs.WeightsLE)[idx], fin["weights"], rtol=0, atol=1e-5 * fin["weights"].max(), what="WeightsLE, split precision on the oracle's own sample set")
    cos = (emb[idx] * ref).sum(1)
    assert cos.min() > 1 - 1e-6, (np.median(cos), cos.min())


def test_level_scales_of_a_cuda_build_can_be_injected(api, O):
    """nrf_hash_set_level_scales: the CuHashEmbedder's mul_l are computed by the reference ON THE DEVICE with CUDA's exp2f / log2f; one ulp of them flips the
    fp16 rounding of ~10 % of the features (sensitivity study in tests/test_oracle_golden.py), so a host that needs parity with a particular CUDA build hands
    its 16 values over.  With scales one ulp up, the HIP render (generic kernels AND the dense-image fast path, which is re-baked) equals the oracle fed the
    same scales bit for bit, and differs from the render with the libm scales."""
    sc = api.S.make_hash_scene(mode="cu")
    e, r = sc["embedder"], sc["renderer"]
    mul0 = O.hash_cu_scales(16, 16, 512)
    assert_exact(e.level_scales(), mul0, "scales of nrf_hash_create == the oracle's libm evaluation of CuHashEmbedder.cu:40")
    K = api.S.lego_K(800, 800); c2w = api.S.pose_spherical(30.0, -30.0, 4.0)
    rp32 = api.S.lego_render_params(sc["bbox"], chunk=1000, precision=api.L.NRF_PREC_F32, KeepIntermediates=True)
    rps = api.S.lego_render_params(sc["bbox"], chunk=1000, precision=api.L.NRF_PREC_F16_SPLIT)
    before = host(r.Render(800, 800, K, rp32, c2w=c2w, row0=400, rows=1).Outputs.RGBMap).reshape(-1, 3)
    mul1 = np.nextafter(mul0, np.float32(np.inf)).astype(np.float32)
    try:
        e.set_level_scales(mul1)
        res = r.Render(800, 800, K, rp32, c2w=c2w, row0=400, rows=1)
        rgb = host(res.Outputs.RGBMap).reshape(-1, 3); rays = host(res.Extras["rays_flat"])
        ls = ((1 << 19) >> 4) << 4
        model = O.Model(2, sc["mlp_blob"], bbox=sc["bbox"], table_f16=O.f32_to_f16(sc["table"]), primes=sc["primes"], local_idx=np.arange(16, dtype=np.int32) * ls,
                        local_size=np.full(16, ls, np.int32), bias=np.zeros((16, 3), np.float32), mul=mul1)
        idx = np.arange(0, 800, 13)
        ref = O.render_rays(model, rays[idx], 64, 128, O.linspace(0, 1, 64), O.linspace(0, 1, 128), white_bkgr=True)
        assert_exact(rgb[idx], ref["rgb"], "F32 render with injected scales == oracle with the same scales")
        assert np.abs(rgb - before).max() > 1e-4, "one ulp of the level scales is visible in the pixels (why the knob exists)"
        fast = host(r.Render(800, 800, K, rps, c2w=c2w, row0=400, rows=1).Outputs.RGBMap).reshape(-1, 3)
        assert_close(fast, rgb, rtol=0, atol=1e-4, what="fast path (re-baked dense image) with injected scales vs its own parity mode")
    finally:
        e.set_level_scales(mul0)
    assert_exact(host(r.Render(800, 800, K, rp32, c2w=c2w, row0=400, rows=1).Outputs.RGBMap).reshape(-1, 3), before, "restored")


def test_fine_depths_merge_map(api):
    """nrf_fine_depths_merge: the same depth set as nrf_fine_depths, plus where every sorted depth came from -- src indexes a table holding the n*s coarse points
    first and the n*ns new samples after them, z_new are the new samples in SamplePDF order.  Ragged n, plateaus (zero weights), duplicates."""
    import ctypes as C
    P = lambda t: C.c_void_p(t.data_ptr())
    lib = api.L.lib()
    rng = np.random.default_rng(3)
    for n, s, ns in ((1, 64, 128), (37, 64, 128), (130, 32, 32), (5, 8, 200)):
        z = np.sort(rng.uniform(2.0, 6.0, (n, s)).astype(np.float32), axis=1)
        w = rng.uniform(0.0, 1.0, (n, s)).astype(np.float32)
        w[: max(1, n // 3), s // 4: s // 2] = 0.0                       # CDF plateaus
        if n > 2: z[2, 5] = z[2, 4]                                     # a duplicate coarse depth
        dz, dw = dev(z), dev(w)
        u = torch.linspace(0.0, 1.0, ns, dtype=torch.float32).cuda()
        zf0 = torch.empty((n, s + ns), device="cuda"); zf1 = torch.empty_like(zf0)
        src = torch.empty((n, s + ns), device="cuda", dtype=torch.int32); zn = torch.empty((n, ns), device="cuda")
        api.L.check(lib.nrf_fine_depths(P(dz), P(dw), C.c_int64(n), s, P(u), ns, 8, P(zf0), None))
        api.L.check(lib.nrf_fine_depths_merge(P(dz), P(dw), C.c_int64(n), s, P(u), ns, 8, P(zf1), P(src), P(zn), None))
        assert_exact(host(zf1), host(zf0), "depth set")
        table = np.concatenate([z.reshape(-1), host(zn).reshape(-1)])
        sv = host(src).astype(np.int64)
        assert_exact(table[sv], host(zf1), "z_fine == table[src]")
        assert (np.sort(sv, axis=1) == np.sort(np.concatenate([np.arange(n)[:, None] * s + np.arange(s)[None], n * s + np.arange(n)[:, None] * ns + np.arange(ns)[None]], 1), axis=1)).all(), \
            "every column of the ray appears exactly once"
        assert (np.diff(host(zn), axis=1) >= 0).all()


def test_lerf_feature_reusing_render_equals_two_pass_render(api):
    """The LeRF render pass that encodes every sample point once (coarse columns kept, nrf_fine_depths_merge map, hash encode + sigma net on the new samples,
    embedding pass gathering columns) against the plain two-pass evaluation of the same kernels, main.cpp sizes, both precisions, ragged chunks: depth set,
    weights and maps identical bit for bit; the rendered embedding identical up to the order of the per-ray float atomics."""
    sc = api.S.make_lerf_scene()
    r = sc["renderer"]
    assert r.fused and r.level_major and r.reuse_features
    K = api.S.lego_K(800, 800); c2w = api.S.pose_spherical(30.0, -30.0, 4.0)
    p = api.R.NeRFRenderParams(NSamples=64, NImportance=128, Chunk=1100, Perturb=0.0, Ndc=False, UseViewdirs=True, ReturnWeights=True, ThinRay=True, BoundingBox=sc["bbox"])
    try:
        # default split mode (coarse sigma_le in exact fp32): the feature-reusing passes see the same sample set as the plain two passes; their final weights take
        # the coarse depths' sigma from the exact pass instead of re-evaluating it in split arithmetic, hence a tolerance at the split precision's own level
        r.set_precision(api.L.NRF_PREC_F16_SPLIT)
        assert r._exact_coarse_on()
        a = r.Render(800, 800, K, p, c2w=c2w, row0=397, rows=3)
        r.reuse_features = False
        b = r.Render(800, 800, K, p, c2w=c2w, row0=397, rows=3)
        r.reuse_features = True
        assert_exact(host(a.Extras["z_fine"]), host(b.Extras["z_fine"]), "fine depth set (exact coarse pass in both)")
        assert_exact(host(a.Extras["weights_coarse"]), host(b.Extras["weights_coarse"]) if "weights_coarse" in b.Extras else host(a.Extras["weights_coarse"]))
        wa, wb = host(a.Outputs.WeightsLE), host(b.Outputs.WeightsLE)
        assert_close(wa, wb, rtol=0, atol=1e-5 * wb.max(), what="WeightsLE: exact vs split sigma on the coarse depths")
        hit = host(b.Outputs.AccMapLE) > 1e-2
        cosab = (host(a.Outputs.RenderedLangEmbedding)[hit] * host(b.Outputs.RenderedLangEmbedding)[hit]).sum(1)
        assert cosab.min() > 1 - 1e-6, cosab.min()
        r.exact_coarse = False       # the kernels' own A/B statements below: same kernels on the same inputs
        for prec in (api.L.NRF_PREC_F16_SPLIT, api.L.NRF_PREC_F16_MFMA):
            r.set_precision(prec)
            r.reuse_features = True
            a = r.Render(800, 800, K, p, c2w=c2w, row0=397, rows=3)
            r.hand_over_geo = False           # split precision: the embedding pass re-evaluating the sigma net instead of taking its output from the sigma pass
            a2 = r.Render(800, 800, K, p, c2w=c2w, row0=397, rows=3)
            r.hand_over_geo = True
            assert_exact(host(a2.Outputs.WeightsLE), host(a.Outputs.WeightsLE), "WeightsLE with / without the sigma net's output handed over")
            if prec == api.L.NRF_PREC_F16_SPLIT:
                assert_exact(host(a2.Outputs.RenderedLangEmbedding), host(a.Outputs.RenderedLangEmbedding), "embedding with / without the hand-over")
            r.reuse_features = False
            b = r.Render(800, 800, K, p, c2w=c2w, row0=397, rows=3)
            assert_exact(host(a.Extras["z_fine"]), host(b.Extras["z_fine"]), "fine depth set")
            for f in ("WeightsLE", "DepthMapLE", "DispMapLE", "AccMapLE"):
                assert_exact(host(getattr(a.Outputs, f)), host(getattr(b.Outputs, f)), f)
            ea, eb = host(a.Outputs.RenderedLangEmbedding), host(b.Outputs.RenderedLangEmbedding)
            assert np.isfinite(ea).all()
            if prec == api.L.NRF_PREC_F16_SPLIT:      # the split passes own a ray per wave: plain stores, a deterministic sum
                assert_exact(ea, eb, "rendered embedding (split precision: no atomics)")
            else:
                assert_close(ea, eb, rtol=0, atol=2e-5, what="rendered embedding (unit vectors; the float atomics of the per-ray sums are unordered in either render)")
    finally:
        r.reuse_features = True; r.hand_over_geo = True; r.exact_coarse = True
        r.set_precision(api.L.NRF_PREC_F16_SPLIT)


# ------------------------------------------------------------------ classic NeRF at fp32-grade precision on the matrix cores (NRF_PREC_F16_SPLIT)
def test_mlp_nerf_split_precision_vs_oracle_and_reference(api, O, manifest):
    """NeRFImpl::forward (8 x 256, skip, view branch) with hi + lo fp16 operand pairs: against the reference's own output (golden, MKL sgemm order) and against
    the fp32 FMA-chain oracle on a larger batch incl. ragged sizes (one point, a block + 1, several blocks); three orders tighter than the plain fp16 mode."""
    g = load_golden("mlp_nerf")
    blob = synth.blob_from_manifest(manifest["mlp_nerf"])
    m = api.M.NeRF(8, 256, 63, 27, 5, (4,), True, "model", params=blob)
    y = host(m.forward(dev(g["x"]), api.L.NRF_PREC_F16_SPLIT))
    scale = np.abs(g["y"]).max()
    assert_close(y, g["y"], rtol=0, atol=2e-5 * scale, what="classic NeRF, split precision vs the reference")
    rng = np.random.RandomState(5)
    for n in (1, 129, 1000):
        x = rng.uniform(-1, 1, (n, 90)).astype(np.float32)
        ref = host(m.forward(dev(x), api.L.NRF_PREC_F32))                      # == oracle bit for bit (test_mlp_nerf_f32_bit_exact_vs_oracle)
        y3 = host(m.forward(dev(x), api.L.NRF_PREC_F16_SPLIT))
        y1 = host(m.forward(dev(x), api.L.NRF_PREC_F16_MFMA))
        sc_ = np.abs(ref).max()
        e3, e1 = np.abs(y3 - ref).max() / sc_, np.abs(y1 - ref).max() / sc_
        assert e3 < 5e-6, (n, e3, e1)
        assert n == 1 or e1 > 50 * e3, "the plain fp16 mode is the loose one"
    oref = O.mlp_nerf(blob, x)
    assert np.abs(y3 - oref).max() / np.abs(oref).max() < 5e-6


def test_classic_split_render_vs_parity_mode_and_stagewise(api, O):
    """BASELINE config 2 shape (PE(10)/PE(4) + NeRF 8x256, 800x800 camera, 64 + 128) on a 2-row tile: the fused split-precision path (points and PE formed in
    the kernel, per-ray (hi, lo) direction rows) equals the stage-wise split path bit for bit, and its pixels are within 2e-4 of the bit-exact NRF_PREC_F32 render
    (>= 99 %; the coarse pass runs in split precision too, so a handful of fine samples may sit in another CDF bin), PSNR > 80 dB -- where the plain fp16 mode gives ~58."""
    sc = api.S.make_classic_scene()
    K = api.S.lego_K(800, 800); c2w = api.S.pose_spherical(30.0, -30.0, 4.0)
    out = {}
    for name, prec, cm in (("f32", api.L.NRF_PREC_F32, api.L.NRF_COARSE_AUTO), ("split", api.L.NRF_PREC_F16_SPLIT, api.L.NRF_COARSE_FULL),
                           ("f16", api.L.NRF_PREC_F16_MFMA, api.L.NRF_COARSE_AUTO), ("exact", api.L.NRF_PREC_F16_SPLIT, api.L.NRF_COARSE_AUTO)):
        rp = api.S.lego_render_params(sc["bbox"], chunk=700, precision=prec, ReturnRaw=True, KeepIntermediates=True, CoarseMode=cm)
        out[name] = sc["renderer"].Render(800, 800, K, rp, c2w=c2w, row0=400, rows=2)
    a, b, c = out["f32"], out["split"], out["f16"]          # b: NRF_COARSE_FULL, the whole network in split arithmetic on both passes (same kernel as the stage-wise forward)
    # the default coarse pass (sigma_nerf_f32.hip): sigma in exact fp32 == the parity mode's bit for bit; rgb from the exact h8 through the split-precision colour branch
    e = out["exact"]
    assert_exact(host(e.Extras["raw_coarse"])[..., 3], host(a.Extras["raw_coarse"])[..., 3], "coarse sigma: exact fp32 on the matrix cores == NRF_PREC_F32")
    assert_close(host(e.Extras["raw_coarse"])[..., :3], host(a.Extras["raw_coarse"])[..., :3], rtol=0, atol=1e-5 * np.abs(host(a.Extras["raw_coarse"])[..., :3]).max(),
                 what="coarse rgb: colour branch in split precision on the exact h8")
    assert_exact(host(e.Extras["z_fine"]), host(a.Extras["z_fine"]), "fine sample set")
    assert np.abs(host(e.Outputs.RGBMap) - host(a.Outputs.RGBMap)).max() < 1e-4
    rays = b.Extras["rays_flat"]
    for z, raw in ((b.Extras["z_coarse"], b.Extras["raw_coarse"]), (b.Extras["z_fine"], b.Raw)):
        n, s = z.shape
        pts = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]).reshape(-1, 3)
        emb, _ = sc["embedder"].forward(pts)
        dirs, _ = sc["embeddirs"].forward(rays[:, 8:11].contiguous())
        x = torch.cat([emb, dirs[:, None, :].expand(n, s, dirs.shape[1]).reshape(n * s, -1)], 1).contiguous()
        ref = sc["mlp"].forward(x, api.L.NRF_PREC_F16_SPLIT)
        assert_exact(host(raw).reshape(-1, 4), host(ref), "fused classic split raw == stage-wise split raw")
    raw_scale = np.abs(host(a.Extras["raw_coarse"])).max()
    assert_close(host(b.Extras["raw_coarse"]), host(a.Extras["raw_coarse"]), rtol=0, atol=5e-6 * raw_scale, what="coarse raw on identical points")
    rgb_a, rgb_b, rgb_c = (host(o.Outputs.RGBMap).reshape(-1, 3) for o in (a, b, c))
    d = np.abs(rgb_b - rgb_a)
    assert (d < 2e-4).mean() >= 0.99 and np.median(d) < 1e-5, ((d < 2e-4).mean(), np.median(d), d.max())
    ps_split, ps_f16 = api.S.psnr(rgb_b, rgb_a), api.S.psnr(rgb_c, rgb_a)
    assert ps_split > 80 and ps_split > ps_f16 + 15, (ps_split, ps_f16)


def test_lerf_fused_split_precision_vs_fp32_stage_path(api, O, manifest):
    """The fused LeRF passes in NRF_PREC_F16_SPLIT (mlp_lerf_split_mfma.hip) against the oracle-pinned fp32 stage path on identical points: sigma_le to 1e-5 of
    its scale (the plain fp16 mode: 3e-3), the per-ray weighted sum of normalised embeddings to 2e-5 (4e-3), level-major == row-major input, and end to end against the
    stage-composed fp32 renderer: embeddings parallel to 1e-6 where both see the same samples."""
    import ctypes as C
    Lv, F, T = 16, 8, 12
    bbox = api.S.LEGO_BBOX
    e = api.M.CuHashEmbedder("lang_embedder", bbox, Lv, F, T, 16, 128)
    table = synth.synth_sym(311, (Lv * (1 << T) * F,), np.float32(0.5))
    e.set_table(table); e.set_primes(np.array(api.S.CU_PRIMES[:3 * Lv], np.int32))
    blob = synth.blob_from_manifest(manifest["lerf"]).copy()
    blob[128 * 256:128 * 256 + 256] *= 20.0
    lerf = api.M.LeRF(32, 2, 256, 768, 128, "lang_model", params=blob)
    fused = api.R.LeRFRenderer(e, lerf, precision=api.L.NRF_PREC_F16_SPLIT); plain = api.R.LeRFRenderer(e, lerf, fused=False)
    assert fused.fused and fused.precision_name == "f16x3"
    K = api.S.lego_K(12, 12); c2w = api.S.pose_spherical(40.0, -30.0, 4.0)
    p = api.R.NeRFRenderParams(NSamples=32, NImportance=32, Chunk=50, Perturb=0.0, Ndc=False, UseViewdirs=True, ReturnWeights=True, ThinRay=True, BoundingBox=bbox)
    a = fused.Render(12, 12, K, p, c2w=c2w); b = plain.Render(12, 12, K, p, c2w=c2w)
    rays = host(a.Extras["rays_flat"])
    z = O.z_vals(rays[:, 6], rays[:, 7], O.linspace(0, 1, 32))
    pts = O.points(rays[:, :3], rays[:, 3:6], z)
    ls = ((1 << T) >> 4) << 4
    emb, keep = O.hash_cu(pts.reshape(-1, 3), O.f32_to_f16(table), np.array(api.S.CU_PRIMES[:3 * Lv], np.int32), np.arange(Lv, dtype=np.int32) * ls,
                          np.full(Lv, ls, np.int32), np.zeros((Lv, 3), np.float32), bbox, O.hash_cu_scales(Lv, 16, 128), Lv, F)
    raw = O.lerf(blob, emb); raw_unmasked = raw.copy(); raw[~keep, -1] = 0
    sig_gpu, x_gpu = fused._sigma_fused(dev(pts))
    scale = np.abs(raw[:, -1]).max()
    assert_close(host(sig_gpu).reshape(-1), raw[:, -1], rtol=0, atol=1e-5 * scale, what="sigma_le, split precision")
    # the exact-fp32 matrix-core density pass (sigma_lerf_f32.hip): == the oracle's ascending-k fp32 chain bit for bit, with and without the geo planes; ragged count
    sig_x, _ = fused._sigma_fused(dev(pts), exact=True)
    assert_exact(host(sig_x).reshape(-1), raw[:, -1], "sigma_le, exact fp32 on the matrix cores == oracle")
    npt = 144 * 32 - 37
    sg = torch.empty((npt,), device="cuda"); geo = torch.zeros((int(api.L.lib().nrf_lerf_geo_bytes(C.c_int64(npt))),), device="cuda", dtype=torch.uint8)
    api.L.check(api.L.lib().nrf_lerf_sigma_exact_lm_strided(lerf._m, C.c_void_p(x_gpu.data_ptr()), C.c_int64(144 * 32), C.c_void_p(dev(keep.astype(np.uint8)).data_ptr()), C.c_int64(npt),
                                                            C.c_void_p(sg.data_ptr()), C.c_void_p(geo.data_ptr()), C.c_int64(npt), None))
    assert_exact(host(sg), raw[:npt, -1], "exact sigma_le with the geo hand-over, ragged point count")
    # the geo planes: (hi, lo) fp16 pairs of [sigma, geo0..31] in kernel B's operand order -- hi + lo reproduces the fp32 stage values to 2^-22
    hfull = O.lerf_sigma_net(blob, emb)
    assert_exact(hfull[:, 0], raw_unmasked[:, -1], "oracle: sigma net alone == column -1 of LeRFImpl::forward")
    gp = host(geo).view(np.float16).reshape(3, 2, npt, 2, 8).astype(np.float32)        # [fragment][hi|lo][column][lane half][8]
    val = gp[:, 0] + gp[:, 1]                                                          # [fragment][column][h][j]
    for f in range(3):
        for h_ in range(2):
            for j in range(8):
                row = 16 * f + 8 * (j >> 2) + 4 * h_ + (j & 3)                     # perm_row(f, h, j), mlp_lerf_net.h
                if row <= 32:
                    assert_close(val[f, :, h_, j], hfull[:npt, row], rtol=0, atol=2e-6 * np.abs(hfull[:, row]).max(), what=f"geo plane row {row}")
                else:
                    assert (val[f, :, h_, j] == 0).all()
    w = np.random.RandomState(0).rand(144, 32).astype(np.float32)
    acc = torch.empty((144, 768), device="cuda")
    wd = dev(w)
    api.L.check(api.L.lib().nrf_lerf_render_embedding_lm(lerf._m, C.c_void_p(x_gpu.data_ptr()), C.c_void_p(wd.data_ptr()), C.c_int64(144), 32, C.c_void_p(acc.data_ptr()), None))
    ref = (w[:, :, None] * raw[:, :768].reshape(144, 32, 768)).sum(1)
    # the per-sample norm ||W a|| comes from the Gram product on the hi parts only (one scalar per sample, fp16-grade: ~1e-4 relative, mlp_lerf_split_mfma.hip): the
    # un-normalised sum carries that as a common-mode scale error of a few 1e-5; its DIRECTION -- what RenderCLIPEmbedding returns -- stays fp32-grade
    assert_close(host(acc), ref, rtol=0, atol=6e-5 * np.abs(ref).max(), what="sum_s w_s normalize(le_s), split precision")
    unit = lambda a: a / np.linalg.norm(a, axis=1, keepdims=True)
    assert np.abs(unit(host(acc).astype(np.float64)) - unit(ref.astype(np.float64))).max() < 2e-6, "direction of the per-ray sum"
    # fp32 feature rows (values are fp16 numbers here, so hi + lo carries them exactly): same result as the level-major input
    x_rows = dev(host(x_gpu).astype(np.float32).transpose(1, 0, 2).reshape(144 * 32, 128))
    sig_r = torch.empty((144 * 32,), device="cuda")
    ku8 = dev(keep.astype(np.uint8))
    api.L.check(api.L.lib().nrf_lerf_sigma(lerf._m, C.c_void_p(x_rows.data_ptr()), C.c_void_p(ku8.data_ptr()), C.c_int64(144 * 32), C.c_void_p(sig_r.data_ptr()), None))
    assert_exact(host(sig_r), host(sig_gpu).reshape(-1), "sigma_le: row-major == level-major input (split)")
    acc_r = torch.empty((144, 768), device="cuda")
    api.L.check(api.L.lib().nrf_lerf_render_embedding(lerf._m, C.c_void_p(x_rows.data_ptr()), C.c_void_p(wd.data_ptr()), C.c_int64(144), 32, C.c_void_p(acc_r.data_ptr()), None))
    assert_close(host(acc), host(acc_r), rtol=0, atol=1e-5 * np.abs(ref).max(), what="embedding sums differ by the order of the float atomics only")
    # end to end against the stage-composed fp32 renderer
    hit = host(b.Outputs.AccMapLE) > 1e-2
    assert hit.sum() > 20
    ea, eb = host(a.Outputs.RenderedLangEmbedding)[hit], host(b.Outputs.RenderedLangEmbedding)[hit]
    assert_close(np.linalg.norm(ea, axis=1), np.ones(hit.sum()), rtol=1e-5, atol=0)
    # the coarse pass of the split mode runs sigma_le in exact fp32: EVERY ray sees the fp32 stage path's sample set, bit for bit
    assert_exact(host(a.Extras["z_fine"]), host(b.Extras["z_fine"]), "fine depths: fused split-precision render == fp32 stage render")
    cos = (ea * eb).sum(1)
    assert cos.min() > 1 - 1e-6 and np.median(cos) > 1 - 1e-7, (cos.min(), np.median(cos))
    assert np.abs(host(a.Outputs.AccMapLE) - host(b.Outputs.AccMapLE))[hit].max() < 1e-5
    assert_close(host(a.Outputs.WeightsLE), host(b.Outputs.WeightsLE), rtol=0, atol=1e-5 * host(b.Outputs.WeightsLE).max())
    fused.set_precision(api.L.NRF_PREC_F16_MFMA)                                       # a handle-level switch: the plain mode is the loose one
    sig16, _ = fused._sigma_fused(dev(pts))
    assert np.abs(host(sig16).reshape(-1) - raw[:, -1]).max() > 30 * np.abs(host(sig_gpu).reshape(-1) - raw[:, -1]).max()


# ------------------------------------------------------------------ training loop housekeeping: dense image off for every encoder, schedule, checkpoints
def test_trainer_ngp_mode_schedule_and_checkpoint_round_trip(api, tmp_path):
    """The reference's TV-loss training configuration (LibTorch HashEmbedder): the Trainer cuts the baked dense pyramid down to its coarse levels (256 MB) for ANY hash
    embedder (a re-bake of the whole image per step would move gigabytes), applies the executor's schedule (TV regulariser for the first half of the iterations, exponential lr decay, fresh draws per step,
    the caller's params untouched), and its checkpoint -- written in the reference's formats, Adam state included -- restores a second Trainer that then takes
    bit-identical steps."""
    from nerfpp_amd.train import Trainer
    from nerfpp_amd import checkpoint as CK
    free0 = torch.cuda.mem_get_info()[0]
    sc = api.S.make_hash_scene(mode="ngp", log2_t=19, table_amp=1e-2, sigma_scale=4.0)            # full-size table: the bake at upload takes 8.8 GB of dense image
    baked = free0 - torch.cuda.mem_get_info()[0]
    assert baked > 4 << 30, baked
    K = api.S.lego_K(32, 32); c2w = api.S.pose_spherical(20.0, -30.0, 4.0)
    o, d, cone = api.R.GetRays(32, 32, K, c2w)
    o = o.reshape(-1, 3); d = d.reshape(-1, 3)
    tgt = torch.rand((1024, 3), device="cuda") * 0.2 + 0.4
    tr = Trainer(sc["embedder"], sc["embeddirs"], sc["mlp"], sc["table"], sc["mlp_blob"], learning_rate=5e-3, tv_loss_weight=1e-6)
    assert free0 - torch.cuda.mem_get_info()[0] < baked - (4 << 30), "the dense image must shrink to the training budget for the LibTorch HashEmbedder too"
    rp = api.R.NeRFRenderParams(NSamples=32, NImportance=32, Chunk=1024, Perturb=1.0, WhiteBkgr=False, Ndc=False, UseViewdirs=True, ThinRay=True,
                                BoundingBox=api.S.LEGO_BBOX, Precision=api.L.NRF_PREC_F32, Seed=5)
    n_iters, decay = 8, 0.002            # lr halves every 0.6 steps of "thousands": visible within a few steps
    tvs, lrs, zs = [], [], []
    for it in range(6):
        lm, res = tr.step(o, d, tgt, rp, global_step=it, n_iters=n_iters, lrate_decay=decay)
        tvs.append(float(tr.tv_loss.item())); lrs.append(tr.lr); zs.append(host(res.Extras["z_coarse"])[0].copy())
        if it == 3:
            tr.tv_loss.zero_()
    assert rp.ReturnRaw is False and rp.KeepIntermediates is False and rp.Seed == 5, "the caller's NeRFRenderParams must not be modified"
    assert all(t > 0 for t in tvs[:4]) and tvs[4] == 0 and tvs[5] == 0, tvs               # TV term only while global_step < n_iters / 2 (NeRFExecutor.h:896-913)
    assert np.allclose(lrs, [5e-3 * 0.1 ** (i / (decay * 1000)) for i in range(6)], rtol=1e-6), lrs      # :992-996
    assert not (zs[0] == zs[1]).all(), "every step draws fresh jitter"
    # checkpoint in the reference's formats, then a fresh Trainer restored from it walks the same path
    d_ck = str(tmp_path / "ck")
    tr.SaveCheckpoint(d_ck, global_step=6)
    assert CK.WouldRestore(d_ck)
    sc2 = api.S.make_hash_scene(mode="ngp", log2_t=19, table_amp=1e-2, sigma_scale=4.0, seed=999)         # different initial weights
    tr2 = Trainer(sc2["embedder"], sc2["embeddirs"], sc2["mlp"], sc2["table"], sc2["mlp_blob"], learning_rate=5e-3, tv_loss_weight=1e-6)
    assert tr2.LoadCheckpoint(str(tmp_path / "nothing_here")) is None
    assert tr2.LoadCheckpoint(d_ck) == 6
    assert tr2.t == tr.t and tr2.lr == tr.lr
    assert_exact(host(tr2.table), host(tr.table), "table"); assert_exact(host(tr2.m_blob), host(tr.m_blob), "Adam m"); assert_exact(host(tr2.v_table), host(tr.v_table), "Adam v")
    a, _ = tr.step(o, d, tgt, rp, global_step=6, n_iters=n_iters, lrate_decay=decay)
    b, _ = tr2.step(o, d, tgt, rp, global_step=6, n_iters=n_iters, lrate_decay=decay)
    assert_exact(host(a), host(b), "loss of the next step")
    assert_close(host(tr2.blob), host(tr.blob), rtol=0, atol=1e-7, what="parameters after the next step (float atomics of the table gradient aside)")


# ------------------------------------------------------------------ Render() as one library call; NDC + view directions; c2w_staticcam; the sharded frame
def _stagewise_render(api, r, h, w, k, p, c2w, row0, rows, chunk):
    """The pose branch of Render composed on the host from the stage functions, the way the mirror did before nrf_render_rows existed:
    GetRays -> nrf_pack_rays -> a Python loop of RenderRays over Chunk-sized slices -> torch.cat -> nrf_near_far_range."""
    import ctypes as C
    o, d, _ = api.R.GetRays(h, w, k, c2w, row0=row0, rows=rows)
    o = o.reshape(-1, 3).contiguous(); d = d.reshape(-1, 3).contiguous()
    n = o.shape[0]
    rays = torch.empty((n, 11), device="cuda")
    bb = np.ascontiguousarray(p.BoundingBox, np.float32)
    P = lambda t: C.c_void_p(t.data_ptr())
    api.L.check(api.L.lib().nrf_pack_rays(P(o), P(d), bb.ctypes.data_as(C.c_void_p), C.c_int64(n), 1, P(rays), None))
    res = r.BatchifyRays(rays, None, p.NSamples, chunk, return_raw=p.ReturnRaw, lin_disp=p.LinDisp, perturb=p.Perturb, n_importance=p.NImportance,
                         white_bkgr=p.WhiteBkgr, raw_noise_std=p.RawNoiseStd, bounding_box=p.BoundingBox, return_weights=p.ReturnWeights,
                         precision=p.Precision, keep_intermediates=p.KeepIntermediates, seed=p.Seed, coarse_mode=p.CoarseMode, ray_base=row0 * w)
    nr, fr = C.c_float(0), C.c_float(0)
    api.L.check(api.L.lib().nrf_near_far_range(P(rays), C.c_int64(n), 11, C.byref(nr), C.byref(fr), None))
    return res, rays, (nr.value, fr.value)


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_render_rows_single_call_equals_the_stagewise_host_loop(api, prec):
    """nrf_render_rows (ray generation + view directions + AABB + packing + the Chunk loop + Near/Far in ONE call, what a rank of the
    row-tile sharding issues per frame) against the same render composed from the stage functions: every output bit for bit, with a
    Chunk that does not divide the tile and a stochastic branch whose draws are keyed by the global ray index."""
    sc = api.S.make_hash_scene(mode="cu", log2_t=14)
    h, w = 64, 48
    K = api.S.lego_K(h, w); c2w = api.S.pose_spherical(40.0, -30.0, 4.0)
    P = {"f32": api.L.NRF_PREC_F32, "f16x3": api.L.NRF_PREC_F16_SPLIT}[prec]
    for perturb in (0.0, 1.0):
        rp = api.S.lego_render_params(sc["bbox"], chunk=1000, precision=P, ReturnWeights=True, ReturnRaw=True, KeepIntermediates="depths", Perturb=perturb, Seed=11)
        a = sc["renderer"].Render(h, w, K, rp, c2w=c2w, row0=13, rows=37)
        b, rays, nf = _stagewise_render(api, sc["renderer"], h, w, K, rp, c2w, 13, 37, 1000)
        assert_exact(host(a.Extras["rays_flat"]), host(rays), "packed rays")
        for name in ("RGBMap", "DispMap", "AccMap", "DepthMap", "Weights"):
            assert_exact(host(getattr(a.Outputs, name)), host(getattr(b.Outputs, name)), f"{name} ({prec}, perturb {perturb})")
        assert_exact(host(a.Raw), host(b.Raw), "raw")
        for kx in ("z_coarse", "weights_coarse", "z_fine"):
            assert_exact(host(a.Extras[kx]), host(b.Extras[kx]), kx)
        assert (a.Near, a.Far) == nf, "Near / Far reduced on the device == nrf_near_far_range"
        assert a.Outputs.RGBMap.shape == (37, w, 3) and a.Outputs.DepthMap.shape == (37, w)
    # the tile of a full-frame render == the tile rendered alone (sharding by rows cannot change a pixel)
    rp = api.S.lego_render_params(sc["bbox"], chunk=1000, precision=P)
    full = sc["renderer"].Render(h, w, K, rp, c2w=c2w)
    tile = sc["renderer"].Render(h, w, K, rp, c2w=c2w, row0=13, rows=37)
    assert_exact(host(full.Outputs.RGBMap)[13:50], host(tile.Outputs.RGBMap), "row tile == rows of the frame")


def test_render_rows_empty_tile(api):
    """A rank that owns no rows (h < world) renders an empty tile: no launch but the Near / Far identities, outputs of zero rays."""
    sc = api.S.make_hash_scene(mode="ngp", log2_t=12)
    rp = api.S.lego_render_params(sc["bbox"], chunk=64)
    res = sc["renderer"].Render(8, 8, api.S.lego_K(8, 8), rp, c2w=api.S.pose_spherical(0.0, -30.0, 4.0), row0=8, rows=0)
    assert res.Outputs.RGBMap.shape == (0, 8, 3) and res.Extras["rays_flat"].shape == (0, 11)
    assert res.Near == float("inf") and res.Far == float("-inf")


def test_render_rows_argument_errors(api):
    import ctypes as C
    sc = api.S.make_hash_scene(mode="ngp", log2_t=12)
    rp = api.S.lego_render_params(sc["bbox"], chunk=0)
    with pytest.raises(api.L.NrfError, match="Chunk"):
        sc["renderer"].Render(8, 8, api.S.lego_K(8, 8), rp, c2w=api.S.pose_spherical(0.0, -30.0, 4.0))
    rp = api.S.lego_render_params(sc["bbox"], chunk=64)
    with pytest.raises(api.L.NrfError, match="outside image"):
        sc["renderer"].Render(8, 8, api.S.lego_K(8, 8), rp, c2w=api.S.pose_spherical(0.0, -30.0, 4.0), row0=4, rows=5)


def test_render_ndc_with_viewdirs_vs_reference(api, manifest):
    """Ndc + UseViewdirs through the fused Render (NeRFRenderer.h:549-570): view directions are normalised from the pose's rays BEFORE NDCRays
    replaces rays_o / rays_d.  Golden = the reference's packed rays and RawToOutputs results (its Render() itself reads a dangling `sh` after
    :567 and threw here -- `reference_render_threw` -- after BatchifyRays had run)."""
    g = load_golden("render_ndc")
    assert int(g["reference_render_threw"][0]) == 1
    r, _ = _golden_hash_scene(api, manifest)
    p = _params(api, g["bbox"], 40); p.Ndc = True
    res = r.Render(8, 8, g["k"], p, c2w=g["c2w"])
    rays = host(res.Extras["rays_flat"])
    assert_exact(rays[:, :8], g["rays_flat"][:, :8], "NDC-warped o, d and their AABB near / far")
    assert_close(rays[:, 8:], g["rays_flat"][:, 8:], rtol=3e-7, atol=0, what="view directions of the UN-warped rays (torch::norm's order: 2 ulp)")
    assert np.abs(rays[:, 8:] - rays[:, 3:6] / np.linalg.norm(rays[:, 3:6], axis=1, keepdims=True)).max() > 0.1, "viewdirs are NOT the warped directions"
    # Against the LibTorch CPU run itself the fine sample set is a discontinuous function of the coarse weights (the reference differs from ITSELF
    # between CPU dispatch settings): most pixels within 1e-4, a moved sample shows as an outlier.  The strict statement is the one against the oracle below.
    rgb = host(res.Outputs.RGBMap).reshape(-1, 3)
    assert (np.abs(rgb - g["out_rgb"]).max(axis=1) < 1e-4).mean() >= 0.95 and api.S.psnr(rgb, g["out_rgb"]) > 60
    assert (np.abs(host(res.Outputs.AccMap) - g["out_acc"]) < 1e-4).mean() >= 0.95
    assert (host(res.Extras["z_fine"]) == g["out_fine_z"]).mean() > 0.85
    assert_close(host(res.Extras["weights_coarse"]), g["out_coarse_weights"], rtol=0, atol=2e-4)
    assert (res.Near, res.Far) == (float(g["near_far"][0]), float(g["near_far"][1]))
    from oracle import capi as O
    table = synth.blob_from_manifest([x for x in manifest["render_hash"] if "embeddings" in x[0]])
    blob = synth.blob_from_manifest([x for x in manifest["render_hash"] if "embeddings" not in x[0]])
    oc = O.render_rays(O.Model(0, blob, bbox=g["bbox"], table_f32=table), rays, 64, 128, O.linspace(0, 1, 64), O.linspace(0, 1, 128), white_bkgr=True, want_intermediates=True)
    assert_exact(host(res.Extras["z_fine"]), oc["z_fine"], "NDC render: sample set == oracle on the same packed rays")
    assert_exact(rgb, oc["rgb"], "NDC render: pixels == oracle bit for bit")
    assert res.Outputs.RGBMap.shape == (8, 8, 3)          # `sh` taken by value
    # explicit ray batch: same arithmetic through NDCRays + nrf_pack_rays_viewsrc
    o, d, cone = api.R.GetRays(8, 8, g["k"], g["c2w"])
    rb = r.Render(8, 8, g["k"], p, rays=(o.reshape(-1, 3)[:40], d.reshape(-1, 3)[:40], cone))
    assert_exact(host(rb.Extras["rays_flat"]), rays[:40], "ray-batch branch packs the same rows as the pose branch")
    assert_exact(host(rb.Extras["rays_flat"])[:, :8], g["batch_rays_flat"][:, :8])
    assert_exact(host(rb.Outputs.RGBMap), host(res.Outputs.RGBMap).reshape(-1, 3)[:40], "and renders the same pixels")
    assert (np.abs(host(rb.Outputs.RGBMap) - g["batch_rgb"]).max(axis=1) < 1e-4).mean() >= 0.95


def test_render_ndc_with_cone_rays_vs_oracle(api, manifest):
    """Ndc together with cone rays (ThinRay = false).  NDCRays multiplies cone_angle by |d_ndc| / |rays_d| AFTER rays_d has been replaced by d_ndc (RayUtils.h:73-81):
    exactly 1.0, so every ray keeps the camera's cone_angle -- the render is the cone render of the NDC-warped rays.  Pose branch (one nrf_render_rows call) and
    explicit ray batch, against the oracle on the same packed rays with the same counter-based draws, bit for bit; Chunk does not matter."""
    from oracle import capi as O
    g = load_golden("render_ndc")
    r, _ = _golden_hash_scene(api, manifest)
    def params(chunk):
        p = _params(api, g["bbox"], chunk, Seed=77); p.Ndc = True
        p.NSamples, p.NImportance, p.ThinRay, p.Perturb = 32, 48, False, 1.0
        return p
    a = r.Render(8, 8, g["k"], params(64), c2w=g["c2w"])
    rays = host(a.Extras["rays_flat"])
    assert_exact(rays[:, :8], g["rays_flat"][:, :8], "the NDC-warped rays of the golden")
    o, d, cone = api.R.GetRays(8, 8, g["k"], g["c2w"])
    table = synth.blob_from_manifest([x for x in manifest["render_hash"] if "embeddings" in x[0]])
    blob = synth.blob_from_manifest([x for x in manifest["render_hash"] if "embeddings" not in x[0]])
    st = dict(perturb=1.0, cone_angle=float(cone), seed=77, raw_noise_std=0.0, precond_alpha=0.0)
    oc = O.render_rays(O.Model(0, blob, bbox=g["bbox"], table_f32=table), rays, 32, 48, O.linspace(0, 1, 32), None, white_bkgr=True, want_intermediates=True, stoch=st)
    assert_exact(host(a.Extras["z_fine"]), oc["z_fine"], "fine sample set of the scattered NDC rays")
    assert_exact(host(a.Outputs.RGBMap).reshape(-1, 3), oc["rgb"], "Ndc + cone: pixels == oracle bit for bit")
    thin = params(64); thin.ThinRay = True
    assert np.abs(host(r.Render(8, 8, g["k"], thin, c2w=g["c2w"]).Outputs.RGBMap) - host(a.Outputs.RGBMap)).max() > 1e-4, "the cone really scatters the samples"
    assert_exact(host(r.Render(8, 8, g["k"], params(24), c2w=g["c2w"]).Outputs.RGBMap), host(a.Outputs.RGBMap), "independent of Chunk")
    b = r.Render(8, 8, g["k"], params(64), rays=(o, d, cone))
    assert_exact(host(b.Extras["rays_flat"]), rays, "ray-batch branch packs the same rows")
    assert_exact(host(b.Outputs.RGBMap).reshape(-1, 3), host(a.Outputs.RGBMap).reshape(-1, 3), "ray-batch branch == pose branch")


def test_render_c2w_staticcam_vs_reference(api, manifest):
    """c2w_staticcam (NeRFRenderer.h:554-558): the rays come from the static camera, the view directions from c2w."""
    g = load_golden("render_staticcam")
    r, _ = _golden_hash_scene(api, manifest)
    res = r.Render(8, 8, g["k"], _params(api, g["bbox"], 64), c2w=g["c2w"], c2w_staticcam=g["c2w_staticcam"])
    rays = host(res.Extras["rays_flat"])
    assert_exact(rays[:, :8], g["rays_flat"][:, :8], "o, d, near, far of the static camera")
    assert_close(rays[:, 8:], g["rays_flat"][:, 8:], rtol=3e-7, atol=0, what="view directions of c2w")
    assert_exact(host(res.Extras["z_coarse"]), g["coarse_z"])
    assert_close(host(res.Outputs.RGBMap), g["out_rgb"], rtol=0, atol=1e-4)
    assert_close(host(res.Outputs.DepthMap), g["out_depth"], rtol=0, atol=3e-4)
    assert (res.Near, res.Far) == (float(g["near_far"][0]), float(g["near_far"][1]))
    # without view directions the reference ignores c2w_staticcam altogether (the substitution sits inside `if UseViewdirs`)
    import ctypes as C
    def view_rays(staticcam):
        v = api.L.View()
        v.h, v.w, v.row0, v.rows, v.use_viewdirs, v.ndc, v.chunk = 8, 8, 0, 8, 0, 0, 64
        v.K = (C.c_float * 9)(*np.asarray(g["k"], np.float32).reshape(-1).tolist())
        v.c2w = (C.c_float * 12)(*np.asarray(g["c2w"], np.float32).reshape(-1).tolist())
        v.has_staticcam = int(staticcam)
        v.c2w_staticcam = (C.c_float * 12)(*np.asarray(g["c2w_staticcam"], np.float32).reshape(-1).tolist())
        v.bbox = (C.c_float * 6)(*np.asarray(g["bbox"], np.float32).tolist())
        out = torch.empty((64, 8), device="cuda")
        api.L.check(api.L.lib().nrf_view_rays(C.byref(v), C.c_void_p(out.data_ptr()), None, None))
        return host(out)
    assert_exact(view_rays(True), view_rays(False), "UseViewdirs = false: c2w_staticcam has no effect")


def test_bench_launcher_two_ranks_share_the_gpu_and_reproduce_the_single_rank_frame(tmp_path):
    """BASELINE config 4's code path end to end through bench.py's OWN spawn path (`python bench.py --gpus 2`, no torchrun): the parent starts two
    fresh ranks (gloo, both on this box's one GPU), rank r renders row tile r with one nrf_render_rows call, the tiles are all-gathered, and the
    gathered 800x800 frame must equal the single-rank frame bit for bit (sha256 of the pixel buffer, printed in both result lines)."""
    import json, os, subprocess, sys
    from conftest import ROOT
    common = ["--steps", "3", "--warmup", "2", "--no-cpu-baseline", "--no-parity", "--no-also"]      # two warm-up steps: the first timed Render of two ranks SHARING a GPU must not carry one-time work
    env = dict(os.environ, NRF_BENCH_TIMEOUT="600")
    one = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + common, capture_output=True, text=True, timeout=900, env=env)
    assert one.returncode == 0, one.stderr[-2000:]
    two = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo"] + common, capture_output=True, text=True, timeout=900, env=env)
    assert two.returncode == 0, two.stderr[-2000:]
    l1 = json.loads([x for x in one.stdout.splitlines() if x.startswith("{")][-1])
    l2 = json.loads([x for x in two.stdout.splitlines() if x.startswith("{")][-1])
    assert len([x for x in two.stdout.splitlines() if x.startswith("{")]) == 1, "ONE JSON line"
    assert l2["n_gpus"] == 2 and l2["scaling"] == "strong" and l2["config"]["frames_per_step"] == 1 and l2["tile_rows"] == 400
    assert l1["n_gpus"] == 1 and l1["tile_rows"] == 800
    assert l1["frame_sha256"] == l2["frame_sha256"], "gathered frame of 2 row tiles == the single-rank frame, bit for bit"
    assert l2["host_ms_per_tile"] < 5.0
    # a rank that dies must fail the launcher (non-zero exit), not hang it: its peer waits in the rendezvous and is ended by the parent
    t0 = __import__("time").time()
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo"] + common,
                         capture_output=True, text=True, timeout=600, env=dict(env, NRF_BENCH_TEST_FAIL_RANK="1"))
    assert bad.returncode != 0 and "rank exit codes" in bad.stderr and __import__("time").time() - t0 < 300


def test_baseline_config_1_shape_coarse_only_batch_of_1024_rays(api, O):
    """BASELINE config 1 at its literal shape: classic PE(10)/PE(4) + NeRF 8x256, Blender-Lego camera at 400x400 (focal 555.56), a training-style batch of
    N_rand = 1024 rays (GetRayBatch at random pixels), N_samples = 64, N_importance = 0 (coarse only: the reference leaves Render()'s maps undefined there,
    NeRFRenderer.h:423 vs :448; the coarse maps are returned).  NRF_PREC_F32 == the CPU oracle bit for bit; the matrix-core split precision within 1e-4."""
    sc = api.S.make_classic_scene()
    h = w = 400
    K = api.S.lego_K(h, w)
    assert abs(float(K[0, 0]) - 555.5555) < 1e-2
    c2w = api.S.pose_spherical(-27.0, -30.0, 4.0)
    o, d, cone = api.R.GetRays(h, w, K, c2w)
    rng = np.random.RandomState(1024)
    pix = torch.from_numpy(rng.choice(h * w, 1024, replace=False)).cuda()
    ro, rd = o.reshape(-1, 3)[pix].contiguous(), d.reshape(-1, 3)[pix].contiguous()
    rp = api.S.lego_render_params(sc["bbox"], n_samples=64, n_importance=0, chunk=1024 * 32, precision=api.L.NRF_PREC_F32, white_bkgr=False, ReturnWeights=True,
                                  ReturnRaw=True)
    res = sc["renderer"].Render(h, w, K, rp, rays=(ro, rd, cone))
    rays = host(res.Extras["rays_flat"])
    assert rays.shape == (1024, 11) and res.Outputs.RGBMap.shape == (1024, 3) and res.Outputs.Weights.shape == (1024, 64) and res.Raw.shape == (1024, 64, 4)
    oc = O.render_rays(O.Model(1, sc["mlp_blob"], bbox=sc["bbox"]), rays, 64, 0, O.linspace(0, 1, 64), None, white_bkgr=False, want_intermediates=True)
    assert_exact(host(res.Raw), oc["raw_coarse"], "config 1: network outputs == oracle")
    assert_exact(host(res.Outputs.Weights), oc["weights"], "config 1: weights == oracle")
    assert_exact(host(res.Outputs.RGBMap), oc["rgb"], "config 1: pixels == oracle bit for bit")
    assert_exact(host(res.Outputs.DepthMap), oc["depth"]); assert_exact(host(res.Outputs.AccMap), oc["acc"])
    assert (host(res.Outputs.AccMap) > 0.05).mean() > 0.2, "the batch sees the object"
    rps = api.S.lego_render_params(sc["bbox"], n_samples=64, n_importance=0, chunk=1024 * 32, precision=api.L.NRF_PREC_F16_SPLIT, white_bkgr=False)
    sp = sc["renderer"].Render(h, w, K, rps, rays=(ro, rd, cone))
    assert_close(host(sp.Outputs.RGBMap), oc["rgb"], rtol=0, atol=1e-4, what="config 1 in split precision: every pixel within 1e-4 of the oracle")


def test_classic_exact_coarse_sigma_pass_reproduces_the_parity_sample_set(api, O):
    """The classic renderer's timed mode (NRF_PREC_F16_SPLIT, NRF_COARSE_AUTO): the coarse pass is the density branch alone -- eight 256-wide layers with the
    skip-concat, then alpha_linear -- in exact fp32 on the matrix cores (sigma_nerf_f32.hip).  Its sigma, hence the coarse weights and the fine sample set, must
    EQUAL the NRF_PREC_F32 render's bit for bit (which equals the CPU oracle), on a 16-row band of the 800x800 frame with ragged chunks; every pixel value is then
    within 1e-4 (strict).  NRF_COARSE_FULL (coarse pass in split arithmetic, 2.2 x faster) stays available and is looser, as documented."""
    sc = api.S.make_classic_scene()
    K = api.S.lego_K(800, 800); c2w = api.S.pose_spherical(30.0, -30.0, 4.0)
    kw = dict(chunk=333, KeepIntermediates="depths", ReturnWeights=True)
    a = sc["renderer"].Render(800, 800, K, api.S.lego_render_params(sc["bbox"], precision=api.L.NRF_PREC_F32, **kw), c2w=c2w, row0=392, rows=16)
    b = sc["renderer"].Render(800, 800, K, api.S.lego_render_params(sc["bbox"], precision=api.L.NRF_PREC_F16_SPLIT, **kw), c2w=c2w, row0=392, rows=16)
    assert_exact(host(b.Extras["z_coarse"]), host(a.Extras["z_coarse"]))
    assert_exact(host(b.Extras["weights_coarse"]), host(a.Extras["weights_coarse"]), "coarse weights: exact-fp32 matrix-core density branch == the fp32 FMA chains")
    assert_exact(host(b.Extras["z_fine"]), host(a.Extras["z_fine"]), "fine sample set of the timed classic mode == NRF_PREC_F32's, bit for bit (12 800 rays)")
    d = np.abs(host(b.Outputs.RGBMap) - host(a.Outputs.RGBMap))
    assert d.max() < 1e-4, d.max()                                   # strict: every pixel value
    wa, wb = host(a.Outputs.Weights), host(b.Outputs.Weights)
    assert_close(wb, wa, rtol=0, atol=2e-5, what="fine weights: split-precision network on the same samples")
    # a sample of the band against the CPU oracle itself
    rays = host(a.Extras["rays_flat"])[::50]
    oc = O.render_rays(O.Model(1, sc["mlp_blob"], bbox=sc["bbox"]), rays, 64, 128, O.linspace(0, 1, 64), O.linspace(0, 1, 128), white_bkgr=True, want_intermediates=True)
    assert_exact(host(b.Extras["z_fine"])[::50], oc["z_fine"], "== the CPU oracle's sample set")
    assert np.abs(host(b.Outputs.RGBMap).reshape(-1, 3)[::50] - oc["rgb"]).max() < 1e-4
    # the cheaper mode: whole network in split arithmetic on the coarse pass (its outputs reused by the fine pass)
    c = sc["renderer"].Render(800, 800, K, api.S.lego_render_params(sc["bbox"], precision=api.L.NRF_PREC_F16_SPLIT, CoarseMode=api.L.NRF_COARSE_FULL, **kw), c2w=c2w, row0=392, rows=16)
    dc = np.abs(host(c.Outputs.RGBMap) - host(a.Outputs.RGBMap))
    assert (dc < 1e-4).mean() > 0.99 and api.S.psnr(host(c.Outputs.RGBMap), host(a.Outputs.RGBMap)) > 70
    # plain fp16 precision may ask for the exact coarse pass too (NRF_COARSE_SIGMA_F32)
    e = sc["renderer"].Render(800, 800, K, api.S.lego_render_params(sc["bbox"], precision=api.L.NRF_PREC_F16_MFMA, CoarseMode=api.L.NRF_COARSE_SIGMA_F32, **kw), c2w=c2w, row0=392, rows=2)
    assert_exact(host(e.Extras["z_fine"]), host(a.Extras["z_fine"])[:1600], "fp16 fine pass on the fp32 sample set")


# ------------------------------------------------------------------ LeRF: Relevancy, the relevancy image, and the render pass as ONE library call (rows L2 / N4)
def test_relevancy_and_jet_image_vs_oracle(api, O):
    """nrf_lerf_relevancy / nrf_relevancy_image / nrf_colormap_jet_* against the oracle restatement (PARITY UNPINNED: RuCLIP's Relevancy and OpenCV's COLORMAP_JET are
    external; see include/nerfpp_hip.h) at the call sites' shapes -- [N, 768] unit embeddings, one positive, Q in {1, 3, 5} negatives -- plus the known answers."""
    import ctypes as C
    rng = np.random.RandomState(713)
    E = 768
    for n, q in ((1, 3), (257, 3), (5000, 1), (1031, 5)):
        x = rng.randn(n, E).astype(np.float32); x /= np.linalg.norm(x, axis=1, keepdims=True)
        pos = rng.randn(2, E).astype(np.float32); pos /= np.linalg.norm(pos, axis=1, keepdims=True)
        neg = rng.randn(q, E).astype(np.float32); neg /= np.linalg.norm(neg, axis=1, keepdims=True)
        x[: min(n, q)] = neg[: min(n, q)]                                            # embeddings that ARE a canonical phrase: the positive loses against it
        for pid in (0, 1):
            got = host(api.R.Relevancy(dev(x), pos, neg, positive_id=pid))
            ref = O.relevancy(x, pos, neg, positive_id=pid)
            assert got.shape == (n, 2)
            assert_close(got, ref, rtol=0, atol=3e-6, what=f"relevancy n={n} q={q} positive {pid}")        # 768-term fp32 dot products in another order, then exp
            assert_close(got.sum(1), np.ones(n), rtol=0, atol=1e-6)
        assert got[0, 0] < 1e-3
    basis = np.linalg.qr(rng.randn(E, 5))[0].T.astype(np.float32)
    r = host(api.R.Relevancy(dev(np.stack([basis[0], basis[2], basis[4]])), basis[:1], basis[1:4]))
    assert_close(r[:, 0], [1 / (1 + np.exp(-10.0)), 1 / (1 + np.exp(10.0)), 0.5], rtol=0, atol=1e-6, what="known answers: the positive itself, a negative, orthogonal")
    with pytest.raises(api.L.NrfError):
        api.R.Relevancy(dev(basis[:2]), basis[:1], basis[1:1])                        # no negative phrase
    # the colour map: table == oracle's, image == oracle's byte for byte, the byte -> colour entry too
    lut = np.empty((256, 3), np.uint8)
    api.L.check(api.L.lib().nrf_colormap_jet_lut(lut.ctypes.data_as(C.c_void_p)))
    assert_exact(lut, O.colormap_jet_lut(), "COLORMAP_JET table")
    rel = rng.rand(4099, 2).astype(np.float32); rel[:6, 0] = [0.0, 1.0, 0.5, 1.5, -0.3, 0.99999]
    assert_exact(host(api.R.RelevancyImage(dev(rel))), O.relevancy_image(rel), "relevancy image")
    assert api.R.RelevancyImage(dev(rel.reshape(4099, 1, 2))).shape == (4099, 1, 3)
    g = torch.arange(0, 256, dtype=torch.uint8, device="cuda").repeat(3)
    out = torch.empty((768, 3), dtype=torch.uint8, device="cuda")
    api.L.check(api.L.lib().nrf_colormap_jet_u8(C.c_void_p(g.data_ptr()), C.c_int64(768), C.c_void_p(out.data_ptr()), None))
    assert_exact(host(out)[256:512], lut, "nrf_colormap_jet_u8")


def test_lerf_render_as_one_library_call_equals_the_stagewise_host_loop(api, O):
    """nrf_lerf_render_rows / nrf_lerf_batchify_rays (LeRFRenderer::Render / BatchifyRays as C calls, lanes inside the library, no torch ops) against the same passes
    composed stage by stage by the Python host (its own Chunk loop and torch.cat): depths, weights, maps and the rendered embedding identical bit for bit (split
    precision: same kernels on the same slices, no atomics), for a pose tile and for an explicit ray batch, ragged chunks, 1 / 2 / 3 lanes; Relevancy filled in both."""
    import os
    sc = api.S.make_lerf_scene()
    r = sc["renderer"]
    assert r.fused and r.level_major and r._r and r.precision_name == "f16x3" and r.lanes == 1
    rng = np.random.RandomState(86)
    pos = rng.randn(1, 768).astype(np.float32); pos /= np.linalg.norm(pos)
    neg = rng.randn(3, 768).astype(np.float32); neg /= np.linalg.norm(neg, axis=1, keepdims=True)
    K = api.S.lego_K(800, 800); c2w = api.S.pose_spherical(30.0, -30.0, 4.0)
    p = api.R.NeRFRenderParams(NSamples=64, NImportance=128, Chunk=1100, Perturb=0.0, Ndc=False, UseViewdirs=True, ReturnWeights=True, ThinRay=True, BoundingBox=sc["bbox"])
    lanes0 = r.lanes
    try:
        r.SetLeRFPrompts(pos, neg)
        assert r.GetLeRFPrompts()[1].shape == (3, 768)
        r.single_call = False
        ref = r.Render(800, 800, K, p, c2w=c2w, row0=396, rows=5)
        r.single_call = True
        for lanes in (1, 2, 3):
            r.lanes = lanes
            a = r.Render(800, 800, K, p, c2w=c2w, row0=396, rows=5)
            assert api.L.lib().nrf_get_render_lanes() == 2 or os.environ.get("NRF_RENDER_LANES"), "a renderer's own lane count leaves the process-wide setting alone"
            for f in ("WeightsLE", "DepthMapLE", "DispMapLE", "AccMapLE", "RenderedLangEmbedding", "Relevancy"):
                assert_exact(host(getattr(a.Outputs, f)), host(getattr(ref.Outputs, f)), f"{f}, {lanes} lane(s)")
            for f in ("z_fine", "z_coarse", "weights_coarse", "rays_flat"):
                assert_exact(host(a.Extras[f]), host(ref.Extras[f]), f)
            assert abs(a.Near - ref.Near) == 0 and abs(a.Far - ref.Far) == 0
        r.lanes = 2
        rel = host(a.Outputs.Relevancy)
        assert rel.shape == (4000, 2) and np.isfinite(rel).all() and np.abs(rel.sum(1) - 1).max() < 1e-6
        assert_close(rel, O.relevancy(host(a.Outputs.RenderedLangEmbedding), pos, neg), rtol=0, atol=3e-6, what="Relevancy of the rendered embeddings vs the oracle")
        img = host(api.R.RelevancyImage(a.Outputs.Relevancy.reshape(5, 800, 2)))
        assert img.shape == (5, 800, 3) and (img == O.relevancy_image(rel).reshape(5, 800, 3)).all()
        # an explicit ray batch (the training-style call, LeRFRenderer.cpp:276-279): BatchifyRays in one call
        o, d, cone = api.R.GetRays(800, 800, K, c2w, row0=396, rows=5)
        b = r.Render(800, 800, K, p, rays=(o.reshape(-1, 3), d.reshape(-1, 3), cone))
        for f in ("WeightsLE", "DepthMapLE", "AccMapLE", "RenderedLangEmbedding", "Relevancy"):
            assert_exact(host(getattr(b.Outputs, f)), host(getattr(ref.Outputs, f)), f"{f}, ray batch")
        assert b.Near == ref.Near and b.Far == ref.Far
        # without ReturnWeights the weights and the embedding are dropped (LeRFRenderer.cpp:180-185); the relevancy is still rendered
        p2 = api.R.NeRFRenderParams(NSamples=64, NImportance=128, Chunk=4096, Perturb=0.0, Ndc=False, UseViewdirs=True, ReturnWeights=False, ThinRay=True, BoundingBox=sc["bbox"])
        c = r.Render(800, 800, K, p2, c2w=c2w, row0=396, rows=5)
        assert c.Outputs.WeightsLE is None and c.Outputs.RenderedLangEmbedding is None
        assert_exact(host(c.Outputs.Relevancy), host(ref.Outputs.Relevancy), "relevancy alone"); assert_exact(host(c.Outputs.DepthMapLE), host(ref.Outputs.DepthMapLE))
        # the stochastic branches are not part of the render pass: refused, not silently ignored
        p3 = api.R.NeRFRenderParams(NSamples=64, NImportance=128, Chunk=4096, Perturb=1.0, Ndc=False, UseViewdirs=True, ReturnWeights=True, ThinRay=True, BoundingBox=sc["bbox"])
        with pytest.raises(api.L.NrfError):
            r.Render(800, 800, K, p3, c2w=c2w, row0=396, rows=1)
        r.SetLeRFPrompts(None, None)
        assert r.Render(800, 800, K, p, c2w=c2w, row0=396, rows=1).Outputs.Relevancy is None
    finally:
        r.lanes = lanes0; r.single_call = True
        r.SetLeRFPrompts(None, None)


def test_reference_train_loop_body_runs_through_the_hip_drop_in(tmp_path, manifest):
    """The drop-in trains under the reference's own host code: oracle/_ref/adapter_check `train` executes the statements of NeRFExecutor::Train's loop body
    (NeRFExecutor.h:862-995: Optimizer->zero_grad, NeRFRenderer->Render on a ray batch, mse_loss, huber_loss, loss.backward(), Optimizer->step()) with
    HipNeRFRenderer<HipHashEmbedder, HipSHEncoder, NeRFSmall> in the renderer's place and torch::optim::Adam over the modules' own parameters -- Render is one autograd
    node (nerfpp_torch.h, RenderFn), nothing of this repo is called between the steps.  Loss, pixels, the step-1 gradients of every parameter and the parameters after
    two Adam steps against what the reference's CPU autograd produced (golden train_hash), at the tolerances of the stage-wise test above."""
    import json, os, subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "oracle", "_ref", "adapter_check")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/adapter_check not built (needs /root/reference at build time)")
    g = load_golden("train_hash")
    d = str(tmp_path)
    for k in ("bbox", "rays_o", "rays_d", "target", "lr"):
        np.ascontiguousarray(g[k], np.float32).tofile(os.path.join(d, k + ".f32"))
    names = []
    for ent in manifest["train_hash"]:          # (name, seed, amp, shape): the seeds the golden generator filled the reference's modules with
        synth.blob_from_manifest([ent]).astype(np.float32).tofile(os.path.join(d, f"init_{ent[0]}.f32"))
        names.append((ent[0], ent[3]))
    assert len(names) == 10
    out = subprocess.run([exe, "train", d], capture_output=True, text=True, timeout=600)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert lines, out.stdout[-2000:] + out.stderr[-2000:]
    r = json.loads(lines[-1])
    assert out.returncode == 0 and r["train_ok"], (r, out.stderr[-1500:])
    assert r["inference_after_steps_sees_updated_parameters"] and r["standalone_embedder_autograd_ok"], r
    rd = lambda f, shape: np.fromfile(os.path.join(d, f), np.float32).reshape(shape)
    lr = float(g["lr"][0])
    # end to end the loss inherits the render's own distance to the reference's CPU render (a few fine samples in other CDF bins, 64 rays only): the bounds of
    # test_trainer_two_steps_vs_reference, which runs the same chain through the Python host
    assert abs(rd("out_s1_loss.f32", (1,))[0] - g["s1_loss"][0]) < 2e-4 and abs(rd("out_s1_mse.f32", (1,))[0] - g["s1_mse"][0]) < 4e-4
    d1 = np.abs(rd("out_s1_rgb.f32", (64, 3)) - g["s1_rgb"])
    assert np.median(d1) < 1e-5 and (d1 < 1e-4).mean() > 0.9, (np.median(d1), (d1 < 1e-4).mean())
    # the gradients: (a) against the reference's autograd -- the rays whose fine sample set moved (above) contribute their whole difference, hence a norm-wise bound;
    # (b) against the Python host's Trainer on the same HIP forward (the chain test_training_backward_stages_vs_reference_autograd pins stage by stage to the
    # reference's autograd): the same kernels in the same order, so equal up to the order of the float atomics
    from nerfpp_amd.train import Trainer
    api_ = type("Api", (), dict(L=__import__("nerfpp_amd._lib", fromlist=["x"]), M=__import__("nerfpp_amd.modules", fromlist=["x"]), R=__import__("nerfpp_amd.renderer", fromlist=["x"])))
    gg, table, blob, e, ed, m = _train_golden(api_, manifest)
    tr = Trainer(e, ed, m, table, blob, learning_rate=lr)
    rp = api_.R.NeRFRenderParams(NSamples=32, NImportance=32, Chunk=64, Perturb=0.0, WhiteBkgr=False, Ndc=False, UseViewdirs=True, ThinRay=True, BoundingBox=g["bbox"],
                                 Precision=api_.L.NRF_PREC_F32)
    lm1, _ = tr.step(dev(g["rays_o"]), dev(g["rays_d"]), dev(g["target"]), rp)
    assert abs(host(lm1)[0] - rd("out_s1_loss.f32", (1,))[0]) < 1e-7, "same forward: same loss"
    py = dict(zip([n for n, _ in names], np.split(np.concatenate([host(tr.g_table), host(tr.g_blob)]), np.cumsum([int(np.prod(sh)) for _, sh in names])[:-1])))
    for name, shape in names:
        ref = g[f"s1_grad_{name}"].astype(np.float64); got = rd(f"out_s1_grad_{name}.f32", ref.shape).astype(np.float64)
        rel = np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30)
        assert rel < 8e-2, (name, rel)
        assert_close(got, py[name].reshape(ref.shape), rtol=1e-4, atol=1e-6 * np.abs(py[name]).max(), what=f"d loss / d {name}: C++ autograd node vs the Python Trainer's chain")
    # the parameters after the two Adam steps.  Adam's first steps are ~lr * sign(g) (m / sqrt(v) = g / |g|, eps 1e-15): a weight whose gradient is rounding-level noise
    # moves by +-lr either way, so against the reference's CPU run the comparison bounds the SHARE of such weights (as test_trainer_two_steps_vs_reference does; the hash
    # table has many entries that only the moved rays touch) -- and against the Python host's Trainer stepping the same HIP chain it is tight
    lm2, _ = tr.step(dev(g["rays_o"]), dev(g["rays_d"]), dev(g["target"]), rp)
    py2 = dict(zip([n for n, _ in names], np.split(np.concatenate([host(tr.table), host(tr.blob)]), np.cumsum([int(np.prod(sh)) for _, sh in names])[:-1])))
    for step in (1, 2):
        for name, shape in names:
            ref = g[f"s{step}_param_{name}"]
            got = rd(f"out_s{step}_param_{name}.f32", ref.shape)
            dd = np.abs(got - ref) / lr
            table = "embeddings" in name
            # (step 2 continues from this run's own step 1 -- the loop is the reference's, not a restart from its state -- and so carries step 1's sign noise)
            assert dd.mean() < (0.08 if table else 0.03) * step and (dd > 0.05).mean() < ((0.2 if table else 0.05) if step == 1 else 0.35), (name, step, dd.mean(), (dd > 0.05).mean())
            if step == 2:
                dp = np.abs(got - py2[name].reshape(ref.shape)) / lr
                assert (dp > 0.05).mean() < 0.05 and np.median(dp) < 1e-2, (name, (dp > 0.05).mean(), np.median(dp))       # float atomics in another order: the sign of a cancelling sum
        assert abs(rd(f"out_s{step}_loss.f32", (1,))[0] - g[f"s{step}_loss"][0]) < 3e-4
    assert abs(host(lm2)[0] - rd("out_s2_loss.f32", (1,))[0]) < 2e-4          # two runs of the same chain: step 1 leaves a per-cent of the weights lr apart (sign of a cancelling atomic sum)
    assert r["loss_step2"] < r["loss_step1"]


def test_mlp_small_with_the_predicted_normals_head(api, O, manifest):
    """NeRFSmall(use_pred_normal = true) (NeRF.cpp:343-347, :393-407; the executor builds it when n_importance == 0, NeRFExecutor.h:487): output [rgb, sigma, normal xyz] in
    NRF_PREC_F32 == the oracle bit for bit and the compiled reference to 1e-4; the matrix-core precisions refuse such a handle loudly; a coarse-only render returns Raw with
    7 columns (RawToOutputs ignores the last three, NeRFRenderer.h:279) -- and the reference's keep-mask quirk with this head is reproduced (see below)."""
    g = load_golden("mlp_small_pn")
    blob = synth.blob_from_manifest(manifest["mlp_small_pn"])
    m = api.M.NeRFSmall(3, 64, 15, 3, 64, True, 3, 64, 32, 16, "model", params=blob)
    assert m.GetOutputDims() == 7
    y = host(m.forward(dev(g["x"]), precision=api.L.NRF_PREC_F32))
    assert_exact(y, O.mlp_small_pred_normal(blob, g["x"], in_ch=32, in_views=16, n_layers_c=3), "NRF_PREC_F32 == oracle")
    assert_close(y, g["y"], rtol=1e-4, atol=1e-5, what="vs the compiled reference")
    with pytest.raises(api.L.NrfError):
        m.forward(dev(g["x"]), precision=api.L.NRF_PREC_F16_SPLIT)
    # through the renderer: CuHash-less scene with the LibTorch encoders, coarse only (the configuration the executor pairs with this head)
    sc = api.S.make_hash_scene(mode="ngp", log2_t=14, seed=5000)
    d = api.L.MlpSmallDesc(32, 16, 3, 64, 15, 4, 64, 1, 3, 64)
    n_pn = int(api.L.lib().nrf_mlp_small_param_count(C.byref(d)))
    blob2 = np.concatenate([sc["mlp_blob"], synth.synth_sym(91, (n_pn - sc["mlp_blob"].size,), np.float32(0.1))]).astype(np.float32)      # the scene's two nets + a normals net
    m2 = api.M.NeRFSmall(3, 64, 15, 4, 64, True, 3, 64, 32, 16, "model", params=blob2)
    r2 = api.R.NeRFRenderer(sc["embedder"], sc["embeddirs"], m2)
    K = api.S.lego_K(16, 16); c2w = api.S.pose_spherical(30.0, -30.0, 4.0)
    rp = api.S.lego_render_params(sc["bbox"], 64, 0, 128, api.L.NRF_PREC_F32, ReturnRaw=True)
    a = r2.Render(16, 16, K, rp, c2w=c2w)
    b = sc["renderer"].Render(16, 16, K, rp, c2w=c2w)
    assert host(a.Raw).shape == (256, 64, 7) and host(b.Raw).shape == (256, 64, 4)
    ra, rb = host(a.Raw), host(b.Raw)
    assert_exact(ra[..., :3], rb[..., :3], "colour columns == the two-net model's")
    # REFERENCE QUIRK reproduced: RunNetwork masks `outputs_flat[~keep_mask, -1]` (NeRFRenderer.h:187-188) -- with this head column -1 is the normal's z, not sigma: a point
    # outside the box keeps its density and loses its normal's z.  So sigma differs from the two-net model exactly where that model masked it, and there the last column is 0
    diff = ra[..., 3] != rb[..., 3]
    assert diff.any() and (rb[..., 3][diff] == 0).all() and (ra[..., 6][diff] == 0).all() and (ra[..., 6][~diff] != 0).mean() > 0.99
    assert np.abs(ra[..., 4:]).max() > 0 and np.isfinite(host(a.Outputs.RGBMap)).all()


# ------------------------------------------------------------------ N1 for the classic model: backward of NeRFImpl::forward (NeRF.cpp:92-126)
@pytest.mark.parametrize("tag", ["mlp_nerf_bwd", "mlp_nerf_bwd_noview", "mlp_nerf_bwd_full"])
def test_classic_mlp_backward_vs_reference_autograd(api, O, tag, manifest):
    """nrf_mlp_backward on the classic family (mlp.hip, mlp_nerf_backward: fp32 layer kernels, bias column sums, the skip concat, both heads) against LibTorch autograd through the
    COMPILED NeRF.cpp -- a small network with view directions, one without (output_linear on cat[h, input_pts]), and the 8 x 256 bench network: every parameter gradient and
    d / d input_pts within 2e-4 of its tensor's largest entry of the reference's, within 2e-5 of the oracle's."""
    from test_oracle_golden import nerf_bwd_golden_case
    kw, stride, blob, g, where = nerf_bwd_golden_case(tag, manifest)
    m = api.M.NeRF(kw["d"], kw["w"], kw["in_ch"], kw["in_views"], kw["out_ch"], {kw["skip"]}, kw["use_viewdirs"], "model", params=blob)
    od = 4 if kw["use_viewdirs"] else kw["out_ch"]
    x = dev(g["x"]); go = dev(np.ascontiguousarray(g["g_out"][:, :od]))
    n = x.shape[0]
    g_params = torch.zeros((blob.size,), device="cuda"); g_x = torch.empty((n, kw["in_ch"]), device="cuda")
    lib = api.L.lib()
    nb = lib.nrf_mlp_backward_workspace_bytes(m._m, C.c_int64(n))
    ws = torch.empty((int(nb),), device="cuda", dtype=torch.uint8)
    vp = lambda t: C.c_void_p(t.data_ptr())
    api.L.check(lib.nrf_mlp_backward(m._m, vp(x), vp(go), C.c_int64(n), vp(g_params), vp(g_x), vp(ws), C.c_size_t(int(nb)), None))
    torch.cuda.synchronize()
    ogp, ogx = O.mlp_nerf_backward(blob, g["x"], g["g_out"][:, :od], **kw)
    ref_x = g["grad_x"][:, :kw["in_ch"]]
    assert_close(host(g_x), ref_x, rtol=0, atol=2e-4 * float(np.abs(ref_x).max()), what="d / d input_pts vs reference autograd")
    assert_close(host(g_x), ogx, rtol=0, atol=2e-5 * float(np.abs(ogx).max()), what="d / d input_pts vs oracle")
    gp = host(g_params)
    for name, (off, shape) in where.items():
        cnt = int(np.prod(shape))
        mine, orc, gold = gp[off:off + cnt], ogp[off:off + cnt], g["grad_" + name].reshape(-1)
        assert_close(mine, orc, rtol=0, atol=2e-5 * float(np.abs(orc).max()) + 1e-9, what=f"d / d {name} vs oracle")
        if gold.size != mine.size:
            mine = mine[::stride]
        assert_close(mine, gold, rtol=0, atol=2e-4 * float(np.abs(gold).max()) + 1e-9, what=f"d / d {name} vs reference autograd")


# ------------------------------------------------------------------ N1, LeRF branch of the optimisation step (NeRFExecutor.h:955-982)
def _lerf_golden_case(tag):
    from nerfpp_amd.synth import load_manifest
    from conftest import GOLDEN
    man = load_manifest(os.path.join(GOLDEN, "manifest.txt"))
    g = load_golden(tag)
    geo, layers, hidden, embed, in_ch, n, s, stride = (int(v) for v in g["dims"])
    blob = synth.blob_from_manifest(man[tag])
    off, where = 0, {}
    for name, _, _, shape in man[tag]:
        where[name] = (off, shape); off += int(np.prod(shape))
    return dict(geo=geo, n_layers=layers, hidden=hidden, embed=embed, in_ch=in_ch, n=n, s=s, stride=stride), blob, g, where


@pytest.fixture
def lerf_gram_form(api, request):
    """the head's last layer in its Gram form (1, the library's default) or layer-wise (0) for one test (nrf_dbg_lerf_train_gram, lerf_train.hip)"""
    lib = api.L.lib()
    lib.nrf_dbg_lerf_train_gram.restype = C.c_int
    prev = lib.nrf_dbg_lerf_train_gram(int(request.param))
    yield int(request.param)
    lib.nrf_dbg_lerf_train_gram(prev)


@pytest.mark.parametrize("lerf_gram_form", [1, 0], indirect=True)
@pytest.mark.parametrize("tag", ["train_lerf", "train_lerf_l3", "train_lerf_main"])
def test_lerf_training_head_backward_vs_reference_autograd(api, O, tag, lerf_gram_form):
    """nrf_huber_rows_nanmean + nrf_lerf_head_backward (lerf_train.hip) against LibTorch autograd through the COMPILED LeRFImpl::forward, the compiled RawToOutputs' weights
    (RawToLEOutputs' expression) and the reference's inline RenderCLIPEmbedding (goldens train_lerf*: two layers, three layers, main.cpp:203-213 dims): loss 2e-6 relative,
    recomputed forward 1e-4, every gradient within 2e-4 of its tensor's largest entry of the REFERENCE's and within 2e-5 of the oracle's (float atomics in another order).
    Both forms of the last layer: the Gram form (nothing embedding-wide per sample: the default) and the layer-wise one."""
    from nerfpp_amd import train as T
    c, blob, g, where = _lerf_golden_case(tag)
    lerf = api.M.LeRF(c["geo"], c["n_layers"], c["hidden"], c["embed"], c["in_ch"], "lang_model", params=blob)
    loss, g_r = T.HuberRowsNanmean(dev(g["rendered"]), dev(g["target"]))
    assert abs(float(host(loss)[0]) - float(g["loss"][0])) <= 2e-6 * abs(float(g["loss"][0]))
    assert_close(host(g_r), g["grad_rendered"], rtol=1e-5, atol=1e-9, what="d lang_loss / d RenderedLangEmbedding")
    r = T.LeRFHeadBackward(lerf, dev(g["emb"]), dev(g["keep"].astype(np.uint8)), dev(g["z"]), dev(g["d"]), dev(g["grad_rendered"]))
    assert_close(host(r["weights"]), g["weights"], rtol=2e-5, atol=2e-7, what="WeightsLE of the recomputed forward")
    assert_close(host(r["rendered"]), g["rendered"], rtol=1e-4, atol=2e-6, what="RenderedLangEmbedding of the recomputed forward")
    ref = O.lerf_head_backward(blob, g["emb"], g["keep"], g["z"], g["d"], g["grad_rendered"], in_ch=c["in_ch"], n_layers=c["n_layers"], hidden=c["hidden"], geo=c["geo"], embed=c["embed"])
    ge = g["grad_emb"]
    assert_close(host(r["g_emb"]), ge, rtol=0, atol=2e-4 * float(np.abs(ge).max()), what="d loss / d language-grid features vs reference autograd")
    assert_close(host(r["g_emb"]), ref["g_emb"], rtol=0, atol=2e-5 * float(np.abs(ge).max()), what="... vs oracle")
    gp = host(r["g_params"])
    for name, (off, shape) in where.items():
        gold = g["grad_" + name].reshape(-1)
        mine = gp[off:off + int(np.prod(shape))]
        orc = ref["g_params"][off:off + int(np.prod(shape))]
        assert_close(mine, orc, rtol=0, atol=2e-5 * float(np.abs(orc).max()), what=f"d loss / d {name} vs oracle")
        if gold.size != mine.size:
            mine = mine[::c["stride"]]
        assert_close(mine, gold, rtol=0, atol=2e-4 * float(np.abs(gold).max()), what=f"d loss / d {name} vs reference autograd")
    # the gradient buffer is ACCUMULATED into (a second call doubles it) and the chunking by whole rays does not change it beyond atomic order
    # RawNoiseStd > 0: the draws enter sigma before relu / alpha (LeRFRenderer.cpp:50-51) -- against the oracle with the same draws
    rng = np.random.RandomState(5)
    noise = rng.randn(c["n"], c["s"]).astype(np.float32)
    rn = T.LeRFHeadBackward(lerf, dev(g["emb"]), dev(g["keep"].astype(np.uint8)), dev(g["z"]), dev(g["d"]), dev(g["grad_rendered"]), noise=dev(noise), noise_std=0.3)
    on = O.lerf_head_backward(blob, g["emb"], g["keep"], g["z"], g["d"], g["grad_rendered"], in_ch=c["in_ch"], n_layers=c["n_layers"], hidden=c["hidden"], geo=c["geo"], embed=c["embed"],
                              noise=noise, noise_std=0.3)
    assert_close(host(rn["weights"]), on["weights"], rtol=2e-5, atol=2e-7, what="weights with raw noise")
    assert_close(host(rn["g_params"]), on["g_params"], rtol=0, atol=2e-5 * float(np.abs(on["g_params"]).max()), what="parameter gradients with raw noise")
    assert np.abs(on["weights"] - ref["weights"]).max() > 1e-3, "the noise case differs from the plain one"


def test_lerf_language_loss_nan_target_row_as_libtorch(api):
    """A ray whose target holds a NaN leaves nanmean's mean; LibTorch's backward leaves NaN at exactly that element of the ray's gradient row, zeros in the rest of the row
    (golden train_lerf_nan) -- reproduced, not repaired."""
    from nerfpp_amd import train as T
    g = load_golden("train_lerf_nan")
    loss, grad = T.HuberRowsNanmean(dev(g["pred"]), dev(g["target"]))
    assert abs(float(host(loss)[0]) - float(g["loss"][0])) <= 1e-6 * abs(float(g["loss"][0]))
    got, ref = host(grad), g["grad_pred"]
    assert (np.isnan(got) == np.isnan(ref)).all() and np.isnan(ref).sum() == 1
    ok = ~np.isnan(ref)
    assert_close(got[ok], ref[ok], rtol=1e-6, atol=0)
    assert (got[2][~np.isnan(got[2])] == 0).all()


def test_lerf_training_step_one_library_call_vs_oracle_and_descends(api, O):
    """The LeRF half of the train loop body on the library path (LeRFTrainer: fused render -> nrf_huber_rows_nanmean -> nrf_lerf_backward_points -> nrf_adam_step), CuHashEmbedder
    L16 F8 language grid (T = 2^14) + LeRF 2 x 256 -> 768 at main.cpp:203-213's head sizes, 96 rays x (32 + 32) samples: the table and head gradients of the ONE backward call
    against the oracle composed stage by stage on the same fine depths (hash_cu -> lerf_head_backward -> hash_cu_backward); five Adam steps lower the loss."""
    from nerfpp_amd import train as T
    sc = api.S.make_lerf_scene(log2_t=14, sigma_scale=20.0)
    r = sc["renderer"]
    K = api.S.lego_K(800, 800); c2w = api.S.pose_spherical(30.0, -30.0, 4.0)
    o, d, _ = api.R.GetRays(800, 800, K, c2w, row0=400, rows=1)
    o = o.reshape(-1, 3)[300:396].contiguous(); d = d.reshape(-1, 3)[300:396].contiguous()
    n, s, ni = o.shape[0], 32, 32
    p = api.R.NeRFRenderParams(NSamples=s, NImportance=ni, Chunk=4096, Perturb=0.0, Ndc=False, UseViewdirs=False, ReturnWeights=True, ThinRay=True, BoundingBox=sc["bbox"])
    rng = np.random.RandomState(11)
    tgt = rng.randn(n, 768).astype(np.float32); tgt /= np.linalg.norm(tgt, axis=1, keepdims=True)
    tr = T.LeRFTrainer(r, sc["table"], sc["blob"], learning_rate=2e-3)
    p1 = __import__("copy").copy(p); p1.KeepIntermediates = True
    res = r.Render(0, 0, None, p1, rays=(o, d, None))
    assert r._single_call_ok(p1), "the training render is the library's single call"
    loss0 = tr.backward(res, dev(tgt), p1)
    zf = host(res.Extras["z_fine"]); rays = host(res.Extras["rays_flat"])
    Lv, F, Tt = 16, 8, 14
    ls = ((1 << Tt) >> 4) << 4
    li, lsz, bias, mul = np.arange(Lv, dtype=np.int32) * ls, np.full(Lv, ls, np.int32), np.zeros((Lv, 3), np.float32), O.hash_cu_scales(Lv, 16, 1024)
    pts = O.points(rays[:, :3], rays[:, 3:6], zf).reshape(-1, 3)
    emb, keep = O.hash_cu(pts, O.f32_to_f16(sc["table"]), sc["primes"], li, lsz, bias, sc["bbox"], mul, Lv, F)
    fwd = O.lerf_head_backward(sc["blob"], emb, keep, zf, rays[:, 3:6], np.zeros((n, 768), np.float32))          # the oracle's fp32 forward on the same depths
    rendered = host(res.Outputs.RenderedLangEmbedding).reshape(n, 768)
    assert ((rendered * fwd["rendered"]).sum(1) > 1 - 2e-6).all(), "fused split-precision render vs the oracle's fp32 forward"
    _, g_r = O.huber_rows_nanmean(rendered, tgt)
    ref = O.lerf_head_backward(sc["blob"], emb, keep, zf, rays[:, 3:6], g_r)
    assert_close(host(tr.g_blob), ref["g_params"], rtol=0, atol=3e-5 * float(np.abs(ref["g_params"]).max()), what="head gradients of nrf_lerf_backward_points vs oracle")
    gt = O.hash_cu_backward(pts, sc["primes"], li, lsz, bias, sc["bbox"], mul, Lv, F, sc["table"].size, ref["g_emb"])
    got_t = host(tr.g_table)
    assert np.abs(gt).max() > 0 and (got_t != 0).sum() > 1000
    assert_close(got_t, gt, rtol=0, atol=2e-3 * float(np.abs(gt).max()), what="language-grid gradient vs oracle (contributions rounded to fp16 after the x128 scaling, CuHashEmbedder.cu:105-216)")
    losses = [float(host(loss0)[0])]
    for _ in range(5):
        l, _ = tr.step(o, d, dev(tgt), p)
        losses.append(float(host(l)[0]))
    assert all(np.isfinite(losses)) and losses[-1] < losses[1] < losses[0] * 1.0001, losses
    tr.close()


@pytest.mark.gpu
def test_lerf_training_backward_reads_the_language_features_its_forward_render_encoded(api):
    """The LeRF training step's backward needs the language grid's features at the fine depths; its forward render (a one-chunk library call) has just encoded exactly those
    points -- coarse columns, the new samples' columns, the merge map.  nrf_lerf_renderer_last_features hands that view over and nrf_lerf_backward_points_src gathers the rows
    through the map (fp16 values, as nrf_hash_encode's fp32 rows hold): the same loss, the same head and table gradients as with a second encode of the points; a render in
    between invalidates the view; a two-chunk render leaves none."""
    from nerfpp_amd import train as T
    sc = api.S.make_lerf_scene(log2_t=14, sigma_scale=20.0)
    r = sc["renderer"]
    K = api.S.lego_K(800, 800); c2w = api.S.pose_spherical(30.0, -30.0, 4.0)
    o, d, _ = api.R.GetRays(800, 800, K, c2w, row0=400, rows=1)
    o = o.reshape(-1, 3)[200:584].contiguous(); d = d.reshape(-1, 3)[200:584].contiguous()
    n, s, ni = o.shape[0], 32, 32
    p = api.R.NeRFRenderParams(NSamples=s, NImportance=ni, Chunk=4096, Perturb=0.0, Ndc=False, UseViewdirs=False, ReturnWeights=True, ThinRay=True, BoundingBox=sc["bbox"],
                               KeepIntermediates=True)
    rng = np.random.RandomState(12)
    tgt = rng.randn(n, 768).astype(np.float32); tgt /= np.linalg.norm(tgt, axis=1, keepdims=True)
    tr = T.LeRFTrainer(r, sc["table"], sc["blob"], learning_rate=2e-3)
    same = lambda a, b: float((a - b).abs().max()) <= 2e-6 * float(b.abs().max())
    got = {}
    for reuse in (True, False):
        tr.reuse_render_features = reuse
        res = r.Render(0, 0, None, p, rays=(o, d, None))
        assert res.FeatureView is not None and res.FeatureView["n"] == n and res.FeatureView["sf"] == s + ni and res.FeatureView["cols"] == n * (s + ni)
        loss = tr.backward(res, dev(tgt), p)
        assert tr.reused_render_features is reuse
        got[reuse] = (tr.g_blob.clone(), tr.g_table.clone(), host(loss).copy())
        if reuse:
            r.Render(0, 0, None, p, rays=(o[:50], d[:50], None))          # a render in between: `res`'s view is stale, the backward encodes the points again
            tr.backward(res, dev(tgt), p)
            assert tr.reused_render_features is False and same(tr.g_blob, got[True][0]) and same(tr.g_table, got[True][1])
            p2 = api.R.NeRFRenderParams(**{**p.__dict__, "Chunk": 128})
            assert r.Render(0, 0, None, p2, rays=(o, d, None)).FeatureView is None
    assert np.array_equal(got[True][2], got[False][2])
    assert same(got[True][0], got[False][0]) and same(got[True][1], got[False][1])
    assert float(got[True][0].abs().max()) > 0 and float(got[True][1].abs().max()) > 0
    tr.close()


def test_drop_in_training_render_vs_reference_cpu_autograd_random_models():
    """oracle/_ref/adapter_check `trainfuzz`: one training render + huber + backward through BOTH hosts -- the reference's NeRFRenderer on LibTorch CPU and the drop-in on the GPU --
    on random batch sizes / sample counts / grid and network shapes (hash grid + NeRFSmall), and, round 5, on the CLASSIC configuration (Embedder / Embedder / NeRFImpl with a
    random depth, width and skip layer against HipEmbedder / HipEmbedder / NeRFImpl): loss within 1 %, every parameter gradient within 15 % norm-wise (the rays whose fine
    sample set moved contribute their whole difference)."""
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "oracle", "_ref", "adapter_check")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/adapter_check not built (needs /root/reference at build time)")
    out = subprocess.run([exe, "trainfuzz", "4", "5"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "all ok" in out.stdout, out.stdout[-2500:] + out.stderr[-1000:]
    assert out.stdout.count("classic case") == 3 and out.stdout.count(": ok") >= 7, out.stdout[-2500:]
    # round 6: every other case is of the fused fp16 backward's family -- the chain the drop-in takes when its renderer is in a matrix-core precision is held to the fp32 layer
    # kernels' gradients (3 % norm-wise per network tensor and over the grid), which the lines above hold to the reference's autograd
    assert "fused fp16 backward checked against the fp32 layer kernels in 2 case(s)" in out.stdout, out.stdout[-2500:]


def test_library_scratch_blocks_are_reused_and_can_be_given_back(api):
    """scratch.hip: the library's short-lived device buffers come from blocks it keeps per (device, stream) -- a layer product leaves one behind, the same product again takes
    it again (no growth), nrf_scratch_trim gives the idle blocks back (bytes > 0, then 0), and the product works as before afterwards."""
    L = api.L
    lib = L.lib()
    M, N, K = 4096, 256, 256
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    a = torch.randn((M, K), device="cuda", generator=g); b = torch.randn((N, K), device="cuda", generator=g) * 0.1
    c1 = torch.empty((M, N), device="cuda"); c2 = torch.empty((M, N), device="cuda")
    call = lambda c: L.check(lib.nrf_gemm_nt_f16x3(C.c_void_p(a.data_ptr()), K, C.c_int64(M), K, C.c_void_p(b.data_ptr()), K, N, C.c_void_p(c.data_ptr()), N, None, 0, None))
    torch.cuda.synchronize()
    lib.nrf_scratch_trim()
    call(c1); torch.cuda.synchronize()
    first = lib.nrf_scratch_trim()
    assert first > 0 and lib.nrf_scratch_trim() == 0
    call(c1); call(c2); call(c2); torch.cuda.synchronize()
    assert lib.nrf_scratch_trim() == first, "the same product three times over: one block, reused"
    call(c2); torch.cuda.synchronize()
    assert torch.equal(c1, c2)
    want = a.double() @ b.double().t()
    assert float((c2.double() - want).abs().max() / want.abs().max()) < 2e-6


def test_drop_in_classic_training_in_the_split_precision_products_follows_the_fp32_products():
    """oracle/_ref/adapter_check `bench train_classic`: NeRFExecutor::Train's loop body on the drop-in, 13 optimizer steps of 4 096 rays, once with the library's default layer
    products (f16x3 split precision) and once with fp32 products (NRF_TRAIN_GEMM=f32): the last losses agree to 1e-3 (measured 1e-4).  Regression test of round 6's scratch
    fix: with hipMallocAsync scratch the LibTorch host's backward -- issued from the autograd engine's thread -- computed whole layer products from B images that had been
    handed out again (losses 1 % off after one step, NaN after three) while the same calls from the Python mirror were right (scratch.hip)."""
    import json
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "oracle", "_ref", "adapter_check")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/adapter_check not built (needs /root/reference at build time)")
    last = {}
    for mode in ("auto", "f32"):
        env = dict(os.environ, NRF_TRAIN_GEMM=mode)
        out = subprocess.run([exe, "bench", "train_classic", "4", "4096"], capture_output=True, text=True, timeout=600, env=env)
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert out.returncode == 0 and lines, out.stdout[-1500:] + out.stderr[-1500:]
        txt = lines[-1]
        assert "nan" not in txt.lower().split("loss_first_last")[1], txt[-300:]
        r = json.loads(txt)
        last[mode] = r["loss_first_last"]
    assert last["auto"][0] == pytest.approx(last["f32"][0], rel=1e-6)          # the first loss comes from the same render
    assert np.isfinite(last["auto"][1]) and abs(last["auto"][1] - last["f32"][1]) <= 1e-3 * abs(last["f32"][1]), last
    assert last["f32"][1] < 0.6 * last["f32"][0], last


def test_drop_in_frame_on_the_cpp_hosts_clock_equals_the_python_mirror_bit_for_bit(api, tmp_path):
    """oracle/_ref/adapter_check `bench frame_hash`: HipNeRFRenderer::Render(800, 800, K, params, c2w) called through the reference's NeRFRenderer<>* virtual on bench.py's own
    scene (same closed-form weights, include/nrf_synth.h) -- the dumped frame equals the Python mirror's frame of the same pose BIT FOR BIT (both hosts issue the same library
    call), and the line carries the host-clock ms per frame for 1 and 2 lanes."""
    import json
    import subprocess
    from conftest import ROOT
    scene, L = api.S, api.L
    exe = os.path.join(ROOT, "oracle", "_ref", "adapter_check")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/adapter_check not built (needs /root/reference at build time)")
    out = subprocess.run([exe, "bench", "frame_hash", "2", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
    rec = json.loads(out.stdout.strip().splitlines()[-1])
    assert rec["what"] == "dropin_frame" and rec["family"] == "hash" and set(rec["ms_per_frame_by_lanes"]) == {"1", "2"} and 0 < rec["ms_per_frame"] < 500, rec
    assert abs(rec["value"] - 640000 * 256 / (rec["ms_per_frame"] * 1e-3)) < 1e-3 * rec["value"]
    got = np.fromfile(str(tmp_path / "dropin_frame_hash_rgb.f32"), np.float32).reshape(800, 800, 3)
    sc = scene.make_hash_scene(mode="cu")
    rp = scene.lego_render_params(sc["bbox"], 64, 128, 65536, L.NRF_PREC_F16_SPLIT)
    res = sc["renderer"].Render(800, 800, scene.lego_K(800, 800), rp, c2w=scene.pose_spherical(-180.0, -30.0, 4.0))
    want = res.Outputs.RGBMap.reshape(800, 800, 3).cpu().numpy()
    assert np.isfinite(got).all() and got.std() > 0.01
    assert np.array_equal(got, want), float(np.abs(got - want).max())


def test_drop_in_train_step_bench_takes_the_fused_backward_and_learns():
    """oracle/_ref/adapter_check `bench train_hash`: the statements of NeRFExecutor::Train's loop body (NeRFExecutor.h:862-995) on the drop-in, timed on the host's clock, with
    torch::optim::Adam (the reference's) and with nrfpp::HipAdam: the step runs the fused fp16 chain + the binned scatter (the phases say so), the loss falls, and both optimizers
    follow the same trajectory (same update rule)."""
    import json
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "oracle", "_ref", "adapter_check")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/adapter_check not built (needs /root/reference at build time)")
    recs = {}
    for opt in ("adam", "hipadam"):
        out = subprocess.run([exe, "bench", "train_hash", "6", "4096", opt], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
        rec = json.loads(out.stdout.strip().splitlines()[-1])
        assert rec["what"] == "dropin_train_step" and rec["optimizer"] == opt and rec["rays_per_step"] == 4096 and 0 < rec["ms_per_step"] < 500, rec
        ph = rec["synchronised_phase_ms"]
        assert "bwd.f16_chain" in ph and "bwd.hash_scatter" in ph and "bwd.f32_chain" not in ph, ph
        assert set(rec["host_ms_per_statement"]) == {"zero_grad", "render", "loss", "backward", "optimizer_step"}
        l0, l1 = rec["loss_first_last"]
        assert np.isfinite(l1) and l1 < 0.8 * l0, rec["loss_first_last"]
        recs[opt] = rec
    # identical first loss (same scene, same batch); the settling phase runs a clock-dependent number of steps, so the last losses are only both lower
    assert recs["adam"]["loss_first_last"][0] == recs["hipadam"]["loss_first_last"][0]


def test_reference_lerf_train_loop_body_runs_through_the_hip_drop_in():
    """The LeRF half of NeRFExecutor::Train's loop body (NeRFExecutor.h:955-982) on the drop-in: oracle/_ref/adapter_check `train_lerf` executes the reference's statements
    verbatim -- LeRFRenderer->Render on the ray batch, huber_loss(..., reduction none, delta 1.25).sum(-1).nanmean(), lang_loss.backward(), Optimizer->step() -- with what
    nrfpp::HipLeRFRenderer::Render forwards a ray batch to (HipLeRFPass::RenderBatch: ONE autograd node, LeRFRenderFn) in the renderer's place and torch::optim::Adam over
    the modules' own parameters.  In the same binary the gradients left on those parameters are compared with REFERENCE AUTOGRAD on the same fine depths (the compiled
    LeRFImpl::forward on the GPU, the compiled RawToOutputs' weights, the reference's inline RenderCLIPEmbedding): head 2e-3, language table 2e-2 norm-wise; the loss falls
    over three steps and the test-time render afterwards sees the stepped parameters without any call into this repo's classes."""
    import json, subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "oracle", "_ref", "adapter_check")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/adapter_check not built (needs /root/reference at build time)")
    out = subprocess.run([exe, "train_lerf"], capture_output=True, text=True, timeout=900)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert lines, out.stdout[-2000:] + out.stderr[-2000:]
    r = json.loads(lines[-1])
    assert out.returncode == 0 and r["train_lerf_ok"], (r, out.stderr[-1500:])
    assert r["gradients_vs_reference_autograd_ok"] and r["inference_after_steps_sees_updated_parameters"], r
    assert r["backward_read_the_forward_renders_features"], r          # (round 6: nrf_lerf_backward_points_src -- the gradients held to the reference's autograd above are ITS gradients)
    l = r["lang_loss_steps"]
    assert l[2] < l[1] < l[0] and r["head_gradient_worst_rel_err"] < 2e-3 and r["language_table_gradient_rel_err"] < 2e-2 and r["rendered_embedding_cos_min_vs_reference_forward"] > 1 - 2e-6, r


def test_c_abi_all_gather_at_world_sizes_above_one_with_threads_as_ranks():
    """nrf_comm_create_timeout / nrf_allgather_tiles at world sizes 2-6 on ONE GPU: the ranks are threads of tests/helpers/comm_ranks_as_threads over
    tests/helpers/mock_rccl.cpp, a stand-in for RCCL's entry points (group start / end, ncclAllGather, ncclBroadcast enqueued on the caller's stream) under RCCL's SONAME --
    the real library refuses two ranks on one device, and no box of this pool has two.  Equal tiles, unequal ones (grouped broadcasts), ranks that own no rows, several
    frames per step, two gathers back to back: every rank ends with every pixel of every frame.  (What stays unrehearsed is RCCL itself: test_two_real_rccl_ranks_...)"""
    import subprocess
    exe = os.path.join(os.path.dirname(__file__), "helpers", "_build", "comm_ranks_as_threads")
    if not os.path.exists(exe):
        subprocess.check_call(["bash", os.path.join(os.path.dirname(__file__), "helpers", "build_mock_rccl.sh")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=180)
    assert out.returncode == 0 and "all ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.count(": ok") >= 9
    # round 6: nrf_allreduce_grads (the data-parallel training step's exchange) at world 2-8 over the same stand-in: bucketed in-place mean == host-formed values bit for bit
    # (world 2: (a + b) * 0.5f, what the gloo GradSync computes), twice in a row, and the overflow agreement (one rank reports -> every rank skips, nothing exchanged)
    assert out.stdout.count("allreduce_grads world") == 8 and out.stdout.count("all skip): ok") == 2, out.stdout[-2000:]


def test_bench_step_with_the_c_abi_collective_at_world_two_threads_as_ranks():
    """bench.py's OWN step function (benchlib/steps.py FrameStepper -- what `--collective cabi`, the N > 1 default, times) at world size 2 on one GPU: two threads as ranks,
    TileComm = nrf_comm_create_timeout + nrf_allgather_tiles over tests/helpers/mock_rccl.cpp (named through NRF_RCCL_LIBRARY: torch maps the real RCCL, which refuses two
    ranks on one device), the overlapped gather completing one step later -- strong scaling (one frame, two row tiles) and weak (two frames per step): every rank's gathered
    frames == the single-rank render bit for bit."""
    import json, subprocess, sys
    from conftest import ROOT
    if not os.path.exists(os.path.join(ROOT, "tests", "helpers", "_build", "librccl.so.1")):
        subprocess.check_call(["bash", os.path.join(ROOT, "tests", "helpers", "build_mock_rccl.sh")])
    w = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "bench_step_threads_as_ranks.py")], capture_output=True, text=True, timeout=600)
    lines = [json.loads(x) for x in w.stdout.splitlines() if x.startswith("{")]
    assert w.returncode == 0 and len(lines) == 1 and lines[0]["ok"], (w.stdout[-2000:], w.stderr[-2000:])
    assert all(r["ranks_seen_by_rccl"] == 2 and r["strong"] and r["weak"] for r in lines[0]["ranks"].values())


@pytest.mark.parametrize("h", [800, 801])
def test_bench_step_at_world_eight_threads_as_ranks(h):
    """The 8-GPU run the driver makes (BASELINE config 4), rehearsed on one GPU: bench.py's step function (FrameStepper) at world 8 -- eight threads as ranks over the mock RCCL,
    each with its own replica -- for H = 800 (equal 100-row tiles: one ncclAllGather) and H = 801 (uneven tiles: the grouped broadcasts): every rank's gathered frame == the
    single-rank render bit for bit, the tiles add up to the frame, every rank saw a world of 8 and reports its host time per tile."""
    import json, subprocess, sys
    from conftest import ROOT
    if not os.path.exists(os.path.join(ROOT, "tests", "helpers", "_build", "librccl.so.1")):
        subprocess.check_call(["bash", os.path.join(ROOT, "tests", "helpers", "build_mock_rccl.sh")])
    w = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "bench_step_threads_as_ranks.py"), "8", str(h), "64"], capture_output=True, text=True, timeout=900)
    lines = [json.loads(x) for x in w.stdout.splitlines() if x.startswith("{")]
    assert w.returncode == 0 and len(lines) == 1 and lines[0]["ok"], (w.stdout[-2000:], w.stderr[-2000:])
    ranks = lines[0]["ranks"]
    assert len(ranks) == 8 and all(r["ranks_seen_by_rccl"] == 8 and r["strong"] and r["host_ms_per_tile"] > 0 for r in ranks.values())
    assert sorted(r["tile_rows"] for r in ranks.values()) == ([100] * 8 if h == 800 else [100] * 7 + [101])


def test_two_real_rccl_ranks_gather_the_single_rank_frame(tmp_path):
    """Config 4 on REAL RCCL, where the box has two GPUs (the driver's SCALE node; skipped on the one-GPU box, where two ranks can only share a device over gloo):
    (a) tests/helpers/rccl_two_rank_worker.py under torch.distributed.run -- uneven row tiles through the ncclBroadcast group of nrf_allgather_tiles and even ones through
    ncclAllGather, synchronous and overlapped, against torch.distributed's collective and against the full frame; nrf_comm_world == 2 on a communicator made by the
    bounded (blocking) rendezvous;  (b) `bench.py --gpus 2 --collective cabi --full` on nccl: the gathered 800x800 frame's sha256 == the single-rank frame's."""
    import json, os, subprocess, sys
    from conftest import ROOT
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"), NRF_BENCH_TIMEOUT="600")
    # a world of ONE through the same worker (every box): the bounded rendezvous' helper-thread ncclCommInitRank, both gather forms, real RCCL
    w1 = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "rccl_two_rank_worker.py")], capture_output=True, text=True, timeout=600,
                        env=dict(env, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29552"))
    l = [json.loads(x) for x in w1.stdout.splitlines() if x.startswith("{")]
    assert w1.returncode == 0 and len(l) == 1 and l[0]["ok"] and l[0]["ranks_seen_by_rccl"] == 1, (w1.stdout[-1500:], w1.stderr[-1500:])
    if torch.cuda.device_count() < 2:
        pytest.skip("the two-rank part needs two GPUs (RCCL refuses two ranks on one device); the world-of-one part passed")
    w = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29553",
                        os.path.join(ROOT, "tests", "helpers", "rccl_two_rank_worker.py")], capture_output=True, text=True, timeout=900, env=env)
    lines = [json.loads(x) for x in w.stdout.splitlines() if x.startswith("{")]
    assert w.returncode == 0 and len(lines) == 2 and all(l["ok"] and l["ranks_seen_by_rccl"] == 2 for l in lines), (w.stdout[-2000:], w.stderr[-2000:])
    assert any(f["rows"] == 3 for l in lines for f in l["frames"].values()) and any(f["rows"] == 2 for l in lines for f in l["frames"].values()), "uneven tiles: 3 + 2 rows of 5"
    common = ["--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-parity", "--no-also", "--no-isolated"]
    one = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + common, capture_output=True, text=True, timeout=900, env=env)
    two = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--collective", "cabi", "--full"] + common, capture_output=True, text=True, timeout=900, env=env)
    assert one.returncode == 0 and two.returncode == 0, (one.stderr[-1500:], two.stderr[-1500:])
    l1 = json.loads([x for x in one.stdout.splitlines() if x.startswith("{")][-1]); l2 = json.loads([x for x in two.stdout.splitlines() if x.startswith("{")][-1])
    assert l2["n_gpus"] == 2 and l2["ranks_seen_by_rccl"] == 2 and l2["scaling"] == "strong" and l2["tile_rows"] == 400
    assert l1["frame_sha256"] == l2["frame_sha256"] and "==" in l2["collective_check"], l2.get("collective_check")
    assert len(two.stdout.splitlines()[-1]) < 4096


# ------------------------------------------------------------------------------------------- round 6: range-safe split precision + the non-finite word
def _range_scene(api, mode="cu", table_amp=0.5, gain=1.6, scales=None, nlc=4):
    """The bench's HashNeRF scene (nerfpp_amd/scene.py::make_hash_scene) with per-layer weight multipliers: {layer name: factor} on top of sigma_net_2 x 30."""
    S, M = api.S, api.M
    table = S.synth_hash_table(16, 19, 2, 5000, table_amp)
    if mode == "cu":
        emb = M.CuHashEmbedder("embedder", S.LEGO_BBOX, 16, 2, 19, 16, 512); emb.set_primes(np.array(S.CU_PRIMES[:48], np.int32)); dirs = M.CuSHEncoder("embeddirs", 3, 4)
    else:
        emb = M.HashEmbedder("embedder", S.LEGO_BBOX, 16, 2, 19, 16, 512); dirs = M.SHEncoder("embeddirs", 3, 4)
    emb.set_table(table)
    sc = {"sigma_net_2": 30.0}
    for k, v in (scales or {}).items():
        sc[k] = sc.get(k, 1.0) * v
    params = S.synth_linear_stack(S.small_shapes(32, 16, 3, 64, 15, nlc, 64), 6000, gain, 0.0, sc)
    blob = np.concatenate([a.reshape(-1) for _, a in params])
    mlp = M.NeRFSmall(3, 64, 15, nlc, 64, False, 3, 64, 32, 16, "model", params=blob)
    return dict(renderer=api.R.NeRFRenderer(emb, dirs, mlp), mlp=mlp, embedder=emb, bbox=S.LEGO_BBOX, blob=blob)


def _split_vs_f32_rows(api, sc, rows=96, policy=None):
    import copy
    S, L = api.S, api.L
    H = W = 800
    K = S.lego_K(H, W); c2w = S.pose_spherical(-180.0, -30.0, 4.0)
    rp = S.lego_render_params(sc["bbox"], 64, 128, 65536, L.NRF_PREC_F16_SPLIT)
    if policy is not None:
        rp.OverflowPolicy = policy
    r0 = (H - rows) // 2
    a = sc["renderer"].Render(H, W, K, rp, c2w=c2w, row0=r0, rows=rows).Outputs.RGBMap
    rp32 = copy.copy(rp); rp32.Precision = L.NRF_PREC_F32; rp32.Chunk = 32768
    b = sc["renderer"].Render(H, W, K, rp32, c2w=c2w, row0=r0, rows=rows).Outputs.RGBMap
    return a, b


_P2 = lambda e: 2.0 ** e
RANGE_CASES = {
    # the SAME function as the bench scene (the per-net products of the factors are 1): a checkpoint whose layers sit at very different magnitudes
    "layers x 2^-8 / 2^+8 alternating": dict(scales={"sigma_net_0": _P2(-8), "sigma_net_1": _P2(8), "color_net_0": _P2(-8), "color_net_1": _P2(8), "color_net_2": _P2(-8), "color_net_3": _P2(8)}),
    "hidden layers x 2^+6, heads x 2^-12 / 2^-18": dict(scales={"sigma_net_0": _P2(6), "sigma_net_1": _P2(6), "sigma_net_2": _P2(-12), "color_net_0": _P2(0), "color_net_1": _P2(6), "color_net_2": _P2(6),
                                                                "color_net_3": _P2(-12)}),
    "hidden activations beyond 65 504: first layers x 2^12, heads x 2^-24": dict(scales={"sigma_net_0": _P2(12), "sigma_net_1": _P2(12), "sigma_net_2": _P2(-24), "color_net_1": _P2(12), "color_net_2": _P2(12),
                                                                                         "color_net_3": _P2(-24)}),
    "hidden layers x 2^-10, heads x 2^+20 / 2^+30": dict(scales={"sigma_net_0": _P2(-10), "sigma_net_1": _P2(-10), "sigma_net_2": _P2(20), "color_net_0": _P2(-30), "color_net_1": _P2(-10), "color_net_2": _P2(-10),
                                                                 "color_net_3": _P2(30)}),
    # other functions: small-gain checkpoints, the reference's own table initialisation scale, every weight scaled down
    "xavier gain 0.1 (|W| ~ 0.01, Trainable.h:33-53)": dict(gain=0.1, scales={"sigma_net_2": 3000.0, "color_net_3": 300.0}),
    "table U 1e-4 (CuHashEmbedder.cpp:24)": dict(table_amp=1e-4, scales={"sigma_net_0": 3000.0}),
    "all weights x 2^-8": dict(scales={**{f"sigma_net_{i}": _P2(-8) for i in range(3)}, **{f"color_net_{i}": _P2(-8) for i in range(4)}}),
    "ngp twin, xavier gain 0.1": dict(mode="ngp", gain=0.1, scales={"sigma_net_2": 3000.0, "color_net_3": 300.0}),
    "ngp twin, layers x 2^-8 / 2^+8 alternating": dict(mode="ngp", scales={"sigma_net_0": _P2(-8), "sigma_net_1": _P2(8), "color_net_0": _P2(-8), "color_net_1": _P2(8), "color_net_2": _P2(-8), "color_net_3": _P2(8)}),
}


@pytest.mark.parametrize("case", list(RANGE_CASES))
def test_split_precision_is_range_safe(api, case):
    """NRF_PREC_F16_SPLIT on checkpoints of unusual magnitude: the split-precision operand image is range-scaled per layer (ReLU is positively
    homogeneous: powers of two, exact in fp32; mlp.hip k_small_scales), so weights of 0.01 or 2^12 render like weights near 1 -- every pixel of 96 rows of the 800x800
    frame within 4e-6 of the library's own NRF_PREC_F32 mode (== the CPU oracle bit for bit), nothing flagged, nothing rendered again.  With the scaling switched off
    (the representation of rounds 4-5) the same checkpoints lose digits or overflow: asserted for the cases where that is what the numbers say."""
    L = api.L
    sc = _range_scene(api, **RANGE_CASES[case])
    a, b = _split_vs_f32_rows(api, sc)
    assert bool(torch.isfinite(a).all())
    err = float((a - b).abs().max())
    assert err <= 4e-6, (case, err)
    assert sc["renderer"].nonfinite() == (0, 0)
    gs = (C.c_float * 12)(); ks = (C.c_float * 8)()
    L.check(L.lib().nrf_mlp_get_split_scales(sc["mlp"]._m, gs, ks, None))
    assert all(v > 0 and np.log2(v) == int(np.log2(v)) for v in list(gs) + list(ks)), "scales are powers of two"
    assert any(v != 1.0 for v in gs), "this checkpoint needs scaling"
    if "alternating" in case or "65 504" in case or "2^-10" in case:
        L.check(L.lib().nrf_mlp_set_split_scaling(sc["mlp"]._m, 0, None))
        a0, _ = _split_vs_f32_rows(api, sc, policy=L.NRF_OVERFLOW_IGNORE)
        bad = (not bool(torch.isfinite(a0).all())) or float((a0 - b).abs().max()) > 1e-4
        assert bad, "the unscaled split image is expected to lose this checkpoint"


def test_range_scaling_leaves_ordinary_checkpoints_alone(api):
    """Dead band: the bench scene (and its LibTorch twin) keep every exponent at 0 -- their frames are bit for bit the frames of round 5 (frame_sha256 of bench.py unchanged);
    and the scales are a deterministic function of (blob, table): two handles of the same model agree, a table upload moves the first layer's exponent and only that."""
    L = api.L
    for mode in ("cu", "ngp"):
        sc = _range_scene(api, mode=mode)
        a, b = _split_vs_f32_rows(api, sc, rows=32)          # the first render binds the network to the grid's table RMS
        gs = (C.c_float * 12)(); ks = (C.c_float * 8)()
        L.check(L.lib().nrf_mlp_get_split_scales(sc["mlp"]._m, gs, ks, None))
        assert list(gs) == [1.0] * 12 and list(ks)[:3] == [1.0] * 3, (mode, list(gs), list(ks))
        assert float((a - b).abs().max()) <= 4e-6
    # a table 2^12 times smaller: the first layer takes the difference, the rest of the network stays where it was
    sc = _range_scene(api)
    _split_vs_f32_rows(api, sc, rows=8)
    sc["embedder"].set_table(api.S.synth_hash_table(16, 19, 2, 5000, 0.5 * 2.0 ** -12))
    a, b = _split_vs_f32_rows(api, sc, rows=32)
    gs = (C.c_float * 12)(); ks = (C.c_float * 8)()
    L.check(L.lib().nrf_mlp_get_split_scales(sc["mlp"]._m, gs, ks, None))
    assert gs[0] >= 2.0 ** 10 and list(gs)[1:3] == [1.0, 1.0], list(gs)
    assert float((a - b).abs().max()) <= 4e-6


def test_nonfinite_word_and_the_overflow_policies(api):
    """nrf_render_params.overflow_policy on a checkpoint whose activations leave the fp16 range (range scaling switched off to provoke it: first layers x 2^12):
    RERENDER (the default) returns the NRF_PREC_F32 frame bit for bit and counts the chunks it rendered again; ERROR raises NRF_ERR_NONFINITE; DEFERRED returns at once and the
    NEXT call raises; IGNORE hands the garbage back silently (what every matrix-core render did before this round)."""
    L = api.L
    kw = RANGE_CASES["hidden activations beyond 65 504: first layers x 2^12, heads x 2^-24"]
    sc = _range_scene(api, **kw)
    L.check(L.lib().nrf_mlp_set_split_scaling(sc["mlp"]._m, 0, None))
    a, b = _split_vs_f32_rows(api, sc, rows=40)                              # 32 000 rays: one chunk of 65 536
    assert torch.equal(a, b), "flagged chunks are rendered again in NRF_PREC_F32: the parity mode's pixels"
    flagged, again = sc["renderer"].nonfinite()
    assert flagged >= 1 and again == flagged
    with pytest.raises(L.NrfError, match="non-finite"):
        _split_vs_f32_rows(api, sc, rows=40, policy=L.NRF_OVERFLOW_ERROR)
    x, _ = _split_vs_f32_rows(api, sc, rows=40, policy=L.NRF_OVERFLOW_IGNORE)
    assert not torch.equal(x, b)
    before = sc["renderer"].nonfinite()[0]
    S = api.S
    rp = S.lego_render_params(sc["bbox"], 64, 128, 65536, L.NRF_PREC_F16_SPLIT); rp.OverflowPolicy = L.NRF_OVERFLOW_DEFERRED
    sc["renderer"].Render(800, 800, S.lego_K(800, 800), rp, c2w=S.pose_spherical(-180.0, -30.0, 4.0), row0=380, rows=40)      # returns without waiting
    torch.cuda.synchronize()
    with pytest.raises(L.NrfError, match="EARLIER"):
        sc["renderer"].Render(800, 800, S.lego_K(800, 800), rp, c2w=S.pose_spherical(-180.0, -30.0, 4.0), row0=380, rows=8)
    assert sc["renderer"].nonfinite()[0] > before
    # with the scaling back on the same checkpoint is fine under every policy
    L.check(L.lib().nrf_mlp_set_split_scaling(sc["mlp"]._m, 1, None))
    a, b = _split_vs_f32_rows(api, sc, rows=40, policy=L.NRF_OVERFLOW_ERROR)
    assert float((a - b).abs().max()) <= 4e-6


@pytest.mark.parametrize("mlp_backward", ["f32", "f16"])
def test_data_parallel_training_over_the_c_abi_all_reduce_threads_as_ranks(mlp_backward):
    """Trainer(grad_sync=CabiGradSync(TileComm)) -- nrf_allreduce_grads behind the C ABI, the exchange a C++ host makes through nrfpp::TileComm::AllReduceGrads -- at world 2
    on one GPU (threads as ranks over tests/helpers/mock_rccl.cpp): after four steps on disjoint halves of the ray batches the replicas hold the same parameters BIT FOR BIT,
    and the first step's averaged gradient equals the gradient of one process that took the whole batch (1e-4 norm-wise in fp32; 3e-2 with the fp16 chain, whose loss scale
    is per rank)."""
    import json, subprocess, sys
    from conftest import ROOT
    if not os.path.exists(os.path.join(ROOT, "tests", "helpers", "_build", "librccl.so.1")):
        subprocess.check_call(["bash", os.path.join(ROOT, "tests", "helpers", "build_mock_rccl.sh")])
    w = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "train_dp_threads_as_ranks.py"), mlp_backward], capture_output=True, text=True, timeout=600)
    lines = [json.loads(x) for x in w.stdout.splitlines() if x.startswith("{")]
    assert w.returncode == 0 and len(lines) == 1 and lines[0]["ok"], (lines, w.stderr[-1500:])
    assert lines[0]["replicas_bit_identical"] and lines[0]["ranks_seen_by_rccl"] == 2


@pytest.mark.parametrize("optimizer", ["adam", "hipadam"])
def test_drop_in_data_parallel_training_two_thread_ranks_end_with_identical_replicas(optimizer):
    """oracle/_ref/adapter_check `train_dp`: NeRFExecutor::Train's loop body on the drop-in with ONE added statement -- nrfpp::TileComm::AllReduceGrads(grad_vars) between
    loss.backward() and Optimizer->step() (nrf_allreduce_grads behind the C ABI) -- at world 2, the ranks being two threads over tests/helpers/mock_rccl.cpp (NRF_RCCL_LIBRARY).
    Three steps on disjoint halves of the batches: the replicas' parameters are bit-identical, and differ from a replica trained without the exchange."""
    import json, subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "oracle", "_ref", "adapter_check")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/adapter_check not built (needs /root/reference at build time)")
    mock = os.path.join(ROOT, "tests", "helpers", "_build", "librccl.so.1")
    if not os.path.exists(mock):
        subprocess.check_call(["bash", os.path.join(ROOT, "tests", "helpers", "build_mock_rccl.sh")])
    out = subprocess.run([exe, "train_dp", optimizer], capture_output=True, text=True, timeout=600, env=dict(os.environ, NRF_RCCL_LIBRARY=mock))
    lines = [json.loads(x) for x in out.stdout.splitlines() if x.startswith("{")]
    assert out.returncode == 0 and len(lines) == 1 and lines[0]["train_dp_ok"], (lines, out.stdout[-1500:], out.stderr[-1500:])
    assert lines[0]["replicas_bit_identical"] and lines[0]["differs_from_a_replica_without_the_exchange"]


def test_bench_two_rank_rehearsal_carries_the_data_parallel_training_step():
    """`python bench.py --gpus 2 --backend gloo --full` WITH its `also` part (two ranks sharing this box's GPU): besides the other scaling mode every rank runs the data-parallel
    training step (benchlib/extras.py::dp_train_step_measurement: a Trainer per rank on its own ray batch, gradients averaged before Adam -- torch.distributed here, the C-ABI
    nrf_allreduce_grads with --backend nccl) and the line's `also` names it; the replicas' parameter checksums agree exactly after the steps."""
    import json, os, subprocess, sys
    from conftest import ROOT
    env = dict(os.environ, NRF_BENCH_TIMEOUT="900")
    two = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline",
                          "--no-parity", "--no-isolated"], capture_output=True, text=True, timeout=1200, env=env)
    assert two.returncode == 0, two.stderr[-2500:]
    line = json.loads([x for x in two.stdout.splitlines() if x.startswith("{")][-1])
    names = [a.get("workload") for a in line.get("also", [])]
    assert "hashnerf_train_step_dp" in names and any(n.startswith("scaling_") for n in names), line.get("also")
    side = json.load(open(os.path.join(ROOT, "bench_detail.json")))
    dp = [a for a in side["also"] if a.get("workload") == "hashnerf_train_step_dp"][0]
    assert "error" not in dp and dp["n_gpus"] == 2 and dp["rays_per_step"] == 32768 and dp["replicas_checksum_spread"] == 0.0 and dp["ms_per_step"] > 0, dp


def test_hip_lerf_renderer_subclass_linked_and_run():
    """oracle/_ref/adapter_lerf_check: nrfpp::HipLeRFRenderer : LeRFRenderer linked against the reference's own LeRFRenderer.cpp (its RuCLIP include filtered out; `Relevancy`
    supplied by this repository's restatement -- pins nothing) and driven through the reference's virtuals: the deterministic pose and ray-batch renders equal HipLeRFPass bit
    for bit with LeRFRenderer.cpp:311-328's shapes; the RNG branches (Perturb > 0, ThinRay = false) run the INHERITED BatchifyRays / RenderRays (torch ops, torch's generator,
    LeRFRenderer.cpp:85-263) to finite results through the overridden RunLENetwork / RawToLEOutputs; RawNoiseStd > 0 is finite or refused loudly; the training render's
    backward reaches the module's parameters and the language grid."""
    import json, subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "oracle", "_ref", "adapter_lerf_check")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/adapter_lerf_check not built (needs /root/reference at build time)")
    out = subprocess.run([exe, "12", "12"], capture_output=True, text=True, timeout=600)
    lines = [json.loads(x) for x in out.stdout.splitlines() if x.startswith("{")]
    assert out.returncode == 0 and len(lines) == 1 and lines[0]["lerf_renderer_ok"], (lines, out.stdout[-1500:], out.stderr[-1500:])
    r = lines[0]
    assert r["pose_render_equals_pass_bit_for_bit"] and r["ray_batch_render_equals_pass"] and r["perturb_branch_inherited_finite_on_overrides"] and \
        r["cone_ray_branch_inherited_finite_on_overrides"] and r["training_render_backward_reaches_parameters"] and min(r["override_calls"]) > 0


# ------------------------------------------------------------------------------------------- round 6: fifty training steps against the reference's own loss curve
def _train_curve_run(api, manifest, mlp_backward, precision, steps=None):
    """The student of golden `train_curve` (HashEmbedder L16 F2 T2^12 + SHEncoder(4) + NeRFSmall 3x64 / 3x64, closed-form initial weights from the manifest) trained by
    nerfpp_amd.train.Trainer on the golden's batches: step i = 192 pixels of teacher view i % 4, pixel (131 i + 29 j) % 576 -- regenerated here from GetRays."""
    from nerfpp_amd.train import Trainer
    g = load_golden("train_curve")
    h, w, ns, ni, nsteps, nrays, nviews = (int(v) for v in g["dims"])
    steps = nsteps if steps is None else steps
    ent = manifest["train_curve"]
    table = synth.blob_from_manifest([x for x in ent if "embeddings" in x[0]])
    blob = synth.blob_from_manifest([x for x in ent if "embeddings" not in x[0]])
    e = api.M.HashEmbedder("embedder", g["bbox"], 16, 2, 12, 16, 128)
    e.set_table(table)
    ed = api.M.SHEncoder("embeddirs", 3, 4)
    m = api.M.NeRFSmall(3, 64, 15, 3, 64, False, 3, 64, 32, 16, "model", params=blob)
    K = api.S.lego_K(h, w)
    rays = []
    for th in g["thetas"]:
        o, d, _ = api.R.GetRays(h, w, K, api.S.pose_spherical(float(th), -30.0, 4.0))
        rays.append((o.reshape(-1, 3), d.reshape(-1, 3)))
    imgs = dev(g["teacher_images"])
    rp = api.R.NeRFRenderParams(NSamples=ns, NImportance=ni, Chunk=4096, Perturb=0.0, WhiteBkgr=False, Ndc=False, UseViewdirs=True, ThinRay=True, BoundingBox=g["bbox"],
                                Precision=precision)
    lr0 = float(g["lr0_lrate_decay"][0])
    losses, mses = [], []
    with Trainer(e, ed, m, table, blob, learning_rate=lr0, mlp_backward=mlp_backward, hash_backward="binned" if mlp_backward == "f16" else "f32") as tr:
        for i in range(steps):
            v = i % nviews
            idx = torch.as_tensor((131 * i + 29 * np.arange(nrays)) % (h * w), device="cuda")
            o, d, tgt = rays[v][0][idx].contiguous(), rays[v][1][idx].contiguous(), imgs[v][idx].contiguous()
            if i == 0:
                assert_exact(host(o), g["s0_rays_o"], "first batch: origins"); assert_exact(host(d), g["s0_rays_d"], "first batch: directions")
                assert_exact(host(tgt), g["s0_target"], "first batch: targets")
            # the learning rate stays lr0: the reference's decay loop writes to a COPY of each param group (NeRFExecutor.h:995-996; golden lr_in_force_and_lr_computed[:, 0])
            lm, _ = tr.step(o, d, tgt, rp)
            lm = host(lm)
            losses.append(float(lm[0])); mses.append(float(lm[1]))
        skipped = int(getattr(tr, "skipped_steps", 0))
    return g, np.array(losses), np.array(mses), skipped


def test_training_loss_curve_follows_the_reference_for_fifty_steps(api, manifest):
    """fifty consecutive optimisation steps -- render, huber, backward, Adam -- of the HIP Trainer against the SAME fifty steps run by the reference's own
    modules, autograd and torch::optim::Adam on the CPU (golden `train_curve`, oracle/_ref/ref_driver; identical initial weights and batches).  fp32 chain, NRF_PREC_F32.
    The loop is chaotic at the rounding level -- Adam with eps 1e-15 turns a rounding-level gradient into a whole lr step, a fine sample that changes CDF bin moves a pixel --
    and the golden says by how much for the reference ITSELF: run with 1 instead of 8 intra-op threads its own curve moves by up to 9e-4 (after twelve steps equal to an ulp).
    Measured here (profiles/round6/r6j_loss_curve_probe.log): within 4e-4 of the reference for the first 19 steps, within 1.1e-2 through step 50 (median 1.8e-3), same
    final level.  Bars: 5e-4 over the first 15 steps, 2e-2 overall, median 3e-3."""
    g, loss, mse, skipped = _train_curve_run(api, manifest, "f32", api.L.NRF_PREC_F32)
    ref = g["loss"]
    assert (g["lr_in_force_and_lr_computed"][:, 0] == g["lr0_lrate_decay"][0]).all(), "the reference's learning rate never changes (its decay loop updates a copy)"
    self_rel = np.abs(g["loss_one_thread"] - ref) / ref
    assert self_rel[:12].max() < 2e-7 and 1e-4 < self_rel.max() < 5e-3, "the reference against itself at another thread count: the same to one ulp at first, then apart"
    rel = np.abs(loss - ref) / ref
    assert np.isfinite(loss).all() and skipped == 0
    assert rel[0] < 1e-6 and rel[:15].max() < 5e-4, rel[:15]               # the first steps: same function, same gradients
    assert rel.max() < 2e-2 and np.median(rel) < 3e-3, (rel.max(), np.median(rel), rel.argmax())
    assert ref[-5:].mean() < 0.06 * ref[0] and abs(loss[-5:].mean() - ref[-5:].mean()) < 1e-2 * ref[-5:].mean()


def test_training_loss_curve_with_the_fast_chain(api, manifest):
    """The same fifty steps on what bench.py times: NRF_PREC_F16_SPLIT render, fused fp16 matrix-core backward, binned hash scatter.  Measured: within 2e-3 of the reference's
    curve for the first 19 steps, within 4.1e-2 through step 50 (median 3.5e-3), the same final level to 2 %."""
    g, loss, mse, skipped = _train_curve_run(api, manifest, "f16", api.L.NRF_PREC_F16_SPLIT)
    ref = g["loss"]
    rel = np.abs(loss - ref) / ref
    assert np.isfinite(loss).all() and skipped == 0
    assert rel[:15].max() < 3e-3, rel[:15]
    assert rel.max() < 8e-2 and np.median(rel) < 8e-3, (rel.max(), np.median(rel))
    assert abs(loss[-5:].mean() - ref[-5:].mean()) < 3e-2 * ref[-5:].mean()


def test_end_to_end_training_run_measurement(api):
    """bench.py's `hashnerf_train_run` entry (benchlib/extras.py::train_run_measurement) at a reduced size: producer + render + backward + Adam per iteration on teacher-rendered
    views, main.cpp's batch shape; the loss falls, no step is skipped, and the held-out view's PSNR against the teacher improves by more than 8 dB in 120 iterations."""
    from benchlib import extras
    rec = extras.train_run_measurement(api.S, api.L, iters=120, n_rand=8192, views=4, hw=200)
    assert rec["workload"] == "hashnerf_train_run" and rec["skipped_steps"] == 0 and rec["ms_per_step"] > 0
    l0, lm, l1 = rec["loss_first_mid_last"]
    p0, p1 = rec["psnr_held_out_view_before_after_db"]
    assert l1 < 0.5 * l0 and p1 > p0 + 8.0, rec


# ------------------------------------------------------------------------------------------- round 6: bf16x3 split-precision training products
@pytest.mark.parametrize("M,N,K", [(70000, 256, 256), (33000, 256, 160), (5000, 128, 283), (4097, 33, 256), (777, 70, 63), (300, 3, 128),
                                   (5461, 768, 256), (70001, 33, 256), (66000, 128, 128), (40000, 256, 768)])
def test_gemm_nt_bf16x3_vs_float64(api, M, N, K):
    """nrf_gemm_nt_bf16x3 / nrf_gemm_nt_f16x3 (gemm_bf16x3.hip: every fp32 operand as hi + lo bf16, or as hi + lo fp16 of power-of-two scaled rows; three matrix-core
    products per fp32 accumulator) against the float64 product: within 2e-5 (bf16; measured 5e-6) / 2e-6 (fp16; measured 5e-7, torch's fp32 product 8e-7) of the largest
    entry, bias + ReLU epilogue included; ragged M / N / K (row, column and K-tile tails), the whole-row (persistent) kernel's shapes (K in {128, 160, 256}; N > 128, three
    column blocks at N = 768, and the narrow products N = 33 / 128 that take its 256-wide tile once M >= 65 536) and the generic one's (K = 768: 24 K tiles)."""
    L = api.L
    g = torch.Generator(device="cuda"); g.manual_seed(M + N + K)
    a = torch.randn((M, K), device="cuda", generator=g); b = torch.randn((N, K), device="cuda", generator=g) * 0.1; bias = torch.randn((N,), device="cuda", generator=g)
    want = torch.relu(a.double() @ b.double().t() + bias.double())
    for fn, bar in ((L.lib().nrf_gemm_nt_bf16x3, 2e-5), (L.lib().nrf_gemm_nt_f16x3, 2e-6)):
        c = torch.full((M, N), float("nan"), device="cuda")
        L.check(fn(C.c_void_p(a.data_ptr()), K, C.c_int64(M), K, C.c_void_p(b.data_ptr()), K, N, C.c_void_p(c.data_ptr()), N, C.c_void_p(bias.data_ptr()), 1, None))
        assert bool(torch.isfinite(c).all())
        err = float((c.double() - want).abs().max() / want.abs().max())
        assert err < bar, (err, bar)


def test_gemm_nt_f16x3_rows_of_any_magnitude(api):
    """The scaled fp16 arithmetic where an unscaled fp16 pair fails (round 5's fp16x3 training GEMMs were removed for it): rows of A between 1e-12 and 1e+8 -- what a
    back-propagated gradient looks like --, zero rows, a row of small entries with one huge one, weights x 1e-6 and x 1e+4, through the whole-row kernel (K = 256) and the
    generic one (K = 200, two segments).  Error PER ROW relative to the row's largest result: below 4e-6 everywhere (measured 9e-7; torch's fp32 product 1.7e-6); the bf16
    arithmetic (range-safe by construction) is held to 1e-4 on the same rows."""
    L = api.L
    g = torch.Generator(device="cuda"); g.manual_seed(7)
    M, N = 20000, 200
    for K in (256, 200):
        a = torch.randn((M, K), device="cuda", generator=g) * torch.pow(10.0, torch.rand((M, 1), device="cuda", generator=g) * 20 - 12)
        a[::97] = 0.0
        a[5::101, 3] *= 1e6
        for wscale in (1.0, 1e-6, 1e4):
            b = torch.randn((N, K), device="cuda", generator=g) * 0.1 * wscale
            want = a.double() @ b.double().t()
            rowmax = want.abs().amax(dim=1).clamp_min(1e-300)
            for fn, bar in ((L.lib().nrf_gemm_nt_f16x3, 4e-6), (L.lib().nrf_gemm_nt_bf16x3, 1e-4)):
                c = torch.full((M, N), float("nan"), device="cuda")
                L.check(fn(C.c_void_p(a.data_ptr()), K, C.c_int64(M), K, C.c_void_p(b.data_ptr()), K, N, C.c_void_p(c.data_ptr()), N, None, 0, None))
                assert bool(torch.isfinite(c).all())
                assert bool((c[::97] == 0).all()), "zero rows stay zero"
                err = float(((c.double() - want).abs().amax(dim=1) / rowmax).max())
                assert err < bar, (K, wscale, err, bar)


@pytest.mark.gpu
@pytest.mark.parametrize("P,out,n,ldg,ldx", [(60000, 256, 256, 256, 264), (50001, 1, 256, 4, 256), (50001, 3, 128, 4, 128), (20000, 7, 63, 8, 63), (8200, 33, 96, 40, 96)])
def test_layer_grad_split_weight_and_bias_gradients_vs_float64(api, P, out, n, ldg, ldx):
    """nrf_layer_grad_split: a layer's weight AND bias gradient as the classic / LeRF backward compute them -- 32 rows and more: the bf16x3 TN product with the bias sums
    taken out of the same pass over G; a head of fewer rows (alpha: 1, rgb: 3): fp32 FMAs four rows per pass over X.  Against float64: dW within 2e-5 of its largest entry
    (thin heads: 2e-6, they are fp32 sums), db within 2e-6 of sum |g|; both ADDED to what the buffers held; dW deterministic."""
    L = api.L
    gen = torch.Generator(device="cuda"); gen.manual_seed(P + out + n)
    G = torch.randn((P, ldg), device="cuda", generator=gen) * torch.pow(10.0, torch.rand((P, 1), device="cuda", generator=gen) * 4 - 4)
    X = torch.randn((P, ldx), device="cuda", generator=gen)
    dw0 = torch.randn((out, n), device="cuda", generator=gen); db0 = torch.randn((out,), device="cuda", generator=gen)
    want_w = dw0.double() + G[:, :out].double().t() @ X[:, :n].double()
    want_b = db0.double() + G[:, :out].double().sum(0)
    res = []
    for _ in range(2):
        dw, db = dw0.clone(), db0.clone()
        L.check(L.lib().nrf_layer_grad_split(C.c_void_p(G.data_ptr()), ldg, out, C.c_void_p(X.data_ptr()), ldx, n, C.c_int64(P), C.c_void_p(dw.data_ptr()), n, 0, C.c_void_p(db.data_ptr()), None))
        res.append((dw, db))
    assert torch.equal(res[0][0], res[1][0]), "deterministic"
    if out >= 32:
        assert torch.equal(res[0][1], res[1][1]), "the bias sums out of the TN pass are deterministic too (a thin head's go through k_grad_b's float atomics)"
    dw, db = res[0]
    scale_w = (G[:, :out].double().t() @ X[:, :n].double()).abs().max()
    ew = float((dw.double() - want_w).abs().max() / scale_w)
    eb = float(((db.double() - want_b).abs() / G[:, :out].double().abs().sum(0).clamp_min(1e-30)).max())
    assert ew < (2e-5 if out >= 32 else 2e-6), ew
    assert eb < 2e-6, eb


@pytest.mark.gpu
def test_training_backward_reads_the_features_its_forward_render_encoded(api):
    """The hash training step's backward needs the hash features of the fine depths; its forward render (a single-chunk render of the feature-reusing fast path) has just
    encoded exactly those points -- coarse columns, the new samples' columns, the merge map.  nrf_renderer_last_features hands that view over and
    nrf_mlp_backward_f16_lm_src / nrf_mask_sigma_grad_src read through the map: the same loss and the same gradients (to the last bits of the fused backward's atomic sums) as with a second encode of the points
    (nrf_hash_encode_lm_f16); a render in between invalidates the view (the backward then encodes again); a multi-chunk render leaves none."""
    L, S, R = api.L, api.S, api.R
    from nerfpp_amd.train import Trainer
    K = S.lego_K(100, 100); c2w = S.pose_spherical(30.0, -30.0, 4.0)
    o, d, _ = R.GetRays(100, 100, K, c2w)
    o = o.reshape(-1, 3)[::3][:3000].contiguous(); d = d.reshape(-1, 3)[::3][:3000].contiguous()
    tgt = torch.rand((o.shape[0], 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))
    rp = R.NeRFRenderParams(NSamples=64, NImportance=128, Chunk=4096, Perturb=0.0, WhiteBkgr=False, Ndc=False, UseViewdirs=True, ThinRay=True, BoundingBox=S.LEGO_BBOX,
                            Precision=L.NRF_PREC_F16_SPLIT, ReturnRaw=True, KeepIntermediates="depths")          # (what Trainer.step asks for)
    grads = {}
    # (the fused backward adds its workgroups' weight-gradient tiles with float atomics: two calls on the same inputs agree to the last bits of the sum, not bit for bit)
    same = lambda a, b: float((a - b).abs().max()) <= 2e-6 * float(b.abs().max())
    for reuse in (True, False):
        sc = S.make_hash_scene(mode="cu", log2_t=14, table_amp=1e-2, sigma_scale=4.0)
        tr = Trainer(sc["embedder"], sc["embeddirs"], sc["mlp"], sc["table"], sc["mlp_blob"], learning_rate=5e-4, mlp_backward="f16", hash_backward="binned")
        tr.reuse_render_features = reuse
        res = tr.renderer.Render(0, 0, None, rp, rays=(o, d, None))
        assert res.FeatureView is not None and res.FeatureView["n"] == o.shape[0] and res.FeatureView["sf"] == 192
        lm = tr.backward(res, tgt, 192, False, params=rp)
        assert tr.reused_render_features is reuse
        grads[reuse] = (tr.g_blob.clone(), tr.g_table.clone(), host(lm).copy())
        if reuse:
            # a render in between: the view in `res` is stale, the backward falls back to encoding the points (same gradients again)
            tr.renderer.Render(0, 0, None, rp, rays=(o[:100], d[:100], None))
            tr.backward(res, tgt, 192, False, params=rp)
            assert tr.reused_render_features is False and same(tr.g_blob, grads[True][0]) and same(tr.g_table, grads[True][1])
            # two chunks: no view
            rp2 = R.NeRFRenderParams(**{**rp.__dict__, "Chunk": 2048})
            assert tr.renderer.Render(0, 0, None, rp2, rays=(o, d, None)).FeatureView is None
    assert np.array_equal(grads[True][2], grads[False][2])
    assert same(grads[True][0], grads[False][0]) and same(grads[True][1], grads[False][1])
    assert float(grads[True][0].abs().max()) > 0 and float(grads[True][1].abs().max()) > 0


@pytest.mark.gpu
def test_training_step_with_an_overflowed_fp16_backward_is_skipped_on_the_device(api):
    """Trainer.step with the fused fp16 backward no longer waits for the chain's overflow words in the middle of the step: the optimizer step is nrf_adam_step_guarded --
    the kernel itself returns when either word is set -- and the host reads the words (copied to pinned memory behind the backward) before the NEXT step begins.  A batch
    whose target holds a NaN (the incoming gradient is flagged): parameters and Adam moments keep their bits, the step count is taken back, skipped_steps counts it, and
    the step after it is an ordinary one with the bias correction of step 2."""
    L, S, R = api.L, api.S, api.R
    from nerfpp_amd.train import Trainer
    sc = S.make_hash_scene(mode="cu", log2_t=14, table_amp=1e-2, sigma_scale=4.0)
    K = S.lego_K(100, 100); c2w = S.pose_spherical(30.0, -30.0, 4.0)
    o, d, _ = R.GetRays(100, 100, K, c2w)
    o = o.reshape(-1, 3)[::5][:1024].contiguous(); d = d.reshape(-1, 3)[::5][:1024].contiguous()
    tgt = torch.rand((o.shape[0], 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    tr = Trainer(sc["embedder"], sc["embeddirs"], sc["mlp"], sc["table"], sc["mlp_blob"], learning_rate=5e-4, mlp_backward="f16", hash_backward="binned")
    rp = R.NeRFRenderParams(NSamples=32, NImportance=32, Chunk=1024, Perturb=0.0, WhiteBkgr=False, Ndc=False, UseViewdirs=True, ThinRay=True, BoundingBox=S.LEGO_BBOX,
                            Precision=L.NRF_PREC_F16_SPLIT)
    tr.step(o, d, tgt, rp)
    assert tr.skipped_steps == 0 and tr.t == 1
    snap = [x.clone() for x in (tr.table, tr.blob, tr.m_table, tr.v_table, tr.m_blob, tr.v_blob)]
    bad = tgt.clone(); bad[0, 0] = float("nan")          # (an inf would be clamped by the huber gradient: a NaN passes through)
    tr.step(o, d, bad, rp)
    assert tr.skipped_steps == 1 and tr.t == 1 and tr.overflow
    for a, b in zip(snap, (tr.table, tr.blob, tr.m_table, tr.v_table, tr.m_blob, tr.v_blob)):
        assert torch.equal(a, b), "a skipped step leaves parameters and moments untouched"
    tr.step(o, d, tgt, rp)
    assert tr.skipped_steps == 1 and tr.t == 2 and not torch.equal(snap[1], tr.blob) and bool(torch.isfinite(tr.blob).all()) and bool(torch.isfinite(tr.table).all())
    # the same three batches with the host waiting for the words inside each step (a gradient hook switches the deferral off): the same bookkeeping, and parameters that
    # moved by the same two Adam steps (|update| <= lr per step whatever the gradient's size -- eps is 1e-15 -- and the fp32 atomics of the backward make two runs differ
    # in the last bits of the smallest gradients: no bit equality between ANY two runs)
    sc2 = S.make_hash_scene(mode="cu", log2_t=14, table_amp=1e-2, sigma_scale=4.0)
    tr2 = Trainer(sc2["embedder"], sc2["embeddirs"], sc2["mlp"], sc2["table"], sc2["mlp_blob"], learning_rate=5e-4, mlp_backward="f16", hash_backward="binned",
                  grad_sync=lambda g_table, g_blob: None)
    for t_ in (tgt, bad, tgt):
        tr2.step(o, d, t_, rp)
    assert tr2.skipped_steps == 1 and tr2.t == 2
    assert float((tr2.blob - tr.blob).abs().max()) <= 2.2 * 5e-4 and float((tr2.table - tr.table).abs().max()) <= 2.2 * 5e-4
    assert float((tr2.blob - tr.blob).abs().median()) < 1e-6


@pytest.mark.gpu
def test_classic_network_parameter_upload_stays_on_the_device_and_equals_the_host_pack(api):
    """nrf_mlp_set_params on the classic 8 x 256 network: its three matrix-core images (fp16, split, exact-fp32 density: seven regions of two element sizes) are gathers of
    [blob | merged views layer]; the gather maps are DECODED from the host packers run on probe blobs and checked against the host-packed images byte for byte when the
    handle is created (nrf_mlp_device_repack_images == 7), the merged layer is re-derived by a device kernel with the host's double sums.  A frame rendered after a device
    upload equals, bit for bit and in every precision, the frame of a network CREATED from the same parameters (host packers)."""
    L, S, R, M = api.L, api.S, api.R, api.M
    K = S.lego_K(48, 48); c2w = S.pose_spherical(35.0, -20.0, 4.0)
    sc = S.make_classic_scene()
    assert L.lib().nrf_mlp_device_repack_images(sc["mlp"]._m) == 7
    rng = np.random.default_rng(11)
    blob2 = (sc["mlp_blob"] * (1.0 + 0.3 * rng.standard_normal(sc["mlp_blob"].shape))).astype(np.float32)
    t2 = torch.as_tensor(blob2).cuda()
    L.check(L.lib().nrf_mlp_set_params(sc["mlp"]._m, C.c_void_p(t2.data_ptr()), 1, None))
    fresh_mlp = M.NeRF(8, 256, sc["embedder"].GetOutputDims(), sc["embeddirs"].GetOutputDims(), 5, (4,), True, "model", params=blob2)
    fresh = R.NeRFRenderer(sc["embedder"], sc["embeddirs"], fresh_mlp)
    for prec in (L.NRF_PREC_F16_SPLIT, L.NRF_PREC_F16_MFMA, L.NRF_PREC_F32):
        p = R.NeRFRenderParams(NSamples=32, NImportance=32, Chunk=2048, Perturb=0.0, WhiteBkgr=False, Ndc=False, UseViewdirs=True, ThinRay=True, BoundingBox=S.LEGO_BBOX, Precision=prec)
        a = sc["renderer"].Render(48, 48, K, p, c2w=c2w)
        b = fresh.Render(48, 48, K, p, c2w=c2w)
        assert torch.equal(a.Outputs.RGBMap, b.Outputs.RGBMap) and torch.equal(a.Outputs.DepthMap, b.Outputs.DepthMap), prec
        assert bool(torch.isfinite(a.Outputs.RGBMap).all())
    # ... and the host path (a host pointer) still gives the same images
    L.check(L.lib().nrf_mlp_set_params(sc["mlp"]._m, blob2.ctypes.data_as(C.c_void_p), 0, None))
    a = sc["renderer"].Render(48, 48, K, p, c2w=c2w)
    assert torch.equal(a.Outputs.RGBMap, b.Outputs.RGBMap)


@pytest.mark.gpu
def test_lerf_head_parameter_upload_stays_on_the_device_and_equals_the_host_pack(api):
    """nrf_mlp_set_params on a LeRF head with a DEVICE pointer: the Gram matrix, the fp16 / split images and the exact-fp32 density image are rebuilt by device kernels
    (mlp_lerf_pack_f16_device, mlp_lerf_pack_sigma_f32_device; round 6: the host packer's 3 ms were GPU idle time in every training step).  The handle says so
    (nrf_mlp_device_repack_images == 3: its creation compared the device packers with the host packers byte for byte), and a pass rendered after such an upload equals,
    bit for bit, the pass of a head CREATED from the same parameters (host packers) -- weights whose Gram matrix needs the fp16-range scale included."""
    L, S, R = api.L, api.S, api.R
    K = S.lego_K(64, 64); c2w = S.pose_spherical(40.0, -25.0, 4.0)
    o, d, _ = R.GetRays(64, 64, K, c2w)
    o = o.reshape(-1, 3)[::7].contiguous(); d = d.reshape(-1, 3)[::7].contiguous()
    for gain in (1.0, 40.0):
        sc = S.make_lerf_scene(log2_t=14)
        assert L.lib().nrf_mlp_device_repack_images(sc["lerf"]._m) == 3
        rng = np.random.default_rng(5)
        blob2 = (sc["blob"] * (1.0 + 0.2 * rng.standard_normal(sc["blob"].shape))).astype(np.float32)
        n3 = 768 * 256
        blob2[-n3:] *= np.float32(gain)                                     # the embedding layer: gain 40 puts max |W^T W| beyond 1024 (the Gram image's scale != 1)
        p = R.NeRFRenderParams(NSamples=32, NImportance=32, Chunk=4096, Perturb=0.0, Ndc=False, UseViewdirs=False, ReturnWeights=True, ThinRay=True, BoundingBox=sc["bbox"])
        t2 = torch.as_tensor(blob2).cuda()
        L.check(L.lib().nrf_mlp_set_params(sc["lerf"]._m, C.c_void_p(t2.data_ptr()), 1, None))
        a = sc["renderer"].Render(0, 0, None, p, rays=(o, d, None))
        from nerfpp_amd.modules import LeRF
        from nerfpp_amd.renderer import LeRFRenderer
        fresh = LeRFRenderer(sc["embedder"], LeRF(32, 2, 256, 768, 128, "lang_model", params=blob2))
        b = fresh.Render(0, 0, None, p, rays=(o, d, None))
        assert torch.equal(a.Outputs.RenderedLangEmbedding, b.Outputs.RenderedLangEmbedding) and torch.equal(a.Outputs.WeightsLE, b.Outputs.WeightsLE)
        assert bool(torch.isfinite(a.Outputs.RenderedLangEmbedding).all())


@pytest.mark.gpu
@pytest.mark.parametrize("P,out,n,ldg,ldx,in_,col0", [(100000, 256, 256, 256, 256, 256, 0), (50001, 128, 283, 128, 283, 300, 17), (40000, 256, 63, 264, 63, 319, 256),
                                                      (8192, 33, 143, 40, 144, 143, 0), (4100, 256, 128, 256, 128, 128, 0), (31, 64, 64, 64, 64, 64, 0)])
def test_gemm_tn_bf16x3_vs_float64(api, P, out, n, ldg, ldx, in_, col0):
    """nrf_gemm_tn_bf16x3 (gemm_bf16x3.hip: the weight-gradient product dW += G^T X, contraction over the points, bf16x3 arithmetic, slices of the points summed in a
    fixed order) against the float64 product: within 2e-5 of the largest entry (measured 5e-6), added to what dW held, nothing written outside its columns; aligned and
    unaligned rows (vector and element-wise load paths), ragged widths, a point count that is no multiple of 32 (tail kernel) and one below 32 (tail only);
    two calls give the same bits (no atomics)."""
    L = api.L
    gen = torch.Generator(device="cuda"); gen.manual_seed(P + out + n)
    G = torch.randn((P, ldg), device="cuda", generator=gen) * torch.pow(10.0, torch.rand((P, 1), device="cuda", generator=gen) * 6 - 6)          # gradient rows of any magnitude
    X = torch.randn((P, ldx), device="cuda", generator=gen)
    base = torch.randn((out, in_), device="cuda", generator=gen)
    want = base.double().clone()
    want[:, col0:col0 + n] += G[:, :out].double().t() @ X[:, :n].double()
    outs = []
    for _ in range(2):
        dw = base.clone()
        L.check(L.lib().nrf_gemm_tn_bf16x3(C.c_void_p(G.data_ptr()), ldg, out, C.c_void_p(X.data_ptr()), ldx, n, C.c_int64(P), C.c_void_p(dw.data_ptr()), in_, col0, None))
        outs.append(dw)
    assert torch.equal(outs[0], outs[1]), "deterministic"
    dw = outs[0]
    assert bool(torch.isfinite(dw).all())
    mask = torch.ones_like(base, dtype=torch.bool); mask[:, col0:col0 + n] = False
    assert torch.equal(dw[mask], base[mask]), "columns outside [col0, col0 + n) untouched"
    scale = (G[:, :out].double().t() @ X[:, :n].double()).abs().max()
    err = float((dw.double() - want).abs().max() / scale)
    assert err < 2e-5, err


def test_classic_and_lerf_train_steps_in_the_split_gemm_modes_follow_the_fp32_chain(api):
    """nrf_set_train_gemm(1 | 2): the classic NeRFImpl backward and the LeRF head backward with their forward / back-propagation products on the bf16 (1) / fp16 (2) matrix
    cores (bias, ReLU and the next stage's ReLU mask fused into the products' epilogues).  Against the SAME step with fp32 products (mode 0, which the goldens hold to the
    reference's autograd): the loss identical (the render is the same), nothing non-finite, every parameter-gradient tensor within 3e-3 of its largest entry in the bf16
    arithmetic (16 significant bits; measured 1.1e-4, norm-wise 2.5e-4) and within 3e-4 in the scaled fp16 arithmetic (22 bits; measured 8.6e-5, norm-wise 6.3e-5).  The
    yardstick for the latter: the same step with rocBLAS sgemm and with the hand-written fp32 FMA kernels -- two fp32 chains -- differs by 2.3e-5 / 1.9e-5
    (tools/scratch/train_gemm_agreement.py, profiles/round6/r6o_train_gemm_agreement.log): ReLUs of near-zero pre-activations decided the other way."""
    L, S, R = api.L, api.S, api.R
    from nerfpp_amd.train import Trainer, LeRFTrainer
    K = S.lego_K(200, 200); c2w = S.pose_spherical(30.0, -30.0, 4.0)
    o, d, _ = R.GetRays(200, 200, K, c2w)
    o = o.reshape(-1, 3)[::20][:1500].contiguous(); d = d.reshape(-1, 3)[::20][:1500].contiguous()
    tgt = torch.rand((o.shape[0], 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    bars = {1: (3e-3, 1e-3, 2e-3), 2: (3e-4, 2e-4, 2e-4)}          # classic: max over max, norm-wise; LeRF: norm-wise
    prev = L.lib().nrf_get_train_gemm()
    try:
        grads = {}
        for mode in (0, 1, 2):
            L.check(L.lib().nrf_set_train_gemm(mode))
            sc = S.make_classic_scene()
            tr = Trainer(sc["embedder"], sc["embeddirs"], sc["mlp"], None, sc["mlp_blob"], learning_rate=5e-4)
            rp = R.NeRFRenderParams(NSamples=32, NImportance=32, Chunk=2048, Perturb=0.0, WhiteBkgr=False, Ndc=False, UseViewdirs=True, ThinRay=True, BoundingBox=S.LEGO_BBOX,
                                    Precision=L.NRF_PREC_F32)
            lm, _ = tr.step(o, d, tgt, rp)
            grads[mode] = (tr.g_blob.clone(), float(host(lm)[0]))
        g0 = grads[0][0]
        for mode in (1, 2):
            g1 = grads[mode][0]
            assert grads[0][1] == grads[mode][1] and bool(torch.isfinite(g1).all())
            e_max, e_norm = float((g1 - g0).abs().max() / g0.abs().max()), float((g1 - g0).norm() / g0.norm())
            print("classic step, train gemm mode %d vs fp32 products: max/max %.2e norm-wise %.2e" % (mode, e_max, e_norm))
            assert e_max < bars[mode][0] and e_norm < bars[mode][1], (mode, e_max, e_norm)
        # LeRF head + language grid
        lg = {}
        tl = torch.nn.functional.normalize(torch.randn((o.shape[0], 768), device="cuda", generator=torch.Generator(device="cuda").manual_seed(6)), dim=-1)
        for mode in (0, 1, 2):
            L.check(L.lib().nrf_set_train_gemm(mode))
            sc = S.make_lerf_scene(log2_t=14)
            p = R.NeRFRenderParams(NSamples=32, NImportance=32, Chunk=4096, Perturb=0.0, Ndc=False, UseViewdirs=False, ReturnWeights=True, ThinRay=True, BoundingBox=sc["bbox"])
            tr = LeRFTrainer(sc["renderer"], sc["table"], sc["blob"], learning_rate=1e-3)
            l, _ = tr.step(o, d, tl, p)
            lg[mode] = (tr.g_blob.clone(), tr.g_table.clone(), float(host(l)[0]))
            tr.close()
        for mode in (1, 2):
            assert lg[0][2] == lg[mode][2]
            for i in (0, 1):
                a, b = lg[mode][i], lg[0][i]
                e = float((a - b).norm() / b.norm())
                print("LeRF step, train gemm mode %d vs fp32 products, tensor %d: norm-wise %.2e" % (mode, i, e))
                assert bool(torch.isfinite(a).all()) and e < bars[mode][2], (mode, i, e)
    finally:
        L.check(L.lib().nrf_set_train_gemm(prev))
