"""GPU tests of every NeRFSmall shape the library dispatches onto the matrix cores (mlp_small_mfma.hip: small_mfma_supported / dispatch_small; sigma_small_f32.hip;
mlp.hip: the device repack and the split-scale groups; render.hip: fast_path).  Cases and the float64 yardstick are tests/mlp_small_ref.py's, which
tests/test_mlp_small_shapes_host.py pins against the C oracle on the CPU.

Which test executes which instantiation k_mlp_small_mfma<2, V / 16, NL, NLC, LM, SPLIT, LMLO, GEOIN, A32> of dispatch_small()'s twelve NRF_CASE(V / 16, NL, NLC):
  rows form (LM = false), fp16 and split, all twelve at geo 0, 1, 7, 14, 15 ...... test_forward_rows_exact_on_integer_networks, test_forward_rows_random_networks,
                                                                                 test_set_params_on_the_device (geo 0, 7, 15)
  level-major fp16 (LM, !SPLIT: the whole network on both passes), all twelve ... test_integer_lattice_render, fp16 NRF_COARSE_FULL render
  level-major split with 32-bit addresses (LM, SPLIT, A32), all twelve .......... test_integer_lattice_render: the new samples of the default render; both passes with NRF_COARSE_FULL
  colour net from the geo hand-over (GEOIN, A32), V / 16 = 1 and 4, all twelve .. test_integer_lattice_render, default render (asserted by the launch count of its profile slot)
  the same variants on random scenes, six (sh, NL, NLC, geo) ..................... test_render_precisions_vs_parity_mode
  level-major split through the merge map (LM, SPLIT, !A32) ..................... test_render_precisions_vs_parity_mode: fp16 / NRF_COARSE_SIGMA_F32 runs the fp16 kernel through
                                                                                 the merge map; the split kernel without A32 needs >= 2^26 points and is not run here
  LMLO (HashEmbedder's fp32-valued features) is the 'ngp' mode's and stays with test_gpu_parity.py's scenes (geo 15).
test_integer_lattice_render runs the six scenes of test_render_precisions_vs_parity_mode and then the twelve (V, NL, NLC) with geo 7, 14, 15, 1 in turn: 18 cases.
Every GPU step runs once."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import capi as O
import mlp_small_ref as MS

pytestmark = pytest.mark.gpu

NRF_ERR_UNSUPPORTED = 3
host = lambda t: t.detach().cpu().numpy()
P = lambda t: None if t is None else t.data_ptr()
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from types import SimpleNamespace
    from nerfpp_amd import _lib as L, modules as M, renderer as R, scene as S
    return SimpleNamespace(L=L, M=M, R=R, S=S, lib=L.lib(), PRECS=(("f32", L.NRF_PREC_F32), ("f16", L.NRF_PREC_F16_MFMA), ("split", L.NRF_PREC_F16_SPLIT)))


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = (bits(got), bits(want)) if got.dtype == np.float32 and want.dtype == np.float32 else (got, want)
    bad = np.nonzero(g.reshape(-1) != w.reshape(-1))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[:5]}: {got.reshape(-1)[bad[:3]]} vs {want.reshape(-1)[bad[:3]]}"


def equals64(got, want64, what):
    """float32 results against float64 integers: equal as numbers"""
    got = np.asarray(got, np.float64)
    assert got.shape == want64.shape, (what, got.shape, want64.shape)
    bad = np.nonzero((got != want64).reshape(-1))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[:5]}: {got.reshape(-1)[bad[:3]]} vs {want64.reshape(-1)[bad[:3]]}"


def small(api, shape, blob):
    v, nl, nlc, g = shape
    return api.M.NeRFSmall(nl, MS.HIDDEN, g, nlc, MS.HIDDEN, False, 3, 64, MS.IN_CH, v, "model", params=blob)


# ------------------------------------------------------------------ (a) rows form, exact on the integer networks
COUNTS = (1, 63, 65, 257, 513)              # one point; both sides of the 64-point tile and of the 256- (fp16) / 512-point (split) block edges
SPLIT_BLOCK_PTS = 512                       # block_pts_of(true): 8 waves of 64 points
SECOND_BLOCK = {(64, 2, 2, 0): {"f16": 768 * 256 + 1, "split": 256 * SPLIT_BLOCK_PTS + 1},          # one point past the persistent grid's reach: workgroup 0 takes a second block
                (16, 3, 2, 7): {"f16": 768 * 256 + 1, "split": 256 * SPLIT_BLOCK_PTS + 1}}


@pytest.mark.parametrize("shape", MS.SHAPES, ids=MS.shape_id)
def test_forward_rows_exact_on_integer_networks(api, shape):
    """nrf_mlp_forward in NRF_PREC_F32, NRF_PREC_F16_MFMA and NRF_PREC_F16_SPLIT on sparse -1 / 0 / +1 networks with small-integer inputs: every activation is an integer
    below 2048 (asserted in float64 by the builder), so fp16 operands hold it exactly, fp32 sums are exact in any order and the split scales -- powers of two -- keep it
    exact: the output EQUALS forward64 in all three precisions.  A wrong fragment index, column map (pack_small's cmap for geo < 15) or tail guard shows at full size.
    The rows past the batch are NaN-prefilled and stay so.  (No shape needed nrf_mlp_set_split_scaling(m, 0): the default scaling is in force throughout.)"""
    blob, _, _ = MS.integer_network(shape, 11, 1)
    m = small(api, shape, blob)
    counts = {name: list(COUNTS) + ([SECOND_BLOCK[shape][name]] if shape in SECOND_BLOCK and name in SECOND_BLOCK[shape] else []) for name, _ in api.PRECS}
    for p in sorted({c for cs in counts.values() for c in cs}):
        b2, x, want = MS.integer_network(shape, 11, p)
        assert np.array_equal(b2, blob)
        xd = dev(x)
        for name, prec in api.PRECS:
            if p not in counts[name]:
                continue
            out = torch.full((p + 3, 4), float("nan"), device="cuda")
            api.L.check(api.lib.nrf_mlp_forward(m._m, P(xd), p, prec, P(out), None))
            torch.cuda.synchronize()
            got = host(out)
            assert np.isnan(got[p:]).all(), f"{MS.shape_id(shape)} {name} p {p}: rows past the batch were written"
            equals64(got[:p], want, f"{MS.shape_id(shape)} {name} p {p}")


# ------------------------------------------------------------------ (b) rows form, random networks
F16_MAX_BAR, F16_MEAN_BAR, SPLIT_BAR = 4e-3, 6e-4, 3e-6          # test_mlp_small_f16_mfma's and test_mlp_small_split_precision_vs_oracle's, here per column group


@pytest.mark.parametrize("shape", MS.SHAPES, ids=MS.shape_id)
def test_forward_rows_random_networks(api, shape):
    """333 points of synth_linear_stack networks (gain 1.6), without and with the x 30 sigma row, against the C oracle: NRF_PREC_F32 bit for bit; fp16 and split per column
    group -- rgb against max |rgb|, sigma against max |sigma| -- at the project's own bars (fp16 4e-3 max / 6e-4 mean, split 3e-6), which were set on the joint scale
    where the x 30 sigma column hides rgb.  Every shape meets them, so no bar here comes from an emulation of the arithmetic."""
    for sigma_scale in (None, 30.0):
        blob = MS.random_network(shape, 7000 + 13 * MS.SHAPES.index(shape), sigma_scale)
        x = MS.random_inputs(shape, 5, 333)
        ref = O.mlp_small(blob, x, **MS.oracle_kw(shape))
        m = small(api, shape, blob)
        xd = dev(x)
        got = {name: host(m.forward(xd, prec)) for name, prec in api.PRECS}
        what = f"{MS.shape_id(shape)} sigma x {sigma_scale}"
        same(got["f32"], ref, what + ": NRF_PREC_F32 == oracle")
        for name, split in (("f16", False), ("split", True)):
            err = MS.group_errors(got[name], ref)
            for grp in ("rgb", "sigma"):
                print(f"{what} {name} {grp}: max {err[grp][0]:.3e} mean {err[grp][1]:.3e} of the group's maximum")
                if split:
                    assert err[grp][0] < SPLIT_BAR, (what, name, grp, err[grp])
                else:
                    assert err[grp][0] <= F16_MAX_BAR and err[grp][1] < F16_MEAN_BAR, (what, name, grp, err[grp])


# ------------------------------------------------------------------ (c) nrf_mlp_set_params on the device
def has_backward_image(shape):
    """bwd_supported(): the fused backward's W^T image exists for views 16, geo 15, 3 or 4 colour layers; other shapes have four matrix-core images, not five"""
    v, nl, nlc, g = shape
    return v == 16 and g == 15 and nlc in (3, 4)


@pytest.mark.parametrize("shape", [s for s in MS.SHAPES if s[3] in (0, 7, 15)], ids=MS.shape_id)
def test_set_params_on_the_device(api, shape):
    """A handle created with blob A and moved to blob B by nrf_mlp_set_params from device memory equals, bit for bit and in all three precisions, a handle created from
    B: the gather maps decoded from the host packers on probe blobs (build_weight_maps) are right for every shape, and so are the split-scale groups -- at geo 0 the
    group of colour layer 0's geo columns is empty.  The refresh really is the device's: nrf_mlp_device_repack_images counts one map per image (fp16, split, the
    exact sigma kernel's head and tail; the backward image where the shape has one: 5 + NL + NLC there, as test_mlp_set_params_on_the_device_equals_a_freshly_packed_handle
    asserts for its two shapes, 4 + NL + NLC where the library builds no backward image) plus one per layer; 0 would be the host repack."""
    v, nl, nlc, g = shape
    blob_a, blob_b = MS.random_network(shape, 770, 30.0), MS.random_network(shape, 780, None)
    ma, mb = small(api, shape, blob_a), small(api, shape, blob_b)
    images = api.lib.nrf_mlp_device_repack_images(ma._m)
    assert images == (5 if has_backward_image(shape) else 4) + nl + nlc, (MS.shape_id(shape), images)
    if has_backward_image(shape):
        assert images >= 5 + nl + nlc
    x = dev(MS.random_inputs(shape, 8, 333))
    before = host(ma.forward(x, api.L.NRF_PREC_F16_SPLIT))
    bd = dev(blob_b)
    api.L.check(api.lib.nrf_mlp_set_params(ma._m, P(bd), 1, None))
    for name, prec in api.PRECS:
        a, b = host(ma.forward(x, prec)), host(mb.forward(x, prec))
        assert np.isfinite(b).all()
        same(a, b, f"{MS.shape_id(shape)} {name}: updated handle == fresh handle")
    assert np.abs(host(ma.forward(x, api.L.NRF_PREC_F16_SPLIT)) - before).max() > 1e-3, "the output depends on the blob"


# ------------------------------------------------------------------ (d) the fused backward refuses what it was not built for
SENTINEL = 123.0


@pytest.mark.parametrize("shape", MS.BWD_REFUSED, ids=MS.shape_id)
def test_backward_f16_refuses_and_the_fp32_backward_serves(api, shape):
    """nrf_mlp_backward_f16 on a shape outside bwd_supported() answers NRF_ERR_UNSUPPORTED and writes nothing (the gradient buffers keep their sentinel);
    nrf_mlp_backward -- the fp32 layer kernels, ragged in = V + geo -- matches the oracle at test_training_backward_stages_vs_reference_autograd's oracle bars
    (rtol 1e-4, atol 1e-6 of the largest entry) for d / dx and for dW."""
    blob = MS.random_network(shape, 4321, 30.0)
    p = 333
    x_h = MS.random_inputs(shape, 6, p)
    g_h = (np.random.RandomState(9).standard_normal((p, 4)) * 1e-3).astype(np.float32)
    m = small(api, shape, blob)
    x, gr = dev(x_h), dev(g_h)
    nb16 = max(int(api.lib.nrf_mlp_backward_f16_workspace_bytes(m._m, p)), 1 << 20)
    ws = torch.empty(nb16, dtype=torch.uint8, device="cuda")
    g_blob, g_x = torch.full((blob.size,), SENTINEL, device="cuda"), torch.full((p, MS.IN_CH), SENTINEL, device="cuda")
    rc = api.lib.nrf_mlp_backward_f16(m._m, P(x), P(gr), p, P(g_blob), P(g_x), P(ws), ws.numel(), None)
    torch.cuda.synchronize()
    assert rc == NRF_ERR_UNSUPPORTED, rc
    with pytest.raises(api.L.NrfError, match="outside the built matrix-core family"):
        api.L.check(rc)
    assert bool((g_blob == SENTINEL).all()) and bool((g_x == SENTINEL).all()), "a refused call leaves the gradients untouched"
    nb = int(api.lib.nrf_mlp_backward_workspace_bytes(m._m, p))
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda")
    g_blob, g_x = torch.zeros(blob.size, device="cuda"), torch.full((p, MS.IN_CH), float("nan"), device="cuda")
    api.L.check(api.lib.nrf_mlp_backward(m._m, P(x), P(gr), p, P(g_blob), P(g_x), P(ws), ws.numel(), None))
    torch.cuda.synchronize()
    gp_o, gx_o = O.mlp_small_backward(blob, x_h, g_h, **MS.oracle_kw(shape))
    np.testing.assert_allclose(host(g_x), gx_o, rtol=1e-4, atol=1e-6 * np.abs(gx_o).max(), err_msg="d loss / d features vs oracle")
    off = 0
    for li, (i, o) in enumerate(MS.layer_dims(shape)):
        a, b = host(g_blob)[off:off + i * o], gp_o[off:off + i * o]
        off += i * o
        assert np.abs(b).max() > 0
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-6 * np.abs(b).max(), err_msg=f"dW of layer {li} vs oracle")


@pytest.mark.parametrize("shape", MS.BWD_REFUSED, ids=MS.shape_id)
def test_trainer_f16_on_a_refused_shape_raises(api, shape):
    """Trainer(mlp_backward="f16") on such a scene: the step RAISES (the library's refusal, passed on) and leaves the parameters as they were -- it neither trains
    with untouched gradients nor falls back silently.  The fp32 trainer serves the same scene: one step changes the MLP parameters."""
    from nerfpp_amd.train import Trainer
    v, nl, nlc, g = shape
    sc = api.S.make_hash_scene(mode="cu", log2_t=14, seed=4242, table_amp=0.3, sigma_scale=3.0, sh_degree=4 if v == 16 else 8, num_layers=nl, num_layers_color=nlc, geo=g)
    o, d, _ = api.R.GetRays(16, 16, api.S.lego_K(16, 16), api.S.pose_spherical(20.0, -30.0, 4.0))
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    tgt = torch.rand((256, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    rp = api.R.NeRFRenderParams(NSamples=32, NImportance=32, Chunk=1024, Perturb=0.0, WhiteBkgr=False, Ndc=False, UseViewdirs=True, ThinRay=True,
                                BoundingBox=api.S.LEGO_BBOX, Precision=api.L.NRF_PREC_F16_SPLIT, ReturnRaw=True, KeepIntermediates=True)
    with Trainer(sc["embedder"], sc["embeddirs"], sc["mlp"], sc["table"], sc["mlp_blob"], learning_rate=1e-3, mlp_backward="f16") as tr:
        before = host(tr.blob).copy()
        with pytest.raises(api.L.NrfError, match="outside the built matrix-core family"):
            tr.step(o, d, tgt, rp)
        torch.cuda.synchronize()
        same(host(tr.blob), before, "parameters after the refused step")
    with Trainer(sc["embedder"], sc["embeddirs"], sc["mlp"], sc["table"], sc["mlp_blob"], learning_rate=1e-3, mlp_backward="f32") as tr:
        before = host(tr.blob).copy()
        loss = host(tr.step(o, d, tgt, rp)[0])
        torch.cuda.synchronize()
        after = host(tr.blob)
        assert np.isfinite(loss).all() and np.isfinite(after).all()
        off = 0
        for li, (i_, o_) in enumerate(MS.layer_dims(shape)):
            assert (after[off:off + i_ * o_] != before[off:off + i_ * o_]).any(), f"one fp32 step moves the parameters of layer {li}"
            off += i_ * o_


# ------------------------------------------------------------------ (e) through the renderer
RENDER_SCENES = [(4, 3, 4, 7), (4, 2, 2, 15), (4, 3, 3, 0), (4, 3, 4, 1), (8, 3, 4, 15), (8, 2, 2, 14)]          # (SH degree, NL, NLC, geo)
RAY_SETS = ((1, 1, 64), (3, 7, 64), (1, 9, 57), (5, 40, 64))          # test_sigma_f32_kernel_shapes_and_ragged_sizes': (rows, cols, coarse samples) of a 40 x 40 camera
scene_id = lambda sc: "sh%d-nl%d-nlc%d-g%d" % tuple(sc)


def rays_of(api, rows, cols):
    o, d, _ = api.R.GetRays(40, 40, api.S.lego_K(40, 40), api.S.pose_spherical(10.0, -30.0, 4.0), row0=17, rows=rows)
    return o.reshape(-1, 3)[:rows * cols].contiguous(), d.reshape(-1, 3)[:rows * cols].contiguous()


def grouped(got, ref, bar, what):
    """|got - ref| <= bar x max |ref| for the rgb columns and for the sigma column, each on its own scale"""
    got, ref = got.reshape(-1, 4), ref.reshape(-1, 4)
    for grp, e in MS.group_errors(got, ref).items():
        print(f"{what} {grp}: max |difference| = {e[0]:.3e} of the group's maximum (bar {bar:g})")
        assert e[0] <= bar, (what, grp, e[0])


@pytest.mark.parametrize("cfg", RENDER_SCENES, ids=scene_id)
def test_render_precisions_vs_parity_mode(api, cfg):
    """CuHashEmbedder scenes (2^14-entry tables) of six shapes, four ragged ray sets each, 32 importance samples, against NRF_PREC_F32 (which the existing tests hold
    bit-equal to the oracle):
      NRF_PREC_F16_SPLIT, default coarse mode (exact sigma kernel + geo hand-over): coarse weights and z_fine bit-identical; pixels within 1e-4; Raw within 1e-5 of each
        column group's maximum;
      NRF_PREC_F16_SPLIT, NRF_COARSE_FULL: the coarse raw within 3e-6 of each column group's maximum;
      NRF_PREC_F16_MFMA, NRF_COARSE_SIGMA_F32: z_fine bit-identical; pixels finite and within the fp16 bars (4e-3 max, 6e-4 mean of the largest pixel value)."""
    sh, nl, nlc, g = cfg
    sc = api.S.make_hash_scene(mode="cu", log2_t=14, sh_degree=sh, num_layers=nl, num_layers_color=nlc, geo=g)
    r = sc["renderer"]
    for rows, cols, ns in RAY_SETS:
        o, d = rays_of(api, rows, cols)
        what = f"{scene_id(cfg)} n {rows * cols} s {ns}"

        def render(prec, keep, **kw):
            rp = api.S.lego_render_params(sc["bbox"], ns, 32, 4096, prec, KeepIntermediates=keep, ReturnRaw=True, **kw)
            return r.Render(0, 0, None, rp, rays=(o, d, None))
        a = render(api.L.NRF_PREC_F32, True)
        rgb_a, raw_a = host(a.Outputs.RGBMap).reshape(-1, 3), host(a.Raw)
        assert host(a.Extras["weights_coarse"]).max() > 0 and np.isfinite(raw_a).all()
        b = render(api.L.NRF_PREC_F16_SPLIT, "depths")
        assert "raw_coarse" not in b.Extras
        same(host(b.Extras["weights_coarse"]), host(a.Extras["weights_coarse"]), what + ": coarse weights, exact sigma kernel == NRF_PREC_F32")
        same(host(b.Extras["z_fine"]), host(a.Extras["z_fine"]), what + ": z_fine")
        dpx = np.abs(host(b.Outputs.RGBMap).reshape(-1, 3) - rgb_a).max()
        print(f"{what} split: max pixel difference {dpx:.3e} (bar 1e-4)")
        assert dpx < 1e-4, (what, dpx)
        grouped(host(b.Raw), raw_a, 1e-5, what + " split Raw")
        bf = render(api.L.NRF_PREC_F16_SPLIT, True, CoarseMode=api.L.NRF_COARSE_FULL)
        grouped(host(bf.Extras["raw_coarse"]), host(a.Extras["raw_coarse"]), 3e-6, what + " split NRF_COARSE_FULL coarse raw")
        c = render(api.L.NRF_PREC_F16_MFMA, "depths", CoarseMode=api.L.NRF_COARSE_SIGMA_F32)
        same(host(c.Extras["z_fine"]), host(a.Extras["z_fine"]), what + ": z_fine, fp16 fine pass")
        rgb_c = host(c.Outputs.RGBMap).reshape(-1, 3)
        dc = np.abs(rgb_c - rgb_a)
        scale = np.abs(rgb_a).max()
        print(f"{what} fp16: pixel difference max {dc.max():.3e} mean {dc.mean():.3e}, largest pixel {scale:.3f} (bars {F16_MAX_BAR:g} / {F16_MEAN_BAR:g} of it)")
        assert np.isfinite(rgb_c).all() and np.isfinite(host(c.Raw)).all()
        assert dc.max() <= F16_MAX_BAR * scale and dc.mean() < F16_MEAN_BAR * scale, (what, dc.max(), dc.mean())


def stagewise(api, sc, res):
    """the network inputs of every fine depth of a render, built stage by stage -> (x [n s, 32 + V] on the device, keep [n s] bool on the host, n, s)"""
    rays, zf = res.Extras["rays_flat"], res.Extras["z_fine"]
    n, s = zf.shape
    pts = (rays[:, None, 0:3] + rays[:, None, 3:6] * zf[..., None]).reshape(-1, 3)
    emb, keep = sc["embedder"].forward(pts)
    dirs, _ = sc["embeddirs"].forward(rays[:, 8:11].contiguous())
    return torch.cat([emb, dirs[:, None, :].expand(n, s, dirs.shape[1]).reshape(n * s, -1)], 1).contiguous(), host(keep), n, s


@pytest.mark.parametrize("cfg", [(8, 2, 2, 14), (4, 3, 3, 0)], ids=scene_id)
def test_feature_reusing_fine_pass_equals_stagewise(api, cfg):
    """The default split render (sigma-only exact coarse pass that hands (sigma, geo_feat) over; the fine pass runs the whole network on its new samples and the colour
    net alone on its coarse depths) against the stage-wise evaluation of all fine depths, as test_feature_reusing_fine_pass_equals_stagewise_cu does for the default
    scene: new samples == the split-precision MLP bit for bit; at the coarse depths sigma == the NRF_PREC_F32 MLP's bit for bit and rgb within 2e-5 of it and no
    further from it than 1.5 x the full split network is."""
    sh, nl, nlc, g = cfg
    sc = api.S.make_hash_scene(mode="cu", log2_t=14, sh_degree=sh, num_layers=nl, num_layers_color=nlc, geo=g)
    o, d = rays_of(api, 5, 40)
    rp = api.S.lego_render_params(sc["bbox"], 64, 32, 77, api.L.NRF_PREC_F16_SPLIT, ReturnRaw=True, KeepIntermediates="depths")          # ragged chunks
    res = sc["renderer"].Render(0, 0, None, rp, rays=(o, d, None))
    x, keep, n, s = stagewise(api, sc, res)
    assert s == 96
    ref, ref32 = host(sc["mlp"].forward(x, api.L.NRF_PREC_F16_SPLIT)), host(sc["mlp"].forward(x, api.L.NRF_PREC_F32))
    ref[~keep, 3] = 0; ref32[~keep, 3] = 0
    got = host(res.Raw).reshape(-1, 4)
    zf, zc = host(res.Extras["z_fine"]), host(res.Extras["z_coarse"])
    coarse = (zf[:, :, None] == zc[:, None, :]).any(-1)
    tie = np.zeros_like(coarse)
    eq = zf[:, 1:] == zf[:, :-1]
    tie[:, 1:] |= eq; tie[:, :-1] |= eq          # a new sample exactly on a coarse depth cannot be told from it: such pairs are left out
    # check_default_split_fine_pass allows 1e-4 of its 307 200 depths; of the 19 200 here that would be a single pair, so the allowance is four pairs (8 depths)
    assert tie.sum() <= 8, tie.sum()
    assert (coarse & ~tie).sum() + tie.sum() // 2 == n * zc.shape[1], "every coarse depth is among the fine depths"
    tie = tie.reshape(-1); new = ~coarse.reshape(-1) & ~tie; coarse = coarse.reshape(-1) & ~tie
    assert new.sum() + coarse.sum() + tie.sum() == n * s and new.sum() >= n * 32 - 8
    same(got[new], ref[new], scene_id(cfg) + ": new samples == stage-wise split-precision MLP")
    same(got[coarse, 3], ref32[coarse, 3], scene_id(cfg) + ": sigma at the coarse depths == NRF_PREC_F32")
    scale = np.abs(ref32[:, :3]).max()
    err, full = np.abs(got[coarse, :3] - ref32[coarse, :3]).max(), np.abs(ref[coarse, :3] - ref32[coarse, :3]).max()
    print(f"{scene_id(cfg)}: rgb at the coarse depths vs fp32: {err / scale:.3e} of the maximum (bar 2e-5); the full split network: {full / scale:.3e}")
    assert err <= 2e-5 * scale and err <= 1.5 * full + 1e-7 * scale


LATTICE_BBOX = np.array([0, 0, 0, 63, 63, 63], np.float32)
# the six scenes of test_render_precisions_vs_parity_mode, then the twelve instantiations with geo 7, 14, 15, 1 in turn (never 0 there: rgb must say something)
LATTICE_CASES = [(sh * sh, nl, nlc, g) for sh, nl, nlc, g in RENDER_SCENES] + [inst + ((7, 14, 15, 1)[i % 4],) for i, inst in enumerate(MS.INSTANTIATIONS)]
assert len(set(LATTICE_CASES)) == 18


def lattice_scene(api, shape):
    """A CuHashEmbedder scene whose coarse depths fall on lattice points of every level: the box is [0, 63]^3, every level's position scale is 63 (so a point's grid
    coordinate is the point), the table holds -2, -1, 1, 2 (no zeros: a corner value v read with a fraction of 1e-5 rounds to v in fp16, a zero would not round to 0), and
    the rays run along +z from z = -1 through lattice columns: with 64 coarse samples, depth i lies at z = i up to 6e-5 (fp32 rounding of the depths).
    -> (scene, o, d, features of the coarse depths [21 * 64, 32] on the host: they do not depend on the network)"""
    v, nl, nlc, g = shape
    sc = api.S.make_hash_scene(mode="cu", log2_t=14, sh_degree=4 if v == 16 else 8, num_layers=nl, num_layers_color=nlc, geo=g, bbox=LATTICE_BBOX)
    rng = np.random.default_rng(31)
    sc["embedder"].set_table(rng.choice([-2.0, -1.0, 1.0, 2.0], size=sc["table"].size).astype(np.float32))
    sc["embedder"].set_level_scales(np.full(16, 63.0, np.float32))
    iy, ix = np.meshgrid([20.0, 30.0, 40.0], np.arange(5.0, 12.0), indexing="ij")
    o = dev(np.stack([ix.reshape(-1), iy.reshape(-1), np.full(21, -1.0)], 1))
    d = dev(np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (21, 1)))
    rays = torch.empty((21, 11), device="cuda")
    api.L.check(api.lib.nrf_pack_rays(P(o), P(d), LATTICE_BBOX.ctypes.data, 21, 1, P(rays), None))
    t = torch.linspace(0, 1, 64, device="cuda")
    z = rays[:, 6:7] * (1 - t) + rays[:, 7:8] * t          # (within an ulp of nrf_z_vals: only used to pick the network)
    emb, _ = sc["embedder"].forward((rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]).reshape(-1, 3))
    return sc, o, d, host(emb)


def lattice_network(shape, feats):
    """The first integer network (seeds 11, 12, ...) that says something on the lattice features `feats`: sigma varies, a colour channel varies and every geo column
    moves rgb.  Colour layer 0 reads no view feature (spherical harmonics are not integers), so rgb is an exact function of the geo features -- except at geo 0,
    where the colour net would then have no input at all: there the view weights stay, rgb is non-zero and is compared at the precision's bar.  -> blob"""
    v, nl, nlc, g = shape
    assert (feats == np.rint(feats)).all() and np.abs(feats).max() <= 2, "the coarse depths carry small-integer features"
    x = np.concatenate([feats, np.zeros((feats.shape[0], v), np.float32)], 1)
    for seed in range(11, 43):
        mats = MS.matrices(MS.integer_network(shape, seed, 1)[0], shape)
        views = mats[nl][:, :v].copy()
        mats[nl][:, :v] = 0.0
        blob = np.concatenate([w.reshape(-1) for w in mats]).astype(np.float32)
        out = MS.check_integer_network(blob, x, shape, want_varied=False)
        if np.ptp(out[:, 3]) > 0 and (not g or (np.ptp(out[:, :3], axis=0).max() > 0 and MS.geo_columns_matter(blob, x, shape))):
            if not g:
                mats[nl][:, :v] = views
                blob = np.concatenate([w.reshape(-1) for w in mats]).astype(np.float32)
            return blob
    raise AssertionError("no integer network whose outputs vary on the lattice features")


@pytest.mark.parametrize("shape", LATTICE_CASES, ids=MS.shape_id)
def test_integer_lattice_render(api, shape):
    """Level-major kernels and the geo hand-over, exactly: on the lattice scene the features of the coarse depths are small integers, so the Raw of a 3 x 7-ray, 64 + 32
    sample render EQUALS forward64 of the features the encoder produced (read back with the embedder's forward) at every depth whose features are integers -- in
    NRF_PREC_F32, in the default split render (asserted to take the geo hand-over: the colour-only launch is counted in its own profile slot), with NRF_COARSE_FULL in
    split precision and in fp16.  A geo hand-over row off by one (sigma_small_f32.hip's tail of 1 + geo rows, pack_small's cmap through perm_row) changes rgb at full
    size here.  At geo 0 sigma is exact and rgb, which reads the spherical harmonics there, is held to 2e-6 (fp32), 1e-5 (split) and 4e-3 (fp16) of its maximum."""
    v, nl, nlc, g = shape
    sc, o, d, feats = lattice_scene(api, shape)
    blob = lattice_network(shape, feats)
    mlp = small(api, shape, blob)
    r = api.R.NeRFRenderer(sc["embedder"], sc["embeddirs"], mlp)
    ms, cnt = (C.c_double * len(api.L.NRF_PROF_NAMES))(), (C.c_int64 * len(api.L.NRF_PROF_NAMES))()
    for name, prec, kw, rgb_bar in (("NRF_PREC_F32", api.L.NRF_PREC_F32, dict(CoarseMode=api.L.NRF_COARSE_FULL), 2e-6), ("split, geo hand-over", api.L.NRF_PREC_F16_SPLIT, {}, 1e-5),
                                    ("split NRF_COARSE_FULL", api.L.NRF_PREC_F16_SPLIT, dict(CoarseMode=api.L.NRF_COARSE_FULL), 1e-5),
                                    ("fp16 NRF_COARSE_FULL", api.L.NRF_PREC_F16_MFMA, dict(CoarseMode=api.L.NRF_COARSE_FULL), F16_MAX_BAR)):
        rp = api.S.lego_render_params(LATTICE_BBOX, 64, 32, 4096, prec, ReturnRaw=True, KeepIntermediates="depths", **kw)
        api.lib.nrf_profile_enable(1)
        try:
            api.lib.nrf_profile_read(ms, cnt, 1)
            got = r.Render(0, 0, None, rp, rays=(o, d, None))
            torch.cuda.synchronize()
            api.lib.nrf_profile_read(ms, cnt, 1)
        finally:
            api.lib.nrf_profile_enable(0)
        colour_only = cnt[api.L.NRF_PROF_NAMES.index("mlp_colour")]
        assert (colour_only > 0) == (not kw), f"{name}: {colour_only} colour-only launches"
        x, keep, n, s = stagewise(api, sc, got)
        xh = host(x)
        if g:
            xh[:, MS.IN_CH:] = 0.0          # the view features meet zero weights: left out of the float64 model, whose inputs are then all integers
        whole = (xh[:, :MS.IN_CH] == np.rint(xh[:, :MS.IN_CH])).all(1)
        assert (n, s) == (21, 96) and whole.sum() >= n * 64, f"the coarse depths carry integer features: {whole.sum()} of {n * s} rows"
        want = MS.forward64(blob, xh[whole], shape)
        want[~keep[whole], 3] = 0
        raw = host(got.Raw).reshape(-1, 4)[whole]
        what = f"{MS.shape_id(shape)} {name}"
        assert np.ptp(want[:, 3]) > 0 and np.abs(want[:, :3]).max() > 0
        if g:
            equals64(raw, want, what)
        else:
            equals64(raw[:, 3:], want[:, 3:], what + " sigma")
            e = np.abs(raw[:, :3] - want[:, :3]).max() / np.abs(want[:, :3]).max()
            print(f"{what}: rgb max |difference| = {e:.3e} of its maximum (bar {rgb_bar:g})")
            assert e <= rgb_bar, (what, e)
