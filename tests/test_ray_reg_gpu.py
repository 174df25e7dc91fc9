"""GPU tests of the ray regularisers (ray_reg.hip: nrf_ray_regularizers; Trainer(distortion_loss_weight, sparsity_loss_weight)).  The yardstick is tests/ray_reg_ref.py
(float64 torch, the O(s^2) double sum, autograd on the CPU), pinned by tests/test_ray_reg_host.py.  Every GPU step runs once."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import ordered_sum_ref as OS
from conftest import load_golden
import ray_reg_ref as RR

pytestmark = pytest.mark.gpu

P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
host = lambda t: t.detach().cpu().numpy()
dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
W_DIST, W_SPARSE = 0.7, 0.3


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from types import SimpleNamespace
    from nerfpp_amd import _lib as L, modules as M, renderer as R, scene as S, train as T
    assert hasattr(L.lib(), "nrf_ray_regularizers")
    return SimpleNamespace(L=L, M=M, R=R, S=S, T=T)


def close(got, ref, what, keep=None, rtol=2e-4, atol_rel=1e-5):
    """rtol 2e-4, atol 1e-5 * max|ref|: the bar of this chain against the reference's autograd (test_training_backward_stages_vs_reference_autograd)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    atol = atol_rel * np.abs(ref).max()
    err = np.abs(got - ref) - (atol + rtol * np.abs(ref))
    if keep is not None:
        err = np.where(keep, err, -np.inf)
    print(f"{what}: max |got - ref| = {np.where(keep, np.abs(got - ref), 0).max() if keep is not None else np.abs(got - ref).max():.3e}, max |ref| = {np.abs(ref).max():.3e}, "
          f"worst excess over the bar = {err.max():.3e}")
    assert np.isfinite(got).all() and (err <= 0).all(), what


def call(api, b, w_dist, w_sparse, g_init=None, want_weights=False, ws_bytes=None, c=None, s=None, check=True):
    """One nrf_ray_regularizers call on the batch b (ray_reg_ref.seeded_inputs' layout) -> (g_raw [n,s,c], losses [2], weights [n,s] | None, status)."""
    lib = api.L.lib()
    n, s0, c0 = b["raw"].shape
    s, c = s0 if s is None else s, c0 if c is None else c
    raw, z, d, nz = dev(b["raw"]), dev(b["z"]), dev(b["d"]), dev(b["noise"])
    g = torch.zeros((n, s0, c0), device="cuda") if g_init is None else dev(g_init)
    losses = torch.full((2,), -5.0, device="cuda")
    wout = torch.full((n, s0), -7.0, device="cuda") if want_weights else None
    nb = int(lib.nrf_ray_regularizers_workspace_bytes(C.c_int64(n), s0)) if ws_bytes is None else ws_bytes
    ws = torch.empty((max(nb, 8),), dtype=torch.uint8, device="cuda")
    rc = lib.nrf_ray_regularizers(P(raw), P(z), P(d), 3, C.c_int64(n), s, c, P(nz), C.c_float(b["noise_std"]), C.c_float(w_dist), C.c_float(w_sparse), P(g), P(losses),
                                  P(wout), P(ws), C.c_size_t(nb), None)
    torch.cuda.synchronize()
    if check:
        api.L.check(rc)
    return host(g), host(losses), None if wout is None else host(wout), rc


def render_weights(api, b):
    """nrf_raw2outputs(_noise)'s Weights of the batch."""
    lib = api.L.lib()
    n, s, c = b["raw"].shape
    raw, z, d, nz = dev(b["raw"]), dev(b["z"]), dev(b["d"]), dev(b["noise"])
    w = torch.empty((n, s), device="cuda"); rgb = torch.empty((n, 3), device="cuda")
    if nz is None:
        api.L.check(lib.nrf_raw2outputs(P(raw), P(z), P(d), 3, C.c_int64(n), s, c, 0, P(rgb), None, None, P(w), None, None))
    else:
        api.L.check(lib.nrf_raw2outputs_noise(P(raw), P(z), P(d), 3, C.c_int64(n), s, c, 0, P(nz), C.c_float(b["noise_std"]), P(rgb), None, None, P(w), None, None))
    torch.cuda.synchronize()
    return host(w)


def check_against_yardstick(api, b, tag, leave_out_kinks):
    ref = RR.reference(b["raw"], b["z"], b["d"], b["noise"], b["noise_std"])
    keep = ~ref["kink"] if leave_out_kinks else np.ones_like(ref["kink"])
    assert (~keep).mean() <= RR.MAX_KINK_SHARE
    for wd, ws in ((1.0, 0.0), (0.0, 1.0), (W_DIST, W_SPARSE)):
        g, losses, w, _ = call(api, b, wd, ws, want_weights=True)
        assert not g[..., :3].any() and not g[..., 4:].any()
        want = wd * ref["g_dist"] + ws * ref["g_sparse"]
        close(g[..., 3], want, f"{tag} weights ({wd}, {ws}): d / d raw[..., 3]", keep)
        if wd:
            close(losses[0], ref["losses"][0], f"{tag} weights ({wd}, {ws}): L_dist")
        else:
            assert losses[0] == 0.0
        if ws:
            close(losses[1], ref["losses"][1], f"{tag} weights ({wd}, {ws}): L_sparse")
        else:
            assert losses[1] == 0.0
        assert np.array_equal(bits(w), bits(render_weights(api, b))), "d_weights_out == the render's Weights bit for bit"
        close(w, ref["weights"], f"{tag}: weights vs the restatement")
    return ref


# ------------------------------------------------------------------ 1. the kernel against the yardstick
@pytest.mark.parametrize("seed,n,s,c,nz", RR.seeded_cases())
def test_kernel_vs_restatement_seeded(api, seed, n, s, c, nz):
    """Both loss words and the added gradient on the seeded batches (n in {64, 4096}, s in {1, 5, 64, 192}, c in {4, 7}, with and without noise), each term alone and both
    together, rtol 2e-4, atol 1e-5 * max|ref|; the kink samples (ray_reg_ref.kinks, at most 0.1 %) are left out of the gradient comparison."""
    b = RR.seeded_inputs(seed, n, s, c, nz)
    ref = check_against_yardstick(api, b, f"seed {seed} n {n} s {s} c {c} noise {nz}", True)
    if s == 1:
        assert not ref["losses"].any()
    else:
        assert ref["losses"][0] > 0 and ref["losses"][1] > 0 and np.abs(ref["g_dist"]).max() > 0


def test_losses_have_the_bits_of_the_ordered_finish_pass(api):
    """n = 1025 rays of 64 samples, four rays per block: 257 partial pairs, so the finish pass makes a second strided trip, one entry long.  The partials
    ([blocks][2] doubles after the align_up(n * s * 4, 8) bytes of the row scratch) are read back: losses == float32(finish(column) / n), bit for bit."""
    n, s, c = 1025, 64, 4
    blocks, at = -(-n // 4), -(-n * s * 4 // 8) * 8
    assert blocks == 257
    b = RR.seeded_inputs(2000, n, s, c, False)
    b["z"][-1] = b["z"][-2]          # (every 16th ray has no span and adds nothing; the last block is ray 1024 alone: give it one)
    lib = api.L.lib()
    raw, z, d = dev(b["raw"]), dev(b["z"]), dev(b["d"])
    g, losses = torch.zeros((n, s, c), device="cuda"), torch.full((2,), -5.0, device="cuda")
    nb = int(lib.nrf_ray_regularizers_workspace_bytes(C.c_int64(n), s))
    assert nb == at + blocks * 2 * 8
    ws = torch.zeros((nb,), dtype=torch.uint8, device="cuda")
    api.L.check(lib.nrf_ray_regularizers(P(raw), P(z), P(d), 3, C.c_int64(n), s, c, None, C.c_float(0.0), C.c_float(W_DIST), C.c_float(W_SPARSE), P(g), P(losses), None,
                                         P(ws), C.c_size_t(nb), None))
    torch.cuda.synchronize()
    losses, parts = host(losses), host(ws[at:].view(torch.float64)).reshape(blocks, 2)
    want = np.array([np.float32(OS.finish(parts[:, k]) / np.float64(n)) for k in (0, 1)])
    print(f"losses {losses}, float32(finish(partials) / n) {want}, numpy's sums {parts.sum(0)}")
    assert np.isfinite(parts).all() and (parts > 0.0).all()
    assert np.array_equal(bits(losses), bits(want))


@pytest.mark.parametrize("tag", ["raw2out_192", "raw2out_64", "train_hash"])
def test_kernel_vs_restatement_golden_inputs(api, tag):
    """The compiled reference's own raw / z / rays_d (nothing left out: no noise, so fp32 and fp64 agree on every sign of sigma)."""
    g = load_golden(tag)
    if tag == "train_hash":
        b = dict(raw=g["s1_fine_raw"], z=g["s1_fine_z"], d=g["rays_d"], noise=None, noise_std=0.0)
    else:
        b = dict(raw=g["raw"], z=g["z"], d=g["d"], noise=None, noise_std=0.0)
    ref = check_against_yardstick(api, b, tag, False)
    assert ref["losses"][0] > 0


# ------------------------------------------------------------------ 2. bits
@pytest.mark.parametrize("nz", [False, True])
def test_bits(api, nz):
    """Two runs give identical d_losses and d_g_raw; the gradient is ADDED to column 3 of a pre-filled d_g_raw and no other column changes; rays without a span and s == 1
    give an exact 0 and leave their rows alone; both weights 0 leave d_g_raw untouched.  (d_weights_out against the render bit for bit: test 1, every case.)"""
    b = RR.seeded_inputs(77, 1000, 192, 7, nz)
    rng = np.random.default_rng(3)
    pre = rng.standard_normal(b["raw"].shape).astype(np.float32)
    g0, l0, _, _ = call(api, b, W_DIST, W_SPARSE, g_init=pre)
    g1, l1, _, _ = call(api, b, W_DIST, W_SPARSE, g_init=pre)
    assert np.array_equal(bits(g0), bits(g1)) and np.array_equal(bits(l0), bits(l1))
    assert np.array_equal(bits(g0[..., :3]), bits(pre[..., :3])) and np.array_equal(bits(g0[..., 4:]), bits(pre[..., 4:]))
    gz, _, _, _ = call(api, b, W_DIST, W_SPARSE)
    assert np.array_equal(g0[..., 3], pre[..., 3] + gz[..., 3]), "column 3: pre-filled value + the gradient, one fp32 addition"
    flat = b["z"][:, -1] == b["z"][:, 0]
    assert flat.sum() == 63 and np.array_equal(bits(g0[flat]), bits(pre[flat])) and not gz[flat].any() and np.abs(gz[~flat][..., 3]).max() > 0
    b_flat = {**b, "z": np.ascontiguousarray(np.repeat(b["z"][:, :1], 192, 1))}
    gf, lf, _, _ = call(api, b_flat, W_DIST, W_SPARSE, g_init=pre)
    assert np.array_equal(bits(gf), bits(pre)) and not lf.any()
    b1 = RR.seeded_inputs(78, 1000, 1, 4, nz)
    pre1 = rng.standard_normal(b1["raw"].shape).astype(np.float32)
    gs, ls, _, _ = call(api, b1, W_DIST, W_SPARSE, g_init=pre1)
    assert np.array_equal(bits(gs), bits(pre1)) and not ls.any()
    gn, ln, wn, _ = call(api, b, 0.0, 0.0, g_init=pre, want_weights=True)
    assert np.array_equal(bits(gn), bits(pre)) and not ln.any() and (wn == -7.0).all()


# ------------------------------------------------------------------ 3. refusals
def test_refused_arguments(api):
    b = RR.seeded_inputs(79, 64, 64, 4, False)
    pre = np.full(b["raw"].shape, 2.5, np.float32)
    need = int(api.L.lib().nrf_ray_regularizers_workspace_bytes(C.c_int64(64), 64))
    assert need >= 64 * 64 * 4
    for kw, w in ((dict(), (-1.0, 0.0)), (dict(), (0.0, -0.5)), (dict(), (float("nan"), 1.0)), (dict(), (1.0, float("inf"))), (dict(s=0), (1.0, 1.0)),
                  (dict(c=3), (1.0, 1.0)), (dict(c=5), (1.0, 1.0)), (dict(c=8), (1.0, 1.0)), (dict(ws_bytes=need - 8), (1.0, 1.0)), (dict(ws_bytes=0), (1.0, 1.0))):
        g, losses, _, rc = call(api, b, w[0], w[1], g_init=pre, check=False, **kw)
        assert rc != api.L.NRF_OK, (kw, w)
        with pytest.raises(api.L.NrfError):
            api.L.check(rc)
        assert np.array_equal(g, pre) and (losses == -5.0).all(), "a refused call launches nothing"
        g, losses, _, rc = call(api, b, 1.0, 1.0, g_init=pre)          # a valid call right afterwards
        assert rc == api.L.NRF_OK and losses[0] > 0 and losses[1] > 0 and not np.array_equal(g[..., 3], pre[..., 3])


# ------------------------------------------------------------------ 4. the trainer's three paths
def camera_rays(api, h, theta=30.0):
    K = api.S.lego_K(h, h)
    o, d, _ = api.R.GetRays(h, h, K, api.S.pose_spherical(theta, -30.0, 4.0))
    return o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()


def path_setup(api, path):
    """-> (scene, Trainer keyword arguments, render parameters)"""
    common = dict(Chunk=32768, Perturb=0.0, WhiteBkgr=False, Ndc=False, UseViewdirs=True, ThinRay=True, BoundingBox=api.S.LEGO_BBOX)
    if path == "classic":
        sc = api.S.make_classic_scene()
        return sc, dict(), api.R.NeRFRenderParams(NSamples=64, NImportance=0, Precision=api.L.NRF_PREC_F32, **common)
    if path == "f32":
        sc = api.S.make_hash_scene(mode="ngp", log2_t=14, seed=5000)
        return sc, dict(mlp_backward="f32", hash_backward="f32"), api.R.NeRFRenderParams(NSamples=64, NImportance=0, Precision=api.L.NRF_PREC_F32, RawNoiseStd=0.5, **common)
    sc = api.S.make_hash_scene(mode="cu", log2_t=14, table_amp=1e-2, sigma_scale=4.0)
    return sc, dict(mlp_backward="f16", hash_backward="binned"), api.R.NeRFRenderParams(NSamples=64, NImportance=128, Precision=api.L.NRF_PREC_F16_SPLIT, **common)


def make_trainer(api, sc, kw, **extra):
    return api.T.Trainer(sc["embedder"], sc["embeddirs"], sc["mlp"], sc.get("table"), sc["mlp_blob"], learning_rate=1e-3, **kw, **extra)


@pytest.mark.parametrize("path", ["classic", "f32", "f16"])
def test_trainer_composition(api, path):
    """One backward() with both weights on and one with both off on the same render: g_raw[..., 3] with the weights on equals the off-run's g_raw as it stands before
    nrf_mask_sigma_grad plus the standalone kernel's output (fp32), then masked -- bit for bit; ray_losses are the standalone call's loss words; the f16 path still reads
    the render's features.  (f32 path: with RawNoiseStd > 0, the regenerated draws go to the new call as they go to the RawToOutputs backward.)"""
    lib = api.L.lib()
    sc, kw, rp = path_setup(api, path)
    o, d = camera_rays(api, 32)
    n = o.shape[0]
    tgt = torch.rand((n, 3), generator=torch.Generator().manual_seed(3)).cuda()
    p = copy.copy(rp)
    p.ReturnRaw, p.KeepIntermediates, p.Seed = True, "depths", 1234
    s = p.NSamples + p.NImportance
    with make_trainer(api, sc, kw, distortion_loss_weight=W_DIST, sparsity_loss_weight=W_SPARSE) as tr:
        res = tr.renderer.Render(0, 0, None, p, rays=(o, d, None))
        tr.backward(res, tgt, s, False, params=p)
        torch.cuda.synchronize()
        on, ray_losses = host(tr.last["g_raw"]), host(tr.ray_losses)
        if path == "f16":
            assert tr.reused_render_features is True
        tr.distortion_loss_weight = tr.sparsity_loss_weight = 0.0
        tr.backward(res, tgt, s, False, params=p)
        torch.cuda.synchronize()
        off = host(tr.last["g_raw"])
        if path == "f16":
            assert tr.reused_render_features is True
        # the off-run's g_raw before the mask: the RawToOutputs backward again (deterministic), checked against the off-run after masking
        rays, raw = res.Extras["rays_flat"], res.Raw
        z = res.Extras["z_fine"] if "z_fine" in res.Extras else res.Extras["z_coarse"]
        c = raw.shape[-1]
        fine = "z_fine" in res.Extras
        noise = api.R.RngFill(int(p.Seed), api.L.NRF_RNG_NOISE_FINE if fine else api.L.NRF_RNG_NOISE_COARSE, 0, n * s, normal=True, device=rays.device) if p.RawNoiseStd > 0 else None
        g_rgb = tr.last["g_rgb"]
        pre = torch.empty_like(raw)
        api.L.check(lib.nrf_raw2outputs_backward_noise(P(raw), P(z), C.c_void_p(rays.data_ptr() + 12), rays.shape[1], C.c_int64(n), s, c, 0, P(noise), C.c_float(p.RawNoiseStd),
                                                       P(g_rgb), P(pre), None))
        b = dict(raw=host(raw).reshape(n, s, c), z=host(z), d=host(rays[:, 3:6]), noise=None if noise is None else host(noise).reshape(n, s), noise_std=float(p.RawNoiseStd))
        alone, losses, _, _ = call(api, b, W_DIST, W_SPARSE)
        assert np.abs(alone[..., 3]).max() > 0 and np.array_equal(bits(ray_losses), bits(losses)) and losses[0] > 0 and losses[1] > 0

        def masked(g):
            g = g.clone()
            if path == "f32":
                _, keep = tr.embedder.forward(tr.last["pts"])
                k8 = keep.to(torch.uint8)
                api.L.check(lib.nrf_mask_sigma_grad(P(k8), C.c_int64(n * s), c, P(g), None))
                assert 0 < int((~keep).sum()) < keep.numel()
            elif path == "f16":
                v = tr.renderer.feature_view()
                assert v is not None and v["n"] == n and v["sf"] == s
                api.L.check(lib.nrf_mask_sigma_grad_src(C.c_void_p(v["keep"]), C.c_void_p(v["src"]), C.c_int64(n * s), c, P(g), None))
            torch.cuda.synchronize()
            return host(g).reshape(n, s, c)
        assert np.array_equal(bits(masked(pre)), bits(off.reshape(n, s, c))), "the off-run is the RawToOutputs backward, masked"
        summed = pre.reshape(n, s, c).clone()
        summed[..., 3] += dev(alone[..., 3])
        want = masked(summed.reshape(raw.shape))
        assert np.array_equal(bits(want), bits(on.reshape(n, s, c)))
        assert not np.array_equal(on, off)


# ------------------------------------------------------------------ 5. zero weights change nothing
def test_zero_weights_change_nothing_f32(api):
    """A Trainer built with both weights 0.0 against one built without them, fp32 backward: gradients, losses, table and blob after 3 steps, bit for bit.  The table gradient
    goes through the order-free fixed-point scatter (hash_backward packed), as in test_normal_train_gpu."""
    o, d = camera_rays(api, 32)
    tgt = torch.rand((1024, 3), generator=torch.Generator().manual_seed(4)).cuda()
    _, _, rp = path_setup(api, "f32")
    runs = []
    for extra in ({}, dict(distortion_loss_weight=0.0, sparsity_loss_weight=0.0)):
        sc = api.S.make_hash_scene(mode="cu", log2_t=14, seed=5000)
        with make_trainer(api, sc, dict(mlp_backward="f32", hash_backward="packed"), **extra) as tr:
            rec = []
            for _ in range(3):
                lm, _ = tr.step(o, d, tgt, rp)
                rec += [host(lm), host(tr.g_blob), host(tr.g_table), host(tr.last["g_raw"])]
            rec += [host(tr.blob), host(tr.table), host(tr.ray_losses)]
            runs.append(rec)
    for a, b in zip(*runs):
        assert np.array_equal(bits(a), bits(b))
    assert not runs[1][-1].any() and np.abs(runs[0][1]).max() > 0 and np.abs(runs[0][2]).max() > 0


def test_zero_weights_change_nothing_f16(api):
    """The same on the headline path (CuHash, 64 + 128, mlp_backward="f16", binned scatter, render features reused), 3 steps.  The fused fp16 backward adds its waves' and
    workgroups' weight-gradient tiles with float atomics: two runs of the SAME Trainer arguments already differ in the last bits of g_blob (seen: the two default-built
    trainers below differ from each other, see the printed counts; test_training_backward_reads_the_features_its_forward_render_encoded states it and sets the bar of
    2e-6 * max for that sum), so "bit for bit after 3 steps" cannot hold for anything downstream of it, with or without the new arguments.  What is asked instead, and no
    less wherever the step is reproducible: the trainers take every step from the same state (after a step the default-built trainer's parameters and Adam moments are copied
    to the others), and per step the losses, g_raw, g_table, the table and ray_losses are equal bit for bit; g_blob is equal to the bar above, and the blob is equal bit for
    bit in every entry whose g_blob bits are equal (Adam is elementwise)."""
    o, d = camera_rays(api, 32)
    tgt = torch.rand((1024, 3), generator=torch.Generator().manual_seed(4)).cuda()
    trs = []
    for extra in ({}, dict(distortion_loss_weight=0.0, sparsity_loss_weight=0.0), {}):
        sc, kw, rp = path_setup(api, "f16")
        trs.append(make_trainer(api, sc, kw, **extra))
    a, b, a2 = trs
    try:
        for step in range(3):
            rec = []
            for tr in trs:
                lm, _ = tr.step(o, d, tgt, rp)
                assert tr.reused_render_features is True and tr.skipped_steps == 0
                rec.append(dict(lm=host(lm), g_raw=host(tr.last["g_raw"]), g_table=host(tr.g_table), table=host(tr.table), g_blob=host(tr.g_blob), blob=host(tr.blob)))
            ra, rb, ra2 = rec
            print(f"step {step}: g_blob entries with different bits: default vs zero weights {int((bits(ra['g_blob']) != bits(rb['g_blob'])).sum())}, "
                  f"default vs default {int((bits(ra['g_blob']) != bits(ra2['g_blob'])).sum())} of {ra['g_blob'].size}")
            for k in ("lm", "g_raw", "g_table", "table"):
                assert np.array_equal(bits(ra[k]), bits(rb[k])), (step, k)
            assert np.abs(ra["g_raw"]).max() > 0 and np.abs(ra["g_table"]).max() > 0 and np.abs(ra["g_blob"]).max() > 0
            assert np.abs(ra["g_blob"].astype(np.float64) - rb["g_blob"]).max() <= 2e-6 * np.abs(ra["g_blob"]).max()
            eq = bits(ra["g_blob"]) == bits(rb["g_blob"])
            assert eq.any() and np.array_equal(bits(ra["blob"])[eq], bits(rb["blob"])[eq])
            assert not host(b.ray_losses).any()
            for tr in (b, a2):
                for name in ("blob", "table", "m_blob", "v_blob", "m_table", "v_table"):
                    getattr(tr, name).copy_(getattr(a, name))
                tr._push_params()
                assert tr.t == a.t and tr.lr == a.lr
    finally:
        for tr in trs:
            tr.close()


def test_negative_weights_are_refused_by_the_trainer(api):
    sc, kw, _ = path_setup(api, "f32")
    for extra in (dict(distortion_loss_weight=-1.0), dict(sparsity_loss_weight=-1e-3), dict(distortion_loss_weight=float("nan"))):
        with pytest.raises(api.L.NrfError):
            make_trainer(api, sc, kw, **extra)


# ------------------------------------------------------------------ 6. it regularises
def test_it_regularises(api):
    """ngp synthetic scene, targets = the scene's own render of its initial parameters from four views; from one initial state 200 steps x 1 024 rays with the weights on
    and with both 0, same seeds.  On a held-out view's 1 024 rays the unweighted L_dist and L_sparse of the regularised run are below the plain run's (strict; the direction
    only).  The weights (distortion 1, sparsity 1e-4) are chosen by the size of the two terms on this scene at the start (a dense fog: L_dist ~ 0.1, L_sparse ~ 130 per ray)
    so that the weighted distortion term leads: lowering sigma alone, which is all the sparsity term asks for, thins the fog, lengthens a ray's support and RAISES L_dist
    (seen with weights 1e-2 / 1e-4, where the weighted sparsity term was ten times the distortion term: L_dist 0.104 -> 0.153, L_sparse 133 -> 30).  Values seen on the
    MI355X: DESIGN.md section 8f."""
    rp = api.R.NeRFRenderParams(NSamples=64, NImportance=0, Chunk=32768, Perturb=0.0, WhiteBkgr=False, Ndc=False, UseViewdirs=True, ThinRay=True, BoundingBox=api.S.LEGO_BBOX,
                                Precision=api.L.NRF_PREC_F32)
    sc0 = api.S.make_hash_scene(mode="ngp", log2_t=14, seed=5000)
    views = []
    for th in (-120.0, -30.0, 60.0, 150.0, 15.0):          # the last one is held out
        o, d = camera_rays(api, 32, th)
        tgt = sc0["renderer"].Render(0, 0, None, rp, rays=(o, d, None)).Outputs.RGBMap.reshape(-1, 3).clone()
        views.append((o, d, tgt))
    ho, hd, htgt = views.pop()
    out = {}
    for tag, wd, ws in (("regularised", 1.0, 1e-4), ("plain", 0.0, 0.0)):
        sc = api.S.make_hash_scene(mode="ngp", log2_t=14, seed=5000)
        with make_trainer(api, sc, dict(), distortion_loss_weight=wd, sparsity_loss_weight=ws) as tr:
            for it in range(200):
                o, d, tgt = views[it % 4]
                tr.step(o, d, tgt, rp)
            p = copy.copy(rp); p.ReturnRaw, p.KeepIntermediates = True, "depths"
            res = tr.renderer.Render(0, 0, None, p, rays=(ho, hd, None))
            n, s = res.Extras["z_coarse"].shape
            b = dict(raw=host(res.Raw).reshape(n, s, -1), z=host(res.Extras["z_coarse"]), d=host(res.Extras["rays_flat"][:, 3:6]), noise=None, noise_std=0.0)
            _, losses, _, _ = call(api, b, 1.0, 1.0)
            hub = float(torch.nn.functional.huber_loss(res.Outputs.RGBMap.reshape(-1, 3), htgt))
            out[tag] = (float(losses[0]), float(losses[1]), hub)
            print(f"{tag}: weights ({wd}, {ws}); held-out L_dist {losses[0]:.6e}, L_sparse {losses[1]:.6e}, huber {hub:.6e}")
    assert all(np.isfinite(v).all() for v in map(np.array, out.values()))
    assert out["regularised"][0] < out["plain"][0] and out["regularised"][1] < out["plain"][1]
