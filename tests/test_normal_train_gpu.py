"""GPU tests of training the predicted-normals head (normal_loss.hip, nrf_mlp_backward_pn, Trainer(pred_normal_loss_weight, orientation_loss_weight)).  The yardstick is
tests/normal_loss_ref.py (float64 torch, autograd on the CPU), pinned by tests/test_normal_train_host.py."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import ordered_sum_ref as OS
from conftest import load_golden
from nerfpp_amd import synth
from normal_loss_ref import SmallPNRef, normal_losses, t64

pytestmark = pytest.mark.gpu

P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
host = lambda t: t.detach().cpu().numpy()
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from types import SimpleNamespace
    from nerfpp_amd import _lib as L, mesh, modules as M, renderer as R, scene as S, train as T
    assert hasattr(L.lib(), "nrf_normal_losses") and hasattr(L.lib(), "nrf_mlp_backward_pn")
    return SimpleNamespace(L=L, mesh=mesh, M=M, R=R, S=S, T=T)


def close(got, ref, rtol, atol, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref) - (atol + rtol * np.abs(ref))
    print(f"{what}: max |got - ref| = {np.abs(got - ref).max():.3e}, max |ref| = {np.abs(ref).max():.3e}, worst excess over the bar = {err.max():.3e}")
    assert np.isfinite(got).all() and (err <= 0).all(), what


def pn_scene(api, mode="ngp", log2_t=14):
    """make_hash_scene extended by a normals net, as test_mlp_small_with_the_predicted_normals_head does."""
    sc = api.S.make_hash_scene(mode=mode, log2_t=log2_t, seed=5000)
    d = api.L.MlpSmallDesc(32, 16, 3, 64, 15, 4, 64, 1, 3, 64)
    n_pn = int(api.L.lib().nrf_mlp_small_param_count(C.byref(d)))
    blob = np.concatenate([sc["mlp_blob"], synth.synth_sym(91, (n_pn - sc["mlp_blob"].size,), np.float32(0.1))]).astype(np.float32)
    m = api.M.NeRFSmall(3, 64, 15, 4, 64, True, 3, 64, 32, 16, "model", params=blob)
    return sc, m, blob


def step_params(api, **kw):
    a = dict(NSamples=64, NImportance=0, Chunk=32768, Perturb=0.0, WhiteBkgr=False, Ndc=False, UseViewdirs=True, ThinRay=True, BoundingBox=api.S.LEGO_BBOX,
             Precision=api.L.NRF_PREC_F32)
    a.update(kw)
    return api.R.NeRFRenderParams(**a)


def camera_rays(api, h, theta=30.0):
    K = api.S.lego_K(h, h)
    o, d, _ = api.R.GetRays(h, h, K, api.S.pose_spherical(theta, -30.0, 4.0))
    return o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()


def render_and_backward(api, tr, o, d, tgt, rp):
    """Trainer.step's render and backward without the optimizer step (the handle keeps the parameters the gradients belong to)."""
    p = copy.copy(rp)
    p.ReturnRaw, p.KeepIntermediates, p.ReturnWeights = True, "depths", True
    res = tr.renderer.Render(0, 0, None, p, rays=(o, d, None))
    lm = tr.backward(res, tgt, p.NSamples + p.NImportance, p.WhiteBkgr, params=p)
    torch.cuda.synchronize()
    return res, lm


def mlp_backward(api, fn, wsfn, m, x, g_out, n_params, in_ch=32):
    lib = api.L.lib()
    p = x.shape[0]
    nb = int(wsfn(m._m, C.c_int64(p)))
    ws = torch.empty((nb,), dtype=torch.uint8, device="cuda")
    g_blob = torch.zeros((n_params,), device="cuda"); g_x = torch.full((p, in_ch), 7.0, device="cuda")
    api.L.check(fn(m._m, P(x), P(g_out), C.c_int64(p), P(g_blob), P(g_x), P(ws), C.c_size_t(nb), None))
    torch.cuda.synchronize()
    return host(g_blob), host(g_x)


# ------------------------------------------------------------------ 1. the fused loss kernel
def test_normal_losses_vs_restatement(api):
    """nrf_normal_losses on random inputs (n = 257, s = 64, some w == 0, some |g| = 0): losses and d / d raw[..., 4:7] against autograd of the restatement.  About ten
    fp32 operations per element (6e-8 each) with fp64 sums, and pred - nrm may cancel: elementwise rtol 1e-5 with atol 1e-6 * max|ref|, losses rtol 1e-5.  Columns 0:4
    keep their sentinel; two runs give the same bits."""
    n, s, wpn, wor = 257, 64, 0.7, 0.3
    rng = np.random.default_rng(11)
    w = rng.uniform(0, 1, (n, s)).astype(np.float32); w[rng.uniform(size=(n, s)) < 0.2] = 0
    g = rng.standard_normal((n, s, 3)).astype(np.float32) * np.float32(10.0) ** rng.integers(-3, 3, (n, s, 1)).astype(np.float32)
    g[rng.uniform(size=(n, s)) < 0.05] = 0
    raw = rng.standard_normal((n, s, 7)).astype(np.float32)
    raw[0, 0, 4:] = np.inf; w[0, 0] = 0; g[0, 1] = np.nan; w[0, 1] = 0          # a zero-weight sample contributes 0 whatever it holds
    rays = rng.standard_normal((n, 11)).astype(np.float32)
    lib = api.L.lib()
    d_w, d_g, d_raw, d_rays = dev(w), dev(g), dev(raw), dev(rays)
    nb = int(lib.nrf_normal_losses_workspace_bytes(C.c_int64(n), s))
    ws = torch.empty((nb,), dtype=torch.uint8, device="cuda")
    outs = []
    for _ in range(2):
        g_raw = torch.full((n, s, 7), -123.5, device="cuda"); losses = torch.empty((2,), device="cuda")
        api.L.check(lib.nrf_normal_losses(P(d_w), P(d_g), P(d_raw), 7, C.c_void_p(d_rays.data_ptr() + 12), 11, C.c_int64(n), s, C.c_float(wpn), C.c_float(wor), P(g_raw),
                                          P(losses), P(ws), C.c_size_t(nb), None))
        torch.cuda.synchronize()
        outs.append((host(g_raw), host(losses)))
    assert np.array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32)) and np.array_equal(outs[0][1].view(np.uint32), outs[1][1].view(np.uint32))
    g_raw, losses = outs[0]
    assert (g_raw[..., :4] == -123.5).all()
    live = w != 0
    rawc = raw.copy(); rawc[~live] = 0; gc = g.copy(); gc[~live] = 0
    pred = t64(rawc[..., 4:7], grad=True)
    l_pn, l_or = normal_losses(t64(w), t64(gc), pred, t64(rays[:, 3:6]))
    (wpn * l_pn + wor * l_or).backward()
    ref = pred.grad.numpy()
    assert (g_raw[..., 4:][~live] == 0).all() and np.isfinite(g_raw[..., 4:]).all()
    close(g_raw[..., 4:], ref, 1e-5, 1e-6 * np.abs(ref).max(), "d / d raw[..., 4:7]")
    close(losses[0], float(l_pn.detach()), 1e-5, 0, "PredNormalLoss")
    close(losses[1], float(l_or.detach()), 1e-5, 0, "OrientationLoss")
    d_out, d_l = torch.zeros((n, s, 4), device="cuda"), torch.zeros((2,), device="cuda")
    with pytest.raises(api.L.NrfError):          # a 4-column network has no predicted normals
        api.L.check(lib.nrf_normal_losses(P(d_w), P(d_g), P(d_raw), 4, C.c_void_p(d_rays.data_ptr() + 12), 11, C.c_int64(n), s, C.c_float(wpn), C.c_float(wor), P(d_out),
                                          P(d_l), P(ws), C.c_size_t(nb), None))


@pytest.mark.parametrize("n", [1025, 4], ids=["257_blocks", "one_block"])
def test_normal_losses_have_the_bits_of_the_ordered_finish_pass(api, n):
    """s = 64: 256 samples per block, so n = 1025 leaves 257 partial pairs (a second strided trip of the finish pass, one entry long) and n = 4 one.  The workspace
    ([blocks][2] doubles at offset 0) is read back: losses == float32(finish(column) / count), bit for bit."""
    s = 64
    blocks = -(-n * s // 256)
    assert blocks == (257 if n == 1025 else 1)
    rng = np.random.default_rng(12)
    w = rng.uniform(0, 1, (n, s)).astype(np.float32)
    g = rng.standard_normal((n, s, 3)).astype(np.float32)
    raw = rng.standard_normal((n, s, 7)).astype(np.float32)
    rays = rng.standard_normal((n, 11)).astype(np.float32)
    lib = api.L.lib()
    d_w, d_g, d_raw, d_rays = dev(w), dev(g), dev(raw), dev(rays)
    nb = int(lib.nrf_normal_losses_workspace_bytes(C.c_int64(n), s))
    assert nb >= blocks * 2 * 8
    ws = torch.zeros((nb,), dtype=torch.uint8, device="cuda")
    g_raw, losses = torch.zeros((n, s, 7), device="cuda"), torch.empty((2,), device="cuda")
    api.L.check(lib.nrf_normal_losses(P(d_w), P(d_g), P(d_raw), 7, C.c_void_p(d_rays.data_ptr() + 12), 11, C.c_int64(n), s, C.c_float(0.7), C.c_float(0.3), P(g_raw),
                                      P(losses), P(ws), C.c_size_t(nb), None))
    torch.cuda.synchronize()
    losses, parts = host(losses), host(ws[:blocks * 2 * 8].view(torch.float64)).reshape(blocks, 2)
    want = np.array([np.float32(OS.finish(parts[:, 0]) / (np.float64(n * s) * 3.0)), np.float32(OS.finish(parts[:, 1]) / np.float64(n))])
    print(f"n = {n}: losses {losses}, float32(finish(partials) / count) {want}, numpy's sums {parts.sum(0)}")
    assert np.isfinite(parts).all() and (parts > 0.0).all()
    assert np.array_equal(losses.view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------ 2. the 7-column network backward
def test_mlp_backward_pn_vs_restatement_autograd(api, manifest):
    """nrf_mlp_backward_pn on the mlp_small_pn weights, 4 096 random rows, random 7-column g_out, against autograd of the restatement -- the bars of
    test_training_backward_stages_vs_reference_autograd (weight gradients rtol 1e-3, atol 2e-5 * max|ref|; g_x rtol 1e-4, atol 1e-6 * max|ref|).  With g_out[:, 4:7] = 0 the
    head's gradient is exactly 0 and the rest equals nrf_mlp_backward bit for bit."""
    blob = synth.blob_from_manifest(manifest["mlp_small_pn"])
    m = api.M.NeRFSmall(3, 64, 15, 3, 64, True, 3, 64, 32, 16, "model", params=blob)
    rng = np.random.default_rng(21)
    x = rng.uniform(-1, 1, (4096, 48)).astype(np.float32)
    go = rng.standard_normal((4096, 7)).astype(np.float32)
    lib = api.L.lib()
    gb, gx = mlp_backward(api, lib.nrf_mlp_backward_pn, lib.nrf_mlp_backward_pn_workspace_bytes, m, dev(x), dev(go), blob.size)
    ref = SmallPNRef(blob, n_layers_c=3)
    x64 = t64(x, grad=True)
    out, kink = ref.forward(x64)
    (out * t64(go)).sum().backward()
    print("rows with a hidden pre-activation within 1e-5 of zero:", int((kink.numpy() < 1e-5).sum()), "of 4096 (none left out)")
    rb, rx = ref.grad_blob(), x64.grad.numpy()[:, :32]
    for k, (off, cnt) in enumerate(ref.where):
        r = rb[off:off + cnt]
        close(gb[off:off + cnt], r, 1e-3, 2e-5 * np.abs(r).max(), f"weight gradient of matrix {k}")
    assert np.abs(rb[ref.head_offset:]).max() > 0
    close(gx, rx, 1e-4, 1e-6 * np.abs(rx).max(), "g_x")
    go0 = go.copy(); go0[:, 4:] = 0
    gb0, gx0 = mlp_backward(api, lib.nrf_mlp_backward_pn, lib.nrf_mlp_backward_pn_workspace_bytes, m, dev(x), dev(go0), blob.size)
    gb1, gx1 = mlp_backward(api, lib.nrf_mlp_backward, lib.nrf_mlp_backward_workspace_bytes, m, dev(x), dev(go0), blob.size)
    assert (gb0[ref.head_offset:] == 0).all() and (gb1[ref.head_offset:] == 0).all()
    assert np.array_equal(gb0[:ref.head_offset], gb1[:ref.head_offset]) and np.array_equal(gx0, gx1)
    m4 = api.M.NeRFSmall(3, 64, 15, 3, 64, False, 3, 64, 32, 16, "model", params=blob[:ref.head_offset])
    with pytest.raises(api.L.NrfError):
        mlp_backward(api, lib.nrf_mlp_backward_pn, lib.nrf_mlp_backward_workspace_bytes, m4, dev(x), dev(go), ref.head_offset)


# ------------------------------------------------------------------ 3. the whole step
def test_whole_step_gradients_vs_restatement(api):
    """Trainer.backward with both weights non-zero on the 7-column ngp scene, the 256 rays of a 16 x 16 camera x 64 samples (most samples inside the box, some rays leave it:
    the column -1 mask): g_blob and g_table against the restatement chained with the library's own pinned stages -- w, raw and the density gradient from the render and
    nrf_density_grad, d loss / d raw[..., :4] from nrf_raw2outputs_backward, the table gradient through nrf_hash_backward_rays.  Bars of test 2."""
    wpn, wor = 1.0, 0.5
    sc, m, blob = pn_scene(api)
    o, d = camera_rays(api, 16)
    tgt = torch.rand((256, 3), generator=torch.Generator().manual_seed(3)).cuda()
    rp = step_params(api)
    with api.T.Trainer(sc["embedder"], sc["embeddirs"], m, sc["table"], blob, pred_normal_loss_weight=wpn, orientation_loss_weight=wor) as tr:
        res, lm = render_and_backward(api, tr, o, d, tgt, rp)
        n, s = 256, 64
        pts, x, g_raw = tr.last["pts"], tr.last["x"], host(tr.last["g_raw"])
        _, keep = tr.embedder.forward(pts)
        keep = host(keep).astype(bool)
        assert 0 < (~keep).sum() < 0.5 * keep.size, (~keep).sum()          # a few rays leave the box
        _, g = api.mesh.DensityGradient(tr.renderer, pts)
        w, raw, rays = host(res.Outputs.Weights).reshape(n, s), host(res.Raw), host(res.Extras["rays_flat"])
        assert (raw[..., 6].reshape(-1)[~keep] == 0).all() and (g_raw[..., 6].reshape(-1)[~keep] == 0).all() and np.abs(g_raw[..., 3].reshape(-1)[~keep]).max() > 0
        ref = SmallPNRef(blob)
        x64 = t64(host(x), grad=True)
        out, kink = ref.forward(x64)
        print("rows with a hidden pre-activation within 1e-5 of zero:", int((kink.numpy() < 1e-5).sum()), "of", n * s, "(none left out)")
        ro = out.detach().numpy()[:, :6]          # (three 64-term fp32 chains: 3 * 64 * 6e-8 of the largest value)
        close(host(res.Raw).reshape(-1, 7)[:, :6], ro, 1e-4, 2e-5 * np.abs(ro).max(), "the render's raw vs the restatement's forward")
        kz = torch.from_numpy(keep)
        pred = torch.cat([out[:, 4:6], torch.where(kz, out[:, 6], torch.zeros_like(out[:, 6]))[:, None]], 1).reshape(n, s, 3)      # the forward's column -1 mask
        l_pn, l_or = normal_losses(t64(w), t64(host(g)).reshape(n, s, 3), pred, t64(rays[:, 3:6]))
        close(host(tr.normal_losses), [float(l_pn.detach()), float(l_or.detach())], 1e-4, 0, "trainer.normal_losses")
        assert float(l_pn.detach()) > 0 and float(l_or.detach()) > 0
        (wpn * l_pn + wor * l_or + (out[:, :4] * t64(g_raw.reshape(-1, 7)[:, :4])).sum()).backward()
        rb, rx = ref.grad_blob(), x64.grad.numpy()[:, :32]
        gb = host(tr.g_blob)
        for k, (off, cnt) in enumerate(ref.where):
            r = rb[off:off + cnt]
            close(gb[off:off + cnt], r, 1e-3, 2e-5 * np.abs(r).max(), f"weight gradient of matrix {k}")
        assert np.abs(rb[ref.head_offset:]).max() > 0
        close(host(tr.last["g_x"]), rx, 1e-4, 1e-6 * np.abs(rx).max(), "g_x")
        g_table = torch.zeros_like(tr.g_table)
        api.L.check(api.L.lib().nrf_hash_backward_rays(tr.embedder._h, P(pts), C.c_int64(n), s, P(dev(rx)), P(g_table), None))
        torch.cuda.synchronize()
        rt = host(g_table)
        close(host(tr.g_table), rt, 1e-3, 2e-5 * np.abs(rt).max(), "g_table")


# ------------------------------------------------------------------ 4. no change where nothing was asked
def test_zero_weights_change_nothing(api):
    """4-column scene: g_blob, g_table, the losses and the parameters after 3 steps are bit-identical between a Trainer built with the old arguments and one that passes both
    new weights as 0.0 (table gradient through the order-free fixed-point scatter).  7-column scene, both weights 0: the head's gradient is exactly 0, its parameters do
    not move in 3 steps, and the other two nets' gradients equal nrf_mlp_backward on the same x and g_out bit for bit."""
    o, d = camera_rays(api, 32)
    tgt = torch.rand((1024, 3), generator=torch.Generator().manual_seed(4)).cuda()
    rp = step_params(api)
    runs = []
    for extra in ({}, dict(pred_normal_loss_weight=0.0, orientation_loss_weight=0.0)):
        sc = api.S.make_hash_scene(mode="cu", log2_t=14, seed=5000)
        with api.T.Trainer(sc["embedder"], sc["embeddirs"], sc["mlp"], sc["table"], sc["mlp_blob"], learning_rate=1e-3, hash_backward="packed", **extra) as tr:
            rec = []
            for _ in range(3):
                lm, _ = tr.step(o, d, tgt, rp)
                rec += [host(lm), host(tr.g_blob), host(tr.g_table)]
            rec += [host(tr.blob), host(tr.table), host(tr.normal_losses)]
            runs.append(rec)
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert (runs[1][-1] == 0).all() and np.abs(runs[0][1]).max() > 0 and np.abs(runs[0][2]).max() > 0
    sc, m, blob = pn_scene(api, mode="cu")
    ref_head = SmallPNRef(blob).head_offset
    with api.T.Trainer(sc["embedder"], sc["embeddirs"], m, sc["table"], blob, learning_rate=1e-3, hash_backward="packed") as tr:
        res, _ = render_and_backward(api, tr, o, d, tgt, rp)
        gb = host(tr.g_blob)
        assert res.Raw.shape[-1] == 7 and (gb[ref_head:] == 0).all() and np.abs(gb[:ref_head]).max() > 0
        lib = api.L.lib()
        gb1, gx1 = mlp_backward(api, lib.nrf_mlp_backward, lib.nrf_mlp_backward_workspace_bytes, m, tr.last["x"], tr.last["g_raw"].reshape(-1, 7), blob.size)
        assert np.array_equal(gb, gb1) and np.array_equal(host(tr.last["g_x"]), gx1)
        for _ in range(3):
            tr.step(o, d, tgt, rp)
            assert (host(tr.g_blob)[ref_head:] == 0).all()
        after = host(tr.blob)
        assert np.array_equal(after[ref_head:], blob[ref_head:]) and not np.array_equal(after[:ref_head], blob[:ref_head])


# ------------------------------------------------------------------ 5. it learns
def _normal_agreement(api, tr, o, d, rp):
    """Mean cosine between normalize(pred) and the density normal over the samples with w > 1e-3 of one view."""
    p = copy.copy(rp); p.ReturnRaw, p.ReturnWeights, p.KeepIntermediates = True, True, "depths"
    res = tr.renderer.Render(0, 0, None, p, rays=(o, d, None))
    n, s = res.Outputs.Weights.shape
    rays, z = res.Extras["rays_flat"], res.Extras["z_coarse"]
    pts = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]).reshape(-1, 3).contiguous()
    _, g = api.mesh.DensityGradient(tr.renderer, pts)
    nrm = -g / g.norm(dim=1, keepdim=True).clamp_min(1e-8)
    pred = res.Raw.reshape(-1, 7)[:, 4:7]
    pred = pred / pred.norm(dim=1, keepdim=True).clamp_min(1e-8)
    sel = res.Outputs.Weights.reshape(-1) > 1e-3
    assert int(sel.sum()) > 100
    return float((pred * nrm).sum(1)[sel].mean())


def test_head_learns_the_density_normals(api, tmp_path):
    """7-column scene, targets = the scene's own render of its initial parameters, pred_normal_loss_weight = 1, 200 steps of 1 024 rays: the mean of L_pn over the last 10
    steps is below the mean over the first 10 and the predicted normals agree better with the density normals after than before (strict inequalities; the values are
    printed).  Adam, the gradient hook and the checkpoint cover the head's parameters; a trained head renders the same RenderedPredNormals bits after Save / Load."""
    sc, m, blob = pn_scene(api)
    rp = step_params(api)
    views = []
    for th in (-120.0, -30.0, 60.0, 150.0):
        o, d = camera_rays(api, 32, th)
        tgt = api.R.NeRFRenderer(sc["embedder"], sc["embeddirs"], m).Render(0, 0, None, rp, rays=(o, d, None)).Outputs.RGBMap.reshape(-1, 3).clone()
        views.append((o, d, tgt))
    head = SmallPNRef(blob).head_offset
    seen = []
    hook = lambda g_table, g_blob: seen.append((g_blob.numel(), float(g_blob[head:].abs().max())))
    with api.T.Trainer(sc["embedder"], sc["embeddirs"], m, sc["table"], blob, learning_rate=1e-3, pred_normal_loss_weight=1.0, grad_sync=hook) as tr:
        before = _normal_agreement(api, tr, views[0][0], views[0][1], rp)
        l_pn = []
        for it in range(200):
            o, d, tgt = views[it % 4]
            tr.step(o, d, tgt, rp, global_step=it, n_iters=400, lrate_decay=250)
            l_pn.append(tr.normal_losses.clone())
        l_pn = host(torch.stack(l_pn))[:, 0]
        after = _normal_agreement(api, tr, views[0][0], views[0][1], rp)
        first, last = float(l_pn[:10].mean()), float(l_pn[-10:].mean())
        print(f"L_pn first 10 steps {first:.6e}, last 10 steps {last:.6e}; mean cosine(pred, density normal) before {before:.4f}, after {after:.4f}")
        assert np.isfinite(l_pn).all() and last < first and after > before
        # the optimizer, the gradient hook and the schedule see the head: its parameters and Adam moments moved, the hook got the whole blob with a non-zero head slice
        assert len(seen) == 200 and seen[0][0] == blob.size and seen[0][1] > 0 and tr.lr < tr.learning_rate0
        assert not np.array_equal(host(tr.blob)[head:], blob[head:]) and float(tr.m_blob[head:].abs().max()) > 0 and float(tr.v_blob[head:].abs().max()) > 0
        pp = step_params(api, UsePredNormal=True)
        img = host(tr.renderer.Render(0, 0, None, pp, rays=(views[1][0], views[1][1], None)).Outputs.RenderedPredNormals)
        ck = str(tmp_path / "ck")
        tr.SaveCheckpoint(ck, global_step=200)
        trained = host(tr.blob)
    sc2, m2, blob2 = pn_scene(api)
    with api.T.Trainer(sc2["embedder"], sc2["embeddirs"], m2, sc2["table"], blob2, pred_normal_loss_weight=1.0) as tr2:
        assert tr2.LoadCheckpoint(ck) == 200
        assert np.array_equal(host(tr2.blob), trained) and float(tr2.m_blob[head:].abs().max()) > 0
        img2 = host(tr2.renderer.Render(0, 0, None, pp, rays=(views[1][0], views[1][1], None)).Outputs.RenderedPredNormals)
    assert np.abs(img).max() > 0 and np.array_equal(img.view(np.uint32), img2.view(np.uint32))


# ------------------------------------------------------------------ 6. refusals
def test_unsupported_requests_are_refused(api):
    sc, m, blob = pn_scene(api, mode="cu")
    E = api.L.NrfError
    with pytest.raises(E):
        api.T.Trainer(sc["embedder"], sc["embeddirs"], m, sc["table"], blob, mlp_backward="f16", pred_normal_loss_weight=1.0)
    with pytest.raises(E):
        api.T.Trainer(sc["embedder"], sc["embeddirs"], sc["mlp"], sc["table"], sc["mlp_blob"], orientation_loss_weight=1.0)          # a 4-column network
    cl = api.S.make_classic_scene()
    with pytest.raises(E):
        api.T.Trainer(cl["embedder"], cl["embeddirs"], cl["mlp"], None, cl["mlp_blob"], pred_normal_loss_weight=1.0)
    o, d = camera_rays(api, 8)
    tgt = torch.zeros((64, 3), device="cuda")
    with api.T.Trainer(sc["embedder"], sc["embeddirs"], m, sc["table"], blob, pred_normal_loss_weight=1.0) as tr:
        with pytest.raises(E):
            tr.step(o, d, tgt, step_params(api, NImportance=64))
        with pytest.raises(E):
            tr.step(o, d, tgt, step_params(api, Precision=api.L.NRF_PREC_F16_SPLIT))
        assert tr.t == 0 and float(tr.g_blob.abs().max()) == 0
        tr.step(o, d, tgt, step_params(api))
        assert tr.t == 1 and float(tr.g_blob.abs().max()) > 0
