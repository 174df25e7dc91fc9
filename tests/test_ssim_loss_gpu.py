"""GPU tests of the SSIM training loss (image_metrics.hip: nrf_ssim_loss; rays.hip: nrf_rand_patches; metrics.SSIMLoss, NeRFDataset(patch_size),
Trainer(ssim_loss_weight, patch_size)).  The yardstick is tests/ssim_loss_ref.py (numpy float64 in the operation order the header states, with the library's own
window), pinned by tests/test_ssim_loss_host.py against float64 torch.autograd.

Bars.  d_grad64: equal values (==, so a signed zero does not matter).  d_g_x: equal bits.  d_loss against numpy's sum / n: 1e-12, the bar of the means in
test_metrics_gpu.py.  Every GPU step runs once."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import metrics_ref as MR
import ordered_sum_ref as OS
import ssim_loss_ref as SR

pytestmark = pytest.mark.gpu

P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
host = lambda t: t.detach().cpu().numpy()
dev = lambda a: torch.from_numpy(np.array(a)).cuda()          # (a copy: the shared references are read-only)
bits32 = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
bits64 = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)
EPS = 2.0 ** -52
PATTERN = -12345.678          # what d_loss and d_grad64 hold before a call
NRF_OK, NRF_ERR_INVALID_ARG, NRF_ERR_WORKSPACE = 0, 1, 4
GUARD, FILL = 1 << 20, 0xA5
WEIGHT = 0.2


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from types import SimpleNamespace
    from nerfpp_amd import _lib as L, metrics as M, renderer as R, scene as S, dataset as D, train as T
    win = (C.c_double * 11)()
    L.check(L.lib().nrf_ssim_window(win))
    assert hasattr(L.lib(), "nrf_ssim_loss") and hasattr(L.lib(), "nrf_rand_patches")
    return SimpleNamespace(L=L, M=M, R=R, S=S, D=D, T=T, lib=L.lib(), g=np.array(list(win)))


_REF = {}


def ref_case(api, kind, b, h, w, c):
    """The pair, the restatement's (loss, grad64) with the library's window and the pattern d_g_x holds before a call; computed once per case, never modified."""
    key = (kind, b, h, w, c)
    if key not in _REF:
        x, y = MR.pair(kind, b, h, w, c)
        loss, grad = SR.grad64(x, y, api.g)
        pre = (np.random.default_rng(b + 7 * h + 13 * w + c).standard_normal(x.shape) * 1e-3).astype(np.float32)
        for a in (x, y, loss, grad, pre):
            a.setflags(write=False)
        _REF[key] = (x, y, loss, grad, pre)
    return _REF[key]


def loss_call(api, x, y, weight=WEIGHT, data_range=1.0, pre=None, want64=True, ws_bytes=None, shape=None, null=(), check=True):
    """One nrf_ssim_loss call -> (loss [2], g_x, grad64 | None, status).  d_loss and d_grad64 hold PATTERN before it, d_g_x holds `pre` (zeros if None)."""
    b, h, w, c = x.shape
    dx, dy = dev(x), dev(y)
    loss = torch.full((2,), PATTERN, device="cuda", dtype=torch.float64)
    g64 = torch.full((b, h, w, c), PATTERN, device="cuda", dtype=torch.float64) if want64 else None
    gx = torch.zeros((b, h, w, c), device="cuda") if pre is None else dev(pre)
    tb, th, tw, tc = shape or (b, h, w, c)
    need = int(api.lib.nrf_ssim_loss_workspace_bytes(b, h, w, c))
    nb = need if ws_bytes is None else ws_bytes
    ws = torch.empty((max(need, 8),), dtype=torch.uint8, device="cuda")
    a = dict(x=P(dx), y=P(dy), loss=P(loss), gx=P(gx), ws=P(ws))
    for k in null:
        a[k] = None
    rc = api.lib.nrf_ssim_loss(a["x"], a["y"], tb, th, tw, tc, data_range, weight, a["loss"], a["gx"], P(g64), a["ws"], nb, None)
    torch.cuda.synchronize()
    if check:
        api.L.check(rc)
    return host(loss), host(gx), None if g64 is None else host(g64), rc


# ------------------------------------------------------------------ 1. the kernel against the restatement
@pytest.mark.parametrize("kind", SR.KINDS)
@pytest.mark.parametrize("shape", SR.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_vs_restatement(api, shape, kind):
    """d_grad64 == the restatement value for value; d_loss within 1e-12; d_g_x == pattern + float32(weight * grad64) bit for bit; the same bits without d_grad64
    and in a second run."""
    x, y, rloss, rgrad, pre = ref_case(api, kind, *shape)
    loss, gx, g64, _ = loss_call(api, x, y, pre=pre)
    dev_g, dev_l = np.abs(g64 - rgrad).max(), np.abs(loss - rloss).max()
    print(f"{shape} {kind}: max |grad64 - restatement| = {dev_g:.3e} (max |g| = {np.abs(rgrad).max():.3e}), entries that differ {int((g64 != rgrad).sum())} of {g64.size}; "
          f"loss {loss[0]:.15f}, |loss - numpy| = {dev_l:.3e}")
    assert np.isfinite(g64).all() and (g64 == rgrad).all()
    assert dev_l <= 1e-12 and loss[0] == 1.0 - loss[1]
    want = pre + (WEIGHT * g64).astype(np.float32)
    assert np.array_equal(bits32(gx), bits32(want))
    if kind != "same":
        assert np.abs(rgrad).max() > 0 and not np.array_equal(gx, pre)
    loss_b, gx_b, none, _ = loss_call(api, x, y, pre=pre, want64=False)
    assert none is None and np.array_equal(bits64(loss_b), bits64(loss)) and np.array_equal(bits32(gx_b), bits32(gx)), "the same with and without d_grad64"
    loss_c, gx_c, g64_c, _ = loss_call(api, x, y, pre=pre)
    assert np.array_equal(bits64(loss_c), bits64(loss)) and np.array_equal(bits32(gx_c), bits32(gx)) and np.array_equal(bits64(g64_c), bits64(g64)), "two runs, same bits"


def test_loss_has_the_bits_of_the_ordered_finish_pass(api):
    """One 545 x 513 channel: 18 * 17 = 306 gradient tiles, so the finish pass makes a second strided trip that ends off a multiple of 256.  The workspace
    ([b * c][tiles] doubles at offset 0) is read back: loss[1] == finish(partials) / n_valid and loss[0] == 1 - loss[1], bit for bit."""
    h, w, tiles = 17 * 32 + 1, 16 * 32 + 1, 18 * 17
    x, y = MR.pair("noise", 1, h, w, 1)
    need = int(api.lib.nrf_ssim_loss_workspace_bytes(1, h, w, 1))
    assert need >= tiles * 8
    ws = torch.zeros((need,), dtype=torch.uint8, device="cuda")
    loss = torch.full((2,), PATTERN, device="cuda", dtype=torch.float64)
    gx = torch.zeros((1, h, w, 1), device="cuda")
    dx, dy = dev(x), dev(y)
    api.L.check(api.lib.nrf_ssim_loss(P(dx), P(dy), 1, h, w, 1, 1.0, WEIGHT, P(loss), P(gx), None, P(ws), need, None))
    torch.cuda.synchronize()
    loss, parts = host(loss), host(ws[:tiles * 8].view(torch.float64))
    n_valid = np.float64((h - 10) * (w - 10))
    mean = OS.finish(parts) / n_valid
    print(f"{tiles} tiles: loss {loss[0]!r}, mean {loss[1]!r}; finish(partials) / n {mean!r}, numpy's sum / n {parts.sum() / n_valid!r}")
    assert np.isfinite(parts).all() and (parts != 0.0).sum() > 256 and 0.5 < mean < 1.0          # (the last tile row and column lie outside the valid region: zeros)
    assert bits64(loss[1]) == bits64(mean) and bits64(loss[0]) == bits64(1.0 - mean)


def test_closed_forms(api):
    """flat 0.25 / 0.75: every SSIM value is the forward's closed form; y == x: the loss is an exact 0."""
    x, y, _, _, _ = ref_case(api, "flat", 2, 12, 13, 3)
    loss, _, _, _ = loss_call(api, x, y)
    c1, c2 = 1e-4, 9e-4
    want = ((2 * 0.25 * 0.75 + c1) / (0.25 ** 2 + 0.75 ** 2 + c1)) * (c2 / c2)
    assert abs(loss[1] - want) <= 1e-12
    x, y, _, _, _ = ref_case(api, "same", 4, 16, 16, 3)
    loss, gx, g64, _ = loss_call(api, x, y)
    assert loss[1] == 1.0 and loss[0] == 0.0 and np.abs(g64).max() <= 1e-15


def test_data_range_and_the_python_wrapper(api):
    """metrics.SSIMLoss is the same call; data_range 255 on images scaled by 255 gives the loss of data_range 1 (SSIM is scale covariant: 1e-12) and the gradient / 255."""
    x, y, rloss, rgrad, pre = ref_case(api, "noise", 3, 32, 32, 3)
    loss, gx, g64, _ = loss_call(api, x, y, pre=pre)
    l2, g2, g64_2 = api.M.SSIMLoss(dev(x), dev(y), weight=WEIGHT, grad=dev(pre), return_grad64=True)
    assert np.array_equal(bits64(host(l2)), bits64(loss)) and np.array_equal(bits32(host(g2)), bits32(gx)) and np.array_equal(bits64(host(g64_2)), bits64(g64))
    l3, g3 = api.M.SSIMLoss(dev(x), dev(y))
    assert l3.dtype == torch.float64 and l3.is_cuda and np.array_equal(bits32(host(g3)), bits32(g64.astype(np.float32)))
    x255, y255 = (x * np.float32(255.0)).astype(np.float32), (y * np.float32(255.0)).astype(np.float32)
    ref255 = SR.grad64(x255, y255, api.g, 255.0)
    l4, _, g4, _ = loss_call(api, x255, y255, data_range=255.0)
    assert (g4 == ref255[1]).all() and abs(l4[0] - ref255[0][0]) <= 1e-12


# ------------------------------------------------------------------ 2. an image's gradient does not depend on its batch
@pytest.mark.parametrize("shape", [(4, 16, 16, 3), (2, 43, 42, 3)], ids=["whole", "tiles"])
def test_batch_independence(api, shape):
    """grad64 * n of an image, alone and inside its batch.  n differs by a power of two between b = 1, 2, 4, so the division by n is an exact rescaling and the products
    are equal bit for bit; at b = 3 both the division and the product round once each, relative error 2^-53 each, so the two products differ by at most
    2 * (2 * 2^-53) = 2 * EPS of their value (3 * EPS asked: second-order terms)."""
    b, h, w, c = shape
    x, y, _, rgrad, _ = ref_case(api, "noise", *shape)
    per = (h - 10) * (w - 10) * c
    _, _, full, _ = loss_call(api, x, y)
    assert (full == rgrad).all()
    for sub in (1, 2, 3):
        if sub > b:
            continue
        _, _, part, _ = loss_call(api, x[b - sub:], y[b - sub:])
        a, f = part * float(sub * per), full[b - sub:] * float(b * per)
        if (b // sub) * sub == b and (b // sub) & (b // sub - 1) == 0:
            assert np.array_equal(bits64(a), bits64(f)), sub
        else:
            assert (np.abs(a - f) <= 3 * EPS * np.abs(f)).all(), sub
    assert np.abs(full).max() > 0


# ------------------------------------------------------------------ 3. weight 0, refusals, the workspace
def test_weight_zero_leaves_the_gradient_alone(api):
    x, y, rloss, rgrad, pre = ref_case(api, "noise", 1, 43, 42, 3)
    pre0 = pre.copy(); pre0.reshape(-1)[:4] = (0.0, -0.0, np.float32(1e-40), -np.inf)
    loss, gx, g64, _ = loss_call(api, x, y, weight=0.0, pre=pre0)
    assert np.array_equal(bits32(gx), bits32(pre0)) and np.abs(loss - rloss).max() <= 1e-12 and (g64 == rgrad).all()


def test_refused_arguments(api):
    x, y, rloss, _, pre = ref_case(api, "noise", 2, 12, 13, 3)
    need = int(api.lib.nrf_ssim_loss_workspace_bytes(2, 12, 13, 3))
    assert need >= 2 * 3 * 8
    inval = [dict(null=("x",)), dict(null=("y",)), dict(null=("loss",)), dict(null=("gx",)), dict(null=("ws",)), dict(shape=(0, 12, 13, 3)), dict(shape=(2, 10, 13, 3)),
             dict(shape=(2, 12, 10, 3)), dict(shape=(2, 12, 13, 0)), dict(shape=(2, 12, 13, 5)), dict(shape=(-2, 12, 13, 3)), dict(data_range=0.0), dict(data_range=-1.0),
             dict(data_range=float("nan")), dict(data_range=float("inf")), dict(weight=-1.0), dict(weight=float("nan")), dict(weight=float("inf"))]
    for kw, want_rc in [(k, NRF_ERR_INVALID_ARG) for k in inval] + [(dict(ws_bytes=need - 1), NRF_ERR_WORKSPACE), (dict(ws_bytes=0), NRF_ERR_WORKSPACE)]:
        loss, gx, g64, rc = loss_call(api, x, y, pre=pre, check=False, **kw)
        assert rc == want_rc and b"nrf_ssim_loss" in api.lib.nrf_last_error(), (kw, rc)
        with pytest.raises(api.L.NrfError):
            api.L.check(rc)
        assert (loss == PATTERN).all() and (g64 == PATTERN).all() and np.array_equal(bits32(gx), bits32(pre)), f"a refused call launches nothing: {kw}"
    loss, gx, g64, rc = loss_call(api, x, y, pre=pre)          # a valid call right afterwards
    assert rc == NRF_OK and np.abs(loss - rloss).max() <= 1e-12 and not np.array_equal(gx, pre)
    assert api.lib.nrf_ssim_loss_workspace_bytes(2, 10, 13, 3) == 0


@pytest.mark.parametrize("shape", [(4, 16, 16, 3), (1, 64, 43, 3)], ids=["whole", "tiles"])
def test_workspace_guard(api, shape):
    """test_workspace_gpu.py's scheme: given exactly the B bytes its size function reports (in a buffer of B + 1 MiB of 0xA5) the entry succeeds, leaves the guard alone and
    gives the bits it gives with 4 B; given B - 1 it returns NRF_ERR_WORKSPACE and leaves its outputs as they were."""
    x, y, _, rgrad, pre = ref_case(api, "noise", *shape)
    b, h, w, c = shape
    B = int(api.lib.nrf_ssim_loss_workspace_bytes(b, h, w, c))
    assert B > 0
    dx, dy = dev(x), dev(y)
    make = lambda: dict(loss=torch.full((2,), PATTERN, device="cuda", dtype=torch.float64), gx=dev(pre), g64=torch.full(shape, PATTERN, device="cuda", dtype=torch.float64))
    run = lambda ws, nb, o: api.lib.nrf_ssim_loss(P(dx), P(dy), b, h, w, c, 1.0, WEIGHT, P(o["loss"]), P(o["gx"]), P(o["g64"]), P(ws), nb, None)
    raw = lambda o: {k: host(v).view(np.uint8).copy() for k, v in o.items()}
    ws = torch.full((B + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    outs = make()
    rc = run(ws, B, outs)
    torch.cuda.synchronize()
    assert rc == NRF_OK, api.lib.nrf_last_error()
    assert bool((ws[B:] == FILL).all()), f"the entry wrote past the {B} bytes its size function reports"
    assert (host(outs["g64"]) == rgrad).all()
    big = torch.full((4 * B,), FILL, dtype=torch.uint8, device="cuda")
    ref = make()
    rc = run(big, 4 * B, ref)
    torch.cuda.synchronize()
    assert rc == NRF_OK
    a, r = raw(outs), raw(ref)
    for k in a:
        assert np.array_equal(a[k], r[k]), f"{k} differs between the exact and the 4x workspace"
    untouched = make()
    before = raw(untouched)
    rc = run(ws, B - 1, untouched)
    torch.cuda.synchronize()
    assert rc == NRF_ERR_WORKSPACE
    after = raw(untouched)
    for k in after:
        assert np.array_equal(after[k], before[k]), f"{k} was written by a call that returned NRF_ERR_WORKSPACE"


# ------------------------------------------------------------------ 4. patch-shaped batches
def patches_call(api, seed, it, crop, n_patches, patch, check=True):
    n = max(n_patches * patch * patch, 1)
    rh = torch.full((n,), -77, device="cuda", dtype=torch.int64); rw = torch.full((n,), -77, device="cuda", dtype=torch.int64)
    rc = api.lib.nrf_rand_patches(seed, it, crop[0], crop[1], crop[2], crop[3], n_patches, patch, P(rh), P(rw), None)
    torch.cuda.synchronize()
    if check:
        api.L.check(rc)
    return host(rh), host(rw), rc


@pytest.mark.parametrize("patch", [11, 16])
@pytest.mark.parametrize("n_patches", [1, 5])
def test_rand_patches_equals_the_host_model(api, n_patches, patch):
    """A 20 x 23 crop (rows 3..22, columns 5..27), two iterations: equal to ssim_loss_ref.rand_patches, and every patch inside the crop."""
    crop = (3, 22, 5, 27)
    seen = []
    for it in (0, 7):
        rh, rw, _ = patches_call(api, 0x1234567890ABCDEF, it, crop, n_patches, patch)
        mh, mw = SR.rand_patches(0x1234567890ABCDEF, it, *crop, n_patches, patch)
        assert np.array_equal(rh, mh) and np.array_equal(rw, mw)
        assert rh.min() >= crop[0] and rh.max() <= crop[1] and rw.min() >= crop[2] and rw.max() <= crop[3]
        k = rh.reshape(n_patches, patch, patch)
        assert (k[:, :, 0] - k[:, :1, 0] == np.arange(patch)).all() and (rw.reshape(n_patches, patch, patch)[:, 0, :] - rw.reshape(n_patches, patch, patch)[:, 0, :1] == np.arange(patch)).all()
        seen.append((rh, rw))
    assert not (np.array_equal(seen[0][0], seen[1][0]) and np.array_equal(seen[0][1], seen[1][1])), "another iteration, other patches"


def test_rand_patches_refusals(api):
    for crop, n_patches, patch in (((3, 22, 5, 27), 2, 0), ((3, 22, 5, 27), 2, -3), ((3, 22, 5, 27), 2, 21), ((3, 22, 5, 14), 2, 11), ((3, 22, 5, 27), -1, 11),
                                   ((3, 22, 5, 27), 2, 5000)):
        rh, rw, rc = patches_call(api, 1, 0, crop, n_patches, patch, check=False)
        assert rc == NRF_ERR_INVALID_ARG and b"nrf_rand_patches" in api.lib.nrf_last_error() and (rh == -77).all() and (rw == -77).all(), (crop, n_patches, patch)
    rh, rw, rc = patches_call(api, 1, 0, (3, 22, 5, 27), 2, 20)          # the patch that fills the crop's height: one admissible origin row
    assert rc == NRF_OK and (rh.reshape(2, 20, 20)[:, 0, 0] == 3).all() and rw.min() >= 5 and rw.max() <= 27


def test_dataset_patch_batches(api):
    """NeRFDataset(patch_size=16): BatchSize / 256 patches of the current image; rays, targets and the dict's patch_size.  patch_size=0 (and the argument left out): the
    independent pixels of nrf_rand_pixels, as before."""
    D = api.D
    h, w = 40, 50
    img = np.random.RandomState(1).rand(h, w, 3).astype(np.float32)
    v = D.View(H=h, W=w, K=api.S.lego_K(h, w), Pose=api.S.pose_spherical(30.0, -30.0, 4.0), Image=dev(img), Near=2.0, Far=6.0)
    ds = D.NeRFDataset([v], batch_size=1024, seed=11, patch_size=16)
    ds.SetCurrentIter(5)
    b = ds.get_batch()
    rh, rw = host(b["rand_h"]), host(b["rand_w"])
    mh, mw = SR.rand_patches(11, 5, 0, h - 1, 0, w - 1, 4, 16)
    assert b["patch_size"] == 16 and np.array_equal(rh, mh) and np.array_equal(rw, mw)
    assert np.array_equal(host(b["target_s"]), img[rh, rw]) and b["rays_o"].shape == (1024, 3)
    o, d, _ = D.GetRayBatch(dev(mh), dev(mw), h, w, v.K, v.Pose)
    assert np.array_equal(host(b["rays_d"]), host(d)) and np.array_equal(host(b["rays_o"]), host(o))
    pix = []
    for kw in (dict(), dict(patch_size=0)):
        ds0 = D.NeRFDataset([v], batch_size=500, seed=11, **kw)
        ds0.SetCurrentIter(5)
        b0 = ds0.get_batch()
        assert "patch_size" not in b0
        pix.append((host(b0["rand_h"]), host(b0["rand_w"]), host(b0["target_s"]), host(b0["rays_d"])))
    for a0, a1 in zip(*pix):
        assert np.array_equal(a0, a1)
    want_h = np.array([0 + (SR.rng_u32(11, 16, 5 * 500 + k) * h >> 32) for k in range(500)])
    want_w = np.array([0 + (SR.rng_u32(11, 17, 5 * 500 + k) * w >> 32) for k in range(500)])
    assert np.array_equal(pix[0][0], want_h) and np.array_equal(pix[0][1], want_w)
    ds1 = D.NeRFDataset([v], batch_size=41 * 41 * 1, seed=11, patch_size=41)          # larger than the image's height: refused by the entry
    with pytest.raises(api.L.NrfError):
        ds1.get_batch()


# ------------------------------------------------------------------ 5. the trainer's three paths
def patch_rays(api, theta=30.0):
    """1 024 rays: 4 patches of 16 x 16 of a 64 x 64 camera (NeRFDataset(patch_size=16)), fixed."""
    v = api.D.View(H=64, W=64, K=api.S.lego_K(64, 64), Pose=api.S.pose_spherical(theta, -30.0, 4.0), Near=2.0, Far=6.0)
    ds = api.D.NeRFDataset([v], batch_size=1024, seed=3, patch_size=16)
    b = ds.get_batch()
    return b["rays_o"].contiguous(), b["rays_d"].contiguous(), b


def path_setup(api, path):
    """-> (scene, Trainer keyword arguments, render parameters): the three paths of test_ray_reg_gpu.py::test_trainer_composition"""
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
    """One backward() with the weight on and one with it off on the same render of 4 patches of 16 x 16: g_rgb with the weight on equals the off-run's g_rgb (the Huber
    term) plus the standalone kernel's fp32 result, bit for bit; trainer.ssim_loss holds the standalone call's two words; the rest of the chain sees the new g_rgb (g_raw
    differs) and the f16 path still reads the render's features."""
    sc, kw, rp = path_setup(api, path)
    o, d, _ = patch_rays(api)
    n = o.shape[0]
    tgt = torch.rand((n, 3), generator=torch.Generator().manual_seed(3)).cuda()
    p = copy.copy(rp)
    p.ReturnRaw, p.KeepIntermediates, p.Seed = True, "depths", 1234
    s = p.NSamples + p.NImportance
    with make_trainer(api, sc, kw, ssim_loss_weight=WEIGHT, patch_size=16) as tr:
        res = tr.renderer.Render(0, 0, None, p, rays=(o, d, None))
        tr.backward(res, tgt, s, False, params=p)
        torch.cuda.synchronize()
        on, on_raw, words = host(tr.last["g_rgb"]), host(tr.last["g_raw"]), host(tr.ssim_loss)
        if path == "f16":
            assert tr.reused_render_features is True
        tr.ssim_loss_weight = 0.0
        tr.ssim_loss.fill_(-3.0)
        tr.backward(res, tgt, s, False, params=p)
        torch.cuda.synchronize()
        off, off_raw = host(tr.last["g_rgb"]), host(tr.last["g_raw"])
        assert (host(tr.ssim_loss) == -3.0).all(), "weight 0: no call is issued"
        if path == "f16":
            assert tr.reused_render_features is True
        rgb = host(res.Outputs.RGBMap).reshape(4, 16, 16, 3)
        loss, alone, g64, _ = loss_call(api, rgb, host(tgt).reshape(4, 16, 16, 3))
        assert np.abs(alone).max() > 0 and np.array_equal(bits64(words), bits64(loss)) and 0 < loss[0] < 2
        assert np.array_equal(bits32(on.reshape(-1)), bits32((off.reshape(-1) + alone.reshape(-1)).astype(np.float32)))
        assert not np.array_equal(on, off) and not np.array_equal(on_raw, off_raw)
        with pytest.raises(api.L.NrfError):          # 1 000 rays are no whole number of 16 x 16 patches
            tr.ssim_loss_weight = WEIGHT
            res2 = tr.renderer.Render(0, 0, None, p, rays=(o[:1000].contiguous(), d[:1000].contiguous(), None))
            tr.backward(res2, tgt[:1000].contiguous(), s, False, params=p)


def test_trainer_refuses_bad_arguments(api):
    sc, kw, _ = path_setup(api, "f32")
    for extra in (dict(ssim_loss_weight=-1.0, patch_size=16), dict(ssim_loss_weight=float("nan"), patch_size=16), dict(ssim_loss_weight=float("inf"), patch_size=16),
                  dict(ssim_loss_weight=0.2), dict(ssim_loss_weight=0.2, patch_size=10)):
        with pytest.raises(api.L.NrfError):
            make_trainer(api, sc, kw, **extra)
    make_trainer(api, sc, kw, ssim_loss_weight=0.2, patch_size=11).close()
    make_trainer(api, sc, kw, ssim_loss_weight=0.0, patch_size=4).close()


# ------------------------------------------------------------------ 6. zero weight changes nothing
def test_zero_weight_changes_nothing_f32(api):
    """A Trainer built with ssim_loss_weight=0.0, patch_size=16 against one built without the arguments, fp32 backward: gradients, losses, table and blob after 3 steps,
    bit for bit.  The table gradient goes through the order-free fixed-point scatter (hash_backward packed), as in test_ray_reg_gpu."""
    o, d, _ = patch_rays(api)
    tgt = torch.rand((1024, 3), generator=torch.Generator().manual_seed(4)).cuda()
    _, _, rp = path_setup(api, "f32")
    runs = []
    for extra in ({}, dict(ssim_loss_weight=0.0, patch_size=16)):
        sc = api.S.make_hash_scene(mode="cu", log2_t=14, seed=5000)
        with make_trainer(api, sc, dict(mlp_backward="f32", hash_backward="packed"), **extra) as tr:
            rec = []
            for _ in range(3):
                lm, _ = tr.step(o, d, tgt, rp)
                rec += [host(lm), host(tr.g_blob), host(tr.g_table), host(tr.last["g_raw"]), host(tr.last["g_rgb"])]
            rec += [host(tr.blob), host(tr.table)]
            assert not host(tr.ssim_loss).any()
            runs.append(rec)
    for a, b in zip(*runs):
        assert np.array_equal(bits32(a), bits32(b))
    assert np.abs(runs[0][1]).max() > 0 and np.abs(runs[0][2]).max() > 0


def test_zero_weight_changes_nothing_f16(api):
    """The same on the headline path (CuHash, 64 + 128, mlp_backward="f16", binned scatter, render features reused), 3 steps, by the per-step common-state comparison of
    test_ray_reg_gpu.py::test_zero_weights_change_nothing_f16 and for its reason: the fused fp16 backward adds its workgroups' weight-gradient tiles with float atomics, so
    two runs of the SAME Trainer arguments already differ in the last bits of g_blob (the printed counts show it) and nothing downstream of it can be equal bit for bit
    after 3 steps.  The trainers take every step from the same state (after a step the default-built trainer's parameters and Adam moments are copied to the others); per
    step the losses, g_rgb, g_raw, g_table and the table are equal bit for bit, g_blob is equal to 2e-6 * max (the bar that sum has in
    test_training_backward_reads_the_features_its_forward_render_encoded), and the blob is equal bit for bit in every entry whose g_blob bits are equal."""
    o, d, _ = patch_rays(api)
    tgt = torch.rand((1024, 3), generator=torch.Generator().manual_seed(4)).cuda()
    trs = []
    for extra in ({}, dict(ssim_loss_weight=0.0, patch_size=16), {}):
        sc, kw, rp = path_setup(api, "f16")
        trs.append(make_trainer(api, sc, kw, **extra))
    a, b, a2 = trs
    try:
        for step in range(3):
            rec = []
            for tr in trs:
                lm, _ = tr.step(o, d, tgt, rp)
                assert tr.reused_render_features is True and tr.skipped_steps == 0
                rec.append(dict(lm=host(lm), g_rgb=host(tr.last["g_rgb"]), g_raw=host(tr.last["g_raw"]), g_table=host(tr.g_table), table=host(tr.table),
                                g_blob=host(tr.g_blob), blob=host(tr.blob)))
            ra, rb, ra2 = rec
            print(f"step {step}: g_blob entries with different bits: default vs zero weight {int((bits32(ra['g_blob']) != bits32(rb['g_blob'])).sum())}, "
                  f"default vs default {int((bits32(ra['g_blob']) != bits32(ra2['g_blob'])).sum())} of {ra['g_blob'].size}")
            for k in ("lm", "g_rgb", "g_raw", "g_table", "table"):
                assert np.array_equal(bits32(ra[k]), bits32(rb[k])), (step, k)
            assert np.abs(ra["g_raw"]).max() > 0 and np.abs(ra["g_table"]).max() > 0 and np.abs(ra["g_blob"]).max() > 0
            assert np.abs(ra["g_blob"].astype(np.float64) - rb["g_blob"]).max() <= 2e-6 * np.abs(ra["g_blob"]).max()
            eq = bits32(ra["g_blob"]) == bits32(rb["g_blob"])
            assert eq.any() and np.array_equal(bits32(ra["blob"])[eq], bits32(rb["blob"])[eq])
            assert not host(b.ssim_loss).any()
            for tr in (b, a2):
                for name in ("blob", "table", "m_blob", "v_blob", "m_table", "v_table"):
                    getattr(tr, name).copy_(getattr(a, name))
                tr._push_params()
                assert tr.t == a.t and tr.lr == a.lr
    finally:
        for tr in trs:
            tr.close()


# ------------------------------------------------------------------ 7. it trains
def test_it_trains(api):
    """One fixed batch of 4 x 16 x 16 patches of a 64 x 64 view of the teacher (the ngp synthetic scene's render of its own initial parameters, seed 5000); a student from
    other initial parameters (seed 6000) takes 100 steps on it with huber + 0.2 * (1 - SSIM).  trainer.ssim_loss[0] at the last step is below the first step's (strict; the
    direction only).  Values seen on the MI355X: DESIGN.md section 8i."""
    rp = api.R.NeRFRenderParams(NSamples=64, NImportance=0, Chunk=32768, Perturb=0.0, WhiteBkgr=False, Ndc=False, UseViewdirs=True, ThinRay=True, BoundingBox=api.S.LEGO_BBOX,
                                Precision=api.L.NRF_PREC_F32)
    teacher = api.S.make_hash_scene(mode="ngp", log2_t=14, seed=5000)
    o, d, _ = patch_rays(api)
    tgt = teacher["renderer"].Render(0, 0, None, rp, rays=(o, d, None)).Outputs.RGBMap.reshape(-1, 3).clone()
    sc = api.S.make_hash_scene(mode="ngp", log2_t=14, seed=6000)
    seen = []
    with make_trainer(api, sc, dict(), ssim_loss_weight=0.2, patch_size=16) as tr:
        for it in range(100):
            lm, _ = tr.step(o, d, tgt, rp)
            if it in (0, 99):
                seen.append((host(tr.ssim_loss).copy(), host(lm).copy()))
    (s0, l0), (s1, l1) = seen
    print(f"step 0: 1 - SSIM {s0[0]:.6f}, huber {l0[0]:.6e}; step 99: 1 - SSIM {s1[0]:.6f}, huber {l1[0]:.6e}")
    assert np.isfinite(s0).all() and np.isfinite(s1).all() and 0 < s0[0] and s1[0] < s0[0]
