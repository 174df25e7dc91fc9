"""CPU tests of the SSIM training loss (nrf_ssim_loss, nrf_rand_patches, metrics.SSIMLoss, NeRFDataset(patch_size), Trainer(ssim_loss_weight, patch_size)): the
float64 yardstick of the GPU tests (tests/ssim_loss_ref.py) is pinned against float64 torch.autograd of the textbook formula, and the host pieces of the library --
the declarations, the refusals that need no device -- are checked."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import metrics_ref as MR
import ssim_loss_ref as SR

# The bar of the restatement against autograd, relative to the largest gradient entry of the case.  Measured with this file over SHAPES x (noise, indep, flat): the
# worst max|dev| / max|g_autograd| is 6.7e-13 (flat 0.25 / 0.75 at [1, 43, 42, 3]; noise <= 4.2e-14, indep <= 2.6e-15) -- below 2e-12, so the bar is 1e-11.  The margin is
# there because autograd's conv2d adds the 121 taps of the outer-product window in another order than the two separable passes.
REL_BAR = 1e-11
SAME_ABS_BAR = 1e-15          # y == x: autograd's gradient is not an exact 0 (entries up to 2.6e-16 remain from its cancelling terms; the restatement gave 0 at every shape)


def autograd(x, y, data_range=1.0):
    """The textbook formula with conv2d and the outer-product window, float64 -> (mean SSIM over every valid value, d (1 - mean) / dx)."""
    g = torch.from_numpy(MR.window())
    xt = torch.from_numpy(np.asarray(x, np.float64)).permute(0, 3, 1, 2).clone().requires_grad_(True)
    yt = torch.from_numpy(np.asarray(y, np.float64)).permute(0, 3, 1, 2)
    c = xt.shape[1]
    k = torch.outer(g, g)[None, None].repeat(c, 1, 1, 1)
    f = lambda a: torch.nn.functional.conv2d(a, k, groups=c)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mx, my = f(xt), f(yt)
    vx, vy, cxy = f(xt * xt) - mx * mx, f(yt * yt) - my * my, f(xt * yt) - mx * my
    ssim = ((2 * mx * my + c1) * (2 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    mean = ssim.mean()
    (1.0 - mean).backward()
    return float(mean.detach()), xt.grad.permute(0, 2, 3, 1).numpy()


@pytest.fixture(scope="module")
def cases():
    out = {}
    for shape in SR.SHAPES:
        for kind in SR.KINDS:
            x, y = MR.pair(kind, *shape)
            out[shape, kind] = (x, y, SR.grad64(x, y, MR.window()), autograd(x, y))
    return out


def test_restatement_equals_autograd(cases):
    worst = {}
    for (shape, kind), (x, y, (loss, grad), (mean, ag)) in cases.items():
        dev, top = np.abs(grad - ag).max(), np.abs(ag).max()
        assert grad.shape == x.shape and np.isfinite(grad).all()
        if kind == "same":
            print(f"{shape} same: max |restatement| = {np.abs(grad).max():.3e}, max |autograd| = {top:.3e}")
            assert np.abs(grad).max() <= SAME_ABS_BAR and top <= SAME_ABS_BAR
            continue
        rel = dev / top
        worst[kind] = max(worst.get(kind, 0.0), rel)
        print(f"{shape} {kind}: max |dev| = {dev:.3e}, max |g_autograd| = {top:.3e}, ratio {rel:.3e}")
        assert top > 0 and rel <= REL_BAR, (shape, kind, rel)
    print("worst max|dev| / max|g_autograd| per pair kind:", {k: f"{v:.2e}" for k, v in worst.items()})


def test_loss_value(cases):
    """{1 - mean, mean}: against metrics_ref.means_of (per image channel; equal valid counts, so the mean over all values is the mean of those means) at the 1e-12 of
    test_metrics_gpu.py, and against autograd's forward."""
    for (shape, kind), (x, y, (loss, grad), (mean, ag)) in cases.items():
        m = MR.means_of(*MR.ssim_maps(x, y, MR.window()))[..., 0].mean()
        assert abs(loss[1] - m) <= 1e-12 and abs(loss[0] - (1.0 - m)) <= 1e-12 and abs(loss[1] - mean) <= 1e-12, (shape, kind)
        if kind == "same":
            assert loss[1] == 1.0 and loss[0] == 0.0


def test_transposed_window_is_the_adjoint_of_the_valid_filter():
    """<filt(a), m> == <a, filt_t(m)> for both axes, to rounding."""
    rng = np.random.default_rng(11)
    g = MR.window()
    a, m = rng.standard_normal((2, 23, 17, 3)), rng.standard_normal((2, 13, 7, 3))
    lhs = (MR.filt(MR.filt(a, g, 2), g, 1) * m).sum()
    t = SR.filt_t(SR.filt_t(m, g, 1), g, 2)
    assert t.shape == a.shape and abs(lhs - (a * t).sum()) <= 1e-12 * max(1.0, abs(lhs))


def test_new_entries_are_declared_and_exported():
    from nerfpp_amd import _lib as L, metrics
    from nerfpp_amd.dataset import NeRFDataset
    from nerfpp_amd.train import Trainer
    for name in ("nrf_ssim_loss", "nrf_ssim_loss_workspace_bytes", "nrf_rand_patches"):
        assert name in L.SYMBOLS
        assert hasattr(C.CDLL(L.LIB_PATH), name), name
    assert L.SYMBOLS.index("nrf_rand_patches") == L.SYMBOLS.index("nrf_rand_pixels") + 1
    assert L.SYMBOLS.index("nrf_ssim_loss_workspace_bytes") == L.SYMBOLS.index("nrf_ms_ssim") + 1
    sig = inspect.signature(metrics.SSIMLoss).parameters
    assert list(sig) == ["x", "y", "data_range", "weight", "grad", "return_grad64"]
    assert (sig["data_range"].default, sig["weight"].default, sig["grad"].default, sig["return_grad64"].default) == (1.0, 1.0, None, False)
    sig = inspect.signature(Trainer.__init__).parameters
    assert sig["ssim_loss_weight"].default == 0.0 and isinstance(sig["ssim_loss_weight"].default, float) and sig["patch_size"].default == 0
    assert inspect.signature(NeRFDataset.__init__).parameters["patch_size"].default == 0


def test_refusals_that_need_no_device():
    from nerfpp_amd import _lib
    lib = _lib.lib()
    assert lib.nrf_ssim_loss(None, None, 1, 11, 11, 1, 1.0, 1.0, None, None, None, None, 0, None) == 1 and b"nrf_ssim_loss" in lib.nrf_last_error()
    assert lib.nrf_ssim_loss_workspace_bytes(1, 11, 11, 1) > 0 and lib.nrf_ssim_loss_workspace_bytes(4, 16, 16, 3) >= 4 * 3 * 8
    assert lib.nrf_ssim_loss_workspace_bytes(1, 64, 43, 3) >= 3 * 4 * 8
    for b, h, w, c in ((0, 11, 11, 1), (1, 10, 11, 1), (1, 11, 10, 1), (1, 11, 11, 0), (1, 11, 11, 5), (65536, 11, 11, 1), (16384, 11, 11, 4), (-1, 16, 16, 3)):
        assert lib.nrf_ssim_loss_workspace_bytes(b, h, w, c) == 0, (b, h, w, c)
    assert lib.nrf_rand_patches(1, 0, 0, 19, 0, 22, 1, 11, None, None, None) == 1 and b"nrf_rand_patches" in lib.nrf_last_error()


def test_dataset_refuses_a_batch_that_is_no_whole_number_of_patches():
    from nerfpp_amd import _lib as L
    from nerfpp_amd.dataset import NeRFDataset
    for bs, p in ((1000, 16), (0, 16), (256, -1)):
        with pytest.raises(L.NrfError):
            NeRFDataset([], bs, patch_size=p)
    assert NeRFDataset([], 1024, patch_size=16).PatchSize == 16 and NeRFDataset([], 1000).PatchSize == 0


def test_host_model_of_rand_patches():
    """Every patch inside the crop, origins spread over all admissible values, row-major elements."""
    rh, rw = SR.rand_patches(5, 3, 2, 21, 4, 26, 400, 11)          # a 20 x 23 crop: 10 x 13 origins
    rh, rw = rh.reshape(400, 11, 11), rw.reshape(400, 11, 11)
    assert rh.min() == 2 and rh.max() == 21 and rw.min() == 4 and rw.max() == 26
    assert (rh[:, 1:, :] - rh[:, :-1, :] == 1).all() and (rh[:, :, 1:] == rh[:, :, :-1]).all()
    assert (rw[:, :, 1:] - rw[:, :, :-1] == 1).all() and (rw[:, 1:, :] == rw[:, :-1, :]).all()
    assert len(set(rh[:, 0, 0].tolist())) == 10 and len(set(rw[:, 0, 0].tolist())) == 13
