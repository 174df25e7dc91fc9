"""CPU tests of the image metrics: the float64 yardstick (tests/metrics_ref.py) is pinned first -- against an independent definition built on scipy.ndimage.correlate1d,
and at the pairs whose SSIM is known in closed form -- then the host pieces of the library: the window nrf_ssim_window returns, the size functions' refusals, and the
MS-SSIM combination of nerfpp_amd.metrics."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import metrics_ref as MR

FLAT = 0.3751 / 0.6251          # lum of 0.25 against 0.75 with c1 = 1e-4; cs is c2 / c2


@pytest.mark.parametrize("kind", ["noise", "indep"])
def test_restatement_agrees_with_an_independent_definition(kind):
    """1e-10: about 20 roundings of 1.1e-16 in the moments, divided by c2 = 9e-4 where the variances cancel (measured: 1.3e-13)."""
    g = MR.window()
    for h, w, c in MR.SHAPES:
        x, y = MR.pair(kind, 2, h, w, c)
        ssim, cs = MR.ssim_maps(x, y, g)
        ref = MR.ssim_independent(x, y)
        err = np.abs(ssim - ref).max()
        print(f"{kind} {h}x{w}x{c}: max |restatement - independent| = {err:.2e}, ssim in [{ssim.min():.4f}, {ssim.max():.4f}]")
        assert ssim.shape == (2, h - 10, w - 10, c) == cs.shape and err < 1e-10


def test_the_seeded_pairs_cover_the_range_of_ssim():
    """noise: high but not 1; indep: around 0 with negative pixels (the sign the MS-SSIM clamp exists for)."""
    g = MR.window()
    x, y = MR.pair("noise", 3, 43, 42, 3)
    m = MR.means_of(*MR.ssim_maps(x, y, g))[..., 0]
    assert 0.89 < m.min() and m.max() < 0.95 and x.dtype == np.float32 and 0.0 <= min(x.min(), y.min()) and max(x.max(), y.max()) <= 1.0
    x, y = MR.pair("indep", 3, 43, 42, 3)
    ssim, _ = MR.ssim_maps(x, y, g)
    assert np.abs(MR.means_of(ssim, ssim)[..., 0]).max() < 0.05 and ssim.min() < -0.5 and ssim.max() > 0.5


def test_equal_images_give_exactly_one_at_every_pixel():
    """Numerator and denominator are the same operations on equal values."""
    g = MR.window()
    for h, w, c in MR.SHAPES:
        x, y = MR.pair("same", 2, h, w, c)
        ssim, cs = MR.ssim_maps(x, y, g)
        assert (ssim == 1.0).all() and (cs == 1.0).all(), (h, w, c)
        assert (MR.mse(x, y) == 0.0).all()


def test_flat_pair_gives_the_closed_form():
    g = MR.window()
    for h, w, c in MR.SHAPES:
        x, y = MR.pair("flat", 1, h, w, c)
        ssim, cs = MR.ssim_maps(x, y, g)
        assert np.abs(ssim - FLAT).max() < 1e-12 and np.abs(cs - 1.0).max() < 1e-12, (h, w, c)


def test_pooling_drops_the_odd_row_and_column():
    a = np.arange(2 * 5 * 7 * 1, dtype=np.float32).reshape(2, 5, 7, 1)
    p = MR.pool2(a)
    assert p.shape == (2, 2, 3, 1) and p.dtype == np.float64
    assert p[1, 1, 2, 0] == (a[1, 2, 4, 0] + a[1, 2, 5, 0] + a[1, 3, 4, 0] + a[1, 3, 5, 0]) / 4.0
    _, sizes = MR.ms_ssim_scale_means(*MR.pair("noise", 1, 176, 191, 1), MR.window())
    assert sizes == [(176, 191), (88, 95), (44, 47), (22, 23), (11, 11)]


def test_library_window_equals_the_numpy_window():
    from nerfpp_amd import _lib
    out = (C.c_double * 11)()
    assert _lib.lib().nrf_ssim_window(out) == 0
    got, ref = np.array(list(out)), MR.window()
    print(f"max |library window - numpy window| = {np.abs(got - ref).max():.2e}, sum - 1 = {got.sum() - 1.0:.2e}")
    assert np.abs(got - ref).max() < 1e-15 and abs(got.sum() - 1.0) < 1e-15 and abs(ref.sum() - 1.0) < 1e-15
    assert (got == got[::-1]).all() and got.argmax() == 5
    assert _lib.lib().nrf_ssim_window(None) == 1 and b"nrf_ssim_window" in _lib.lib().nrf_last_error()


def test_size_functions_refuse_what_the_entries_refuse():
    from nerfpp_amd import _lib
    lib = _lib.lib()
    assert lib.nrf_ssim_workspace_bytes(1, 11, 11, 1) > 0 and lib.nrf_ssim_workspace_bytes(3, 40, 267, 4) >= 3 * 4 * 9 * 16
    for b, h, w, c in ((0, 11, 11, 1), (1, 10, 11, 1), (1, 11, 10, 1), (1, 11, 11, 0), (1, 11, 11, 5), (70000, 11, 11, 1)):
        assert lib.nrf_ssim_workspace_bytes(b, h, w, c) == 0, (b, h, w, c)
    assert lib.nrf_ms_ssim_workspace_bytes(1, 175, 300, 3, 5) == 0 and lib.nrf_ms_ssim_workspace_bytes(1, 175, 300, 3, 4) > 0
    assert lib.nrf_ms_ssim_workspace_bytes(1, 176, 191, 3, 5) > 0 and lib.nrf_ms_ssim_workspace_bytes(1, 176, 191, 3, 6) == 0
    assert lib.nrf_ms_ssim_workspace_bytes(1, 176, 191, 3, 0) == 0
    assert lib.nrf_image_mse_workspace_bytes(1, 1) > 0 and lib.nrf_image_mse_workspace_bytes(1, 0) == 0 and lib.nrf_image_mse_workspace_bytes(0, 5) == 0
    # null pointers are refused before anything touches a device
    assert lib.nrf_ssim(None, None, 1, 11, 11, 1, 1.0, None, None, None, 0, None) == 1
    assert lib.nrf_image_mse(None, None, 1, 4, None, None, 0, None) == 1
    assert lib.nrf_ms_ssim(None, None, 1, 11, 11, 1, 1.0, 1, None, None, 0, None) == 1


def test_ms_ssim_combination_on_hand_made_scale_means():
    """[scales, b, c, 2] = (ssim, cs): cs of every scale but the last, ssim of the last; a negative cs clamps to 0 and zeroes its channel."""
    from nerfpp_amd import metrics
    m = np.zeros((3, 1, 2, 2))
    m[0, 0, :, 1] = (0.9, -0.2); m[1, 0, :, 1] = (0.8, 0.5); m[2, 0, :, 0] = (0.7, 0.6)
    m[0, 0, :, 0] = (0.1, 0.1); m[1, 0, :, 0] = (0.1, 0.1); m[2, 0, :, 1] = (0.1, -0.9)          # the entries the combination must not read
    wt = (0.2, 0.3, 0.5)
    want = 0.5 * (0.9 ** 0.2 * 0.8 ** 0.3 * 0.7 ** 0.5 + 0.0)
    assert abs(MR.ms_ssim_combine(m, wt)[0] - want) < 1e-15
    got = metrics.CombineMsSsim(torch.from_numpy(m), wt)
    assert got.dtype == torch.float64 and got.shape == (1,) and abs(float(got[0]) - want) < 1e-15
    # the published five weights sum to 1.0001: equal scale means v combine to v^1.0001
    five = np.full((5, 2, 3, 2), 0.5)
    assert tuple(metrics.MS_SSIM_WEIGHTS) == MR.MS_WEIGHTS == (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
    v = 0.5 ** 1.0001
    assert np.abs(MR.ms_ssim_combine(five) - v).max() < 1e-15 and (metrics.CombineMsSsim(torch.from_numpy(five)) - v).abs().max() < 1e-15
    with pytest.raises(Exception):
        metrics.CombineMsSsim(torch.from_numpy(five), wt)
    assert math.isinf(float(10.0 * torch.log10(1.0 / torch.zeros((), dtype=torch.float64))))          # PSNR's form at mse == 0


def test_package_exports_metrics():
    import nerfpp_amd
    assert "metrics" in nerfpp_amd.__all__
    for name in ("MSE", "PSNR", "SSIM", "MSSSIM", "EvaluateViews"):
        assert callable(getattr(nerfpp_amd.metrics, name))
