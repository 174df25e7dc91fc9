"""GPU tests of the image metrics (image_metrics.hip: nrf_ssim, nrf_ms_ssim, nrf_image_mse; nerfpp_amd/metrics.py: MSE, PSNR, SSIM, MSSSIM, EvaluateViews).  The yardstick is
tests/metrics_ref.py (numpy float64 in the operation order the header states, with the library's own window), pinned by tests/test_metrics_host.py.

Bars.  The SSIM map: equal bits.  A mean over n values against numpy's sum / n: n * 2^-52 * (largest |term|, 1 for SSIM) -- the worst case of two summation orders of the
same terms.  Closed forms and the scale covariance: 1e-12 (a few dozen roundings of 1.1e-16 divided by c2 = 9e-4)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import metrics_ref as MR
import ordered_sum_ref as OS

pytestmark = pytest.mark.gpu

P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
host = lambda t: t.detach().cpu().numpy()
dev = lambda a: torch.from_numpy(np.array(a)).cuda()          # (a copy: the shared references are read-only)
bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)
EPS = 2.0 ** -52
PATTERN = -12345.678          # what the output buffers hold before a call


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from types import SimpleNamespace
    from nerfpp_amd import _lib as L, metrics as M, renderer as R, scene as S, dataset as D
    win = (C.c_double * 11)()
    L.check(L.lib().nrf_ssim_window(win))
    return SimpleNamespace(L=L, M=M, R=R, S=S, D=D, lib=L.lib(), g=np.array(list(win)))


_REF = {}


def ref_maps(api, kind, b, h, w, c):
    """The pair and the restatement's (ssim, cs) maps with the library's window; computed once per case and never modified."""
    key = (kind, b, h, w, c)
    if key not in _REF:
        x, y = MR.pair(kind, b, h, w, c)
        ssim, cs = MR.ssim_maps(x, y, api.g)
        for a in (x, y, ssim, cs):
            a.setflags(write=False)
        _REF[key] = (x, y, ssim, cs)
    return _REF[key]


def ssim_call(api, x, y, data_range=1.0, want_map=True, ws_bytes=None, shape=None, null=(), check=True):
    """One nrf_ssim call -> (means [b,c,2], map | None, status); the outputs hold PATTERN before it.  shape / ws_bytes / null override what the call is told."""
    b, h, w, c = x.shape
    dx, dy = dev(x), dev(y)
    means = torch.full((b, c, 2), PATTERN, device="cuda", dtype=torch.float64)
    smap = torch.full((b, h - 10, w - 10, c), PATTERN, device="cuda", dtype=torch.float64) if want_map else None
    tb, th, tw, tc = shape or (b, h, w, c)
    need = int(api.lib.nrf_ssim_workspace_bytes(b, h, w, c))
    nb = need if ws_bytes is None else ws_bytes
    ws = torch.empty((max(need, 8),), dtype=torch.uint8, device="cuda")
    a = dict(x=P(dx), y=P(dy), means=P(means), ws=P(ws))
    for k in null:
        a[k] = None
    rc = api.lib.nrf_ssim(a["x"], a["y"], tb, th, tw, tc, data_range, a["means"], P(smap), a["ws"], nb, None)
    torch.cuda.synchronize()
    if check:
        api.L.check(rc)
    return host(means), None if smap is None else host(smap), rc


def mean_bar(got, maps, what):
    """got [b, c] against numpy's sum of maps [b, oh, ow, c] / n, within n * 2^-52 (every |term| <= about 1)."""
    n = maps.shape[1] * maps.shape[2]
    ref = maps.sum(axis=(1, 2)) / n
    err = np.abs(got - ref).max()
    print(f"{what}: n = {n}, max |mean - numpy| = {err:.3e}, bar {n * EPS:.3e}")
    assert np.isfinite(got).all() and err <= n * EPS, what


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("shape", MR.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ssim_map_has_the_restatement_bits_and_the_means_its_sums(api, shape, b):
    h, w, c = shape
    for kind in ("noise", "indep"):
        x, y, ssim, cs = ref_maps(api, kind, b, h, w, c)
        means, smap, _ = ssim_call(api, x, y)
        diff = int((bits(smap) != bits(ssim)).sum())
        print(f"{kind} {b}x{h}x{w}x{c}: {diff} of {ssim.size} map values differ in bits, max |diff| = {np.abs(smap - ssim).max():.3e}")
        assert smap.shape == ssim.shape and diff == 0
        mean_bar(means[..., 0], ssim, f"{kind} mean ssim")
        mean_bar(means[..., 1], cs, f"{kind} mean cs")
        # determinism; and the map is optional without a change to the means
        means2, smap2, _ = ssim_call(api, x, y)
        assert (bits(means2) == bits(means)).all() and (bits(smap2) == bits(smap)).all()
        means3, none, _ = ssim_call(api, x, y, want_map=False)
        assert none is None and (bits(means3) == bits(means)).all()
        if b > 1:          # an image's result does not depend on the batch it came in
            for i in range(b):
                mi, si, _ = ssim_call(api, x[i:i + 1], y[i:i + 1])
                assert (bits(mi[0]) == bits(means[i])).all() and (bits(si[0]) == bits(smap[i])).all(), i


def test_channels_are_independent(api):
    x, y, _, _ = ref_maps(api, "noise", 3, 43, 42, 3)
    means, smap, _ = ssim_call(api, x, y)
    y2 = y.copy()
    y2[..., 1] = MR.pair("indep", 3, 43, 42, 3)[0][..., 1]
    means2, smap2, _ = ssim_call(api, x, y2)
    for ch in (0, 2):
        assert (bits(means2[:, ch]) == bits(means[:, ch])).all() and (bits(smap2[..., ch]) == bits(smap[..., ch])).all()
    assert (means2[:, 1, 0] < 0.5).all() and (means[:, 1, 0] > 0.85).all()          # and the changed channel did change


def test_fixed_values_same_and_flat(api):
    for h, w, c in MR.SHAPES:
        x, y = MR.pair("same", 2, h, w, c)
        means, smap, _ = ssim_call(api, x, y)
        assert (smap == 1.0).all() and (means == 1.0).all(), (h, w, c)
        x, y = MR.pair("flat", 2, h, w, c)
        means, smap, _ = ssim_call(api, x, y)
        err = max(np.abs(smap - 0.3751 / 0.6251).max(), np.abs(means[..., 0] - 0.3751 / 0.6251).max(), np.abs(means[..., 1] - 1.0).max())
        print(f"flat {h}x{w}x{c}: max |ssim - 0.3751/0.6251| = {err:.3e}")
        assert err < 1e-12, (h, w, c)
    x, y = (dev(a) for a in MR.pair("same", 2, 43, 42, 3))
    mse, psnr, ssim = api.M.MSE(x, y), api.M.PSNR(x, y), api.M.SSIM(x, y)
    assert mse.dtype == psnr.dtype == ssim.dtype == torch.float64 and mse.is_cuda and mse.shape == psnr.shape == ssim.shape == (2,)
    assert (host(mse) == 0.0).all() and np.isposinf(host(psnr)).all() and (host(ssim) == 1.0).all()
    xf, yf = (dev(a) for a in MR.pair("flat", 1, 12, 13, 3))
    assert abs(float(api.M.MSE(xf, yf)[0]) - 0.25) == 0.0 and abs(float(api.M.PSNR(xf, yf)[0]) - 10.0 * math.log10(4.0)) < 1e-14


def test_data_range_scales_with_the_images(api):
    """SSIM(255 x, 255 y, L = 255) == SSIM(x, y, L = 1).  The images hold integer levels k / 256, k = 0..256, so that scaling them by 255 is exact in fp32 (k / 255 is not
    an fp32 value, and its rounding alone would move SSIM by about 1e-7)."""
    h, w, c = 43, 42, 3
    x, y = MR.pair("noise", 2, h, w, c)
    x, y = ((np.round(a * 256.0) / 256.0).astype(np.float32) for a in (x, y))
    xs, ys = x * np.float32(255.0), y * np.float32(255.0)
    assert (xs.astype(np.float64) == x.astype(np.float64) * 255.0).all() and (ys.astype(np.float64) == y.astype(np.float64) * 255.0).all()
    m1, s1, _ = ssim_call(api, x, y, 1.0)
    m255, s255, _ = ssim_call(api, xs, ys, 255.0)
    err = max(np.abs(m1 - m255).max(), np.abs(s1 - s255).max())
    print(f"data_range 255 against 1: max |difference| = {err:.3e}; mean ssim {m1[..., 0].mean():.4f}")
    assert err < 1e-12 and 0.8 < m1[..., 0].mean() < 0.99
    r1, r255 = api.M.SSIM(dev(x), dev(y)), api.M.SSIM(dev(xs), dev(ys), data_range=255.0)
    assert (host(r1) - host(r255)).__abs__().max() < 1e-12
    p1, p255 = api.M.PSNR(dev(x), dev(y)), api.M.PSNR(dev(xs), dev(ys), data_range=255.0)
    assert np.abs(host(p1) - host(p255)).max() < 1e-12


@pytest.mark.parametrize("n", [1, 63, 64, 65, 70001])
def test_mse_against_numpy(api, n):
    b = 2
    x, y = MR.pair("indep", b, 1, n, 1)
    x, y = x.reshape(b, n), y.reshape(b, n)
    ref = MR.mse(x, y)
    d = x.astype(np.float64) - y.astype(np.float64)
    bar = n * EPS * (d * d).max()
    out = torch.full((b,), PATTERN, device="cuda", dtype=torch.float64)
    nb = int(api.lib.nrf_image_mse_workspace_bytes(b, n))
    ws = torch.empty((nb,), dtype=torch.uint8, device="cuda")
    dx, dy = dev(x), dev(y)
    got = []
    for _ in range(2):
        api.L.check(api.lib.nrf_image_mse(P(dx), P(dy), b, n, P(out), P(ws), nb, None))
        torch.cuda.synchronize()
        got.append(host(out).copy())
    print(f"n = {n}: max |mse - numpy| = {np.abs(got[0] - ref).max():.3e}, bar {bar:.3e}")
    assert (bits(got[0]) == bits(got[1])).all() and np.abs(got[0] - ref).max() <= bar
    via = host(api.M.MSE(dev(x.reshape(b, 1, n, 1)), dev(y.reshape(b, 1, n, 1))))
    assert (bits(via) == bits(got[0])).all()
    one = host(api.M.MSE(dev(x[1].reshape(1, n)), dev(y[1].reshape(1, n))))          # [H, W]: a scalar, the bits of the batched entry
    assert one.shape == () and bits(one) == bits(got[0][1])


@pytest.mark.parametrize("n", MR.ORDERED_MSE_ELEMS)
def test_mse_has_the_bits_of_the_ordered_sum_end_to_end(api, n):
    """nrf_image_mse's workspace ([b][blocks] doubles at offset 0) holds the restated block partials and the result is the ordered finish pass over them, bit for bit:
    the block epilogue and the finish pass, pinned together."""
    b = 2
    x, y = MR.ordered_mse_pair(n)
    blocks = -(-n // MR.MSE_PER_BLOCK)
    out = torch.full((b,), PATTERN, device="cuda", dtype=torch.float64)
    nb = int(api.lib.nrf_image_mse_workspace_bytes(b, n))
    assert nb >= b * blocks * 8
    ws = torch.zeros((nb,), dtype=torch.uint8, device="cuda")
    dx, dy = dev(x), dev(y)
    api.L.check(api.lib.nrf_image_mse(P(dx), P(dy), b, n, P(out), P(ws), nb, None))
    torch.cuda.synchronize()
    got, parts = host(out), host(ws[:b * blocks * 8].view(torch.float64)).reshape(b, blocks)
    want_parts = MR.mse_partials(x, y)
    print(f"n = {n}: {int((bits(parts) != bits(want_parts)).sum())} of {parts.size} partials differ in bits; mse {got}, restated {MR.mse_ordered(x, y)}")
    assert (bits(parts) == bits(want_parts)).all()
    assert (bits(got) == bits(np.array([OS.finish(p) / np.float64(n) for p in parts]))).all()
    assert (bits(got) == bits(MR.mse_ordered(x, y))).all()


@pytest.fixture(scope="module")
def ssim_many_tiles(api):
    """One image, one channel, a valid region of 17 x 16 tiles of 32 x 32 plus one pixel in each axis: 18 * 17 = 306 tile partials, a second strided trip of the
    finish pass that ends off a multiple of 256.  -> (means [1,1,2], the partials [306, 2] read back from the workspace, the valid count)"""
    h, w = 17 * 32 + 1 + 10, 16 * 32 + 1 + 10
    x, y = MR.pair("noise", 1, h, w, 1)
    tiles = 18 * 17
    need = int(api.lib.nrf_ssim_workspace_bytes(1, h, w, 1))
    assert need >= tiles * 2 * 8
    ws = torch.zeros((need,), dtype=torch.uint8, device="cuda")
    means = torch.full((1, 1, 2), PATTERN, device="cuda", dtype=torch.float64)
    dx, dy = dev(x), dev(y)
    api.L.check(api.lib.nrf_ssim(P(dx), P(dy), 1, h, w, 1, 1.0, P(means), None, P(ws), need, None))
    torch.cuda.synchronize()
    return host(means), host(ws[:tiles * 2 * 8].view(torch.float64)).reshape(tiles, 2), (h - 10) * (w - 10)


@pytest.mark.parametrize("col", [0, 1], ids=["ssim", "cs"])
def test_ssim_means_have_the_bits_of_the_ordered_finish_pass(ssim_many_tiles, col):
    means, parts, n = ssim_many_tiles
    want = OS.finish(parts[:, col]) / np.float64(n)
    print(f"column {col}: mean {means[0, 0, col]!r}, finish(partials) / n {want!r}, numpy's sum / n {parts[:, col].sum() / n!r}")
    assert len(parts) > 256 and len(parts) % 256 and np.isfinite(parts).all() and (parts[:, col] != 0.0).all()
    assert bits(means[0, 0, col]) == bits(want)


def ms_call(api, x, y, scales, data_range=1.0, ws_bytes=None, check=True):
    b, h, w, c = x.shape
    means = torch.full((max(scales, 1), b, c, 2), PATTERN, device="cuda", dtype=torch.float64)
    need = int(api.lib.nrf_ms_ssim_workspace_bytes(b, h, w, c, scales))
    nb = need if ws_bytes is None else ws_bytes
    ws = torch.empty((max(need, 8),), dtype=torch.uint8, device="cuda")
    dx, dy = dev(x), dev(y)
    rc = api.lib.nrf_ms_ssim(P(dx), P(dy), b, h, w, c, data_range, scales, P(means), P(ws), nb, None)
    torch.cuda.synchronize()
    if check:
        api.L.check(rc)
    return host(means), rc


@pytest.mark.parametrize("kind", ["noise", "indep"])
def test_ms_ssim_scale_means_and_combination(api, kind):
    b, h, w, c = 2, 176, 191, 3
    x, y = MR.pair(kind, b, h, w, c)
    ref, sizes = MR.ms_ssim_scale_means(x, y, api.g, 1.0, 5)
    assert sizes == [(176, 191), (88, 95), (44, 47), (22, 23), (11, 11)]
    got, _ = ms_call(api, x, y, 5)
    again, _ = ms_call(api, x, y, 5)
    assert (bits(got) == bits(again)).all()
    for i, (hi, wi) in enumerate(sizes):
        n = (hi - 10) * (wi - 10)
        err = np.abs(got[i] - ref[i]).max()
        print(f"{kind} scale {i} ({hi}x{wi}): max |mean - restatement| = {err:.3e}, bar {n * EPS:.3e}; mean cs {ref[i, ..., 1].mean():.4f}")
        assert err <= n * EPS, i
    s0, _, _ = ssim_call(api, x, y, want_map=False)
    assert (bits(got[0]) == bits(s0)).all()          # scale 0 is nrf_ssim's computation
    want = MR.ms_ssim_combine(ref)
    res = api.M.MSSSIM(dev(x), dev(y))
    assert res.dtype == torch.float64 and res.is_cuda and res.shape == (b,)
    print(f"{kind} MS-SSIM {host(res)}, numpy {want}")
    assert np.abs(host(res) - want).max() < 1e-12
    three = host(api.M.MSSSIM(dev(x[0]), dev(y[0]), weights=(0.2, 0.3, 0.5)))          # [H, W, C] and another number of scales
    assert three.shape == () and abs(three - MR.ms_ssim_combine(ref[:3, :1], (0.2, 0.3, 0.5))[0]) < 1e-12


def test_ms_ssim_needs_eleven_pixels_at_the_last_scale(api):
    x, y = MR.pair("noise", 1, 175, 300, 3)
    got, rc = ms_call(api, x, y, 5, check=False)          # 175 >> 4 = 10
    assert rc == 1 and (got == PATTERN).all() and b"nrf_ms_ssim" in api.lib.nrf_last_error()
    with pytest.raises(api.L.NrfError):
        api.M.MSSSIM(dev(x), dev(y))
    got, rc = ms_call(api, x, y, 4)
    ref, sizes = MR.ms_ssim_scale_means(x, y, api.g, 1.0, 4)
    assert rc == 0 and sizes[-1] == (21, 37)
    for i, (hi, wi) in enumerate(sizes):
        assert np.abs(got[i] - ref[i]).max() <= (hi - 10) * (wi - 10) * EPS, i


def test_refusals_launch_nothing_and_write_nothing(api):
    h, w, c = 43, 42, 3
    x, y, ssim, cs = ref_maps(api, "noise", 1, h, w, c)
    need = int(api.lib.nrf_ssim_workspace_bytes(1, h, w, c))
    INVALID, WORKSPACE = 1, 4
    cases = [(dict(shape=(1, 10, w, c)), INVALID), (dict(shape=(1, h, 10, c)), INVALID), (dict(shape=(0, h, w, c)), INVALID), (dict(shape=(1, h, w, 0)), INVALID),
             (dict(shape=(1, h, w, 5)), INVALID), (dict(data_range=0.0), INVALID), (dict(data_range=-1.0), INVALID), (dict(data_range=float("nan")), INVALID),
             (dict(data_range=float("inf")), INVALID), (dict(null=("x",)), INVALID), (dict(null=("y",)), INVALID), (dict(null=("means",)), INVALID),
             (dict(null=("ws",)), INVALID), (dict(ws_bytes=need - 1), WORKSPACE), (dict(ws_bytes=0), WORKSPACE)]
    for kw, want in cases:
        means, smap, rc = ssim_call(api, x, y, check=False, **kw)
        assert rc == want and (means == PATTERN).all() and (smap == PATTERN).all(), (kw, rc)
        assert b"nrf_ssim" in api.lib.nrf_last_error()
    # MS-SSIM: scales, the last scale's size, data_range, a short workspace
    xm, ym = MR.pair("noise", 1, 44, 47, 3)
    ms_need = int(api.lib.nrf_ms_ssim_workspace_bytes(1, 44, 47, 3, 3))
    for kw, want in ((dict(scales=0), INVALID), (dict(scales=6), INVALID), (dict(scales=4), INVALID), (dict(scales=3, data_range=0.0), INVALID),
                     (dict(scales=3, ws_bytes=ms_need - 1), WORKSPACE)):
        got, rc = ms_call(api, xm, ym, check=False, **kw)
        assert rc == want and (got == PATTERN).all(), (kw, rc)
    # MSE: the element count, the batch, null pointers, a short workspace
    n = 5000
    dx, dy = dev(np.zeros((1, n), np.float32)), dev(np.ones((1, n), np.float32))
    out = torch.full((1,), PATTERN, device="cuda", dtype=torch.float64)
    nb = int(api.lib.nrf_image_mse_workspace_bytes(1, n))
    ws = torch.empty((nb,), dtype=torch.uint8, device="cuda")
    for args, want in (((P(dx), P(dy), 1, 0, P(out), P(ws), nb), INVALID), ((P(dx), P(dy), 0, n, P(out), P(ws), nb), INVALID), ((None, P(dy), 1, n, P(out), P(ws), nb), INVALID),
                       ((P(dx), None, 1, n, P(out), P(ws), nb), INVALID), ((P(dx), P(dy), 1, n, None, P(ws), nb), INVALID), ((P(dx), P(dy), 1, n, P(out), P(ws), nb - 1), WORKSPACE),
                       ((P(dx), P(dy), 1, n, P(out), None, nb), INVALID), ((P(dx), P(dy), 1, n, P(out), P(ws), 0), WORKSPACE)):
        rc = api.lib.nrf_image_mse(*args, None)
        torch.cuda.synchronize()
        assert rc == want and (host(out) == PATTERN).all(), (args[2:4], rc)
    # the Python surface refuses what it can see
    with pytest.raises(api.L.NrfError):
        api.M.SSIM(dev(x), dev(y[:, :, :-1]))
    with pytest.raises(api.L.NrfError):
        api.M.SSIM(dev(x[:, :10]), dev(y[:, :10]))
    # a valid call right afterwards succeeds
    means, smap, rc = ssim_call(api, x, y)
    assert rc == 0 and (bits(smap) == bits(ssim)).all()
    api.L.check(api.lib.nrf_image_mse(P(dx), P(dy), 1, n, P(out), P(ws), nb, None))
    torch.cuda.synchronize()
    assert host(out)[0] == 1.0


def test_python_surface_shapes_and_dtypes(api):
    x, y, ssim, cs = ref_maps(api, "noise", 3, 43, 42, 3)
    ref = MR.means_of(ssim, cs)[..., 0]          # [b, c]
    n = ssim.shape[1] * ssim.shape[2]
    dx, dy = dev(x), dev(y)
    per, smap = api.M.SSIM(dx, dy, per_channel=True, return_map=True)
    assert per.shape == (3, 3) and per.dtype == torch.float64 and smap.shape == ssim.shape and (bits(host(smap)) == bits(ssim)).all()
    assert np.abs(host(per) - ref).max() <= n * EPS
    mean = api.M.SSIM(dx, dy)
    assert mean.shape == (3,) and np.abs(host(mean) - ref.mean(axis=1)).max() <= n * EPS + 2 * EPS
    one, m1 = api.M.SSIM(dx[1], dy[1], per_channel=True, return_map=True)          # [H, W, C]
    assert one.shape == (3,) and (bits(host(one)) == bits(host(per[1]))).all() and m1.shape == ssim.shape[1:]
    g = api.M.SSIM(dx[1, ..., 2], dy[1, ..., 2], per_channel=True)                # [H, W]: the same numbers as that channel of the colour image
    assert g.shape == (1,) and bits(host(g))[0] == bits(host(per[1, 2]))
    # any dtype: float64 and uint8 images are scored as their fp32 values
    u8x, u8y = (dx * 255).to(torch.uint8), (dy * 255).to(torch.uint8)
    a = api.M.SSIM(u8x, u8y, data_range=255.0)
    bb = api.M.SSIM(u8x.float(), u8y.double(), data_range=255.0)
    assert (bits(host(a)) == bits(host(bb))).all()
    w = api.M.SsimWindow()
    assert w.dtype == torch.float64 and (w.numpy() == api.g).all()
    direct = 10.0 * np.log10(1.0 / MR.mse(x, y))
    assert np.abs(host(api.M.PSNR(dx, dy)) - direct).max() < 1e-12


def test_evaluate_views(api):
    """Two 24 x 20 views of a small hash scene (table 2^14, 16 + 16 samples, NRF_PREC_F32)."""
    S, M, D, R = api.S, api.M, api.D, api.R
    sc = S.make_hash_scene(mode="cu", log2_t=14, seed=5000)
    W, H = 24, 20
    K = S.lego_K(H, W)
    rp = S.lego_render_params(sc["bbox"], n_samples=16, n_importance=16, chunk=4096)
    poses = [S.pose_spherical(30.0, -30.0, 4.0), S.pose_spherical(-70.0, -20.0, 4.0)]
    renders = [R.RenderView(sc["renderer"], p, W, H, K, rp).Outputs.RGBMap.clone() for p in poses]
    assert renders[0].shape == (H, W, 3) and float((renders[0] - renders[1]).abs().max()) > 0.01
    views = [D.View(H=H, W=W, K=K, Pose=p, Image=r) for p, r in zip(poses, renders)]
    res = M.EvaluateViews(sc["renderer"], views, rp)
    assert sorted(res) == ["mean_psnr", "mean_ssim", "psnr", "ssim"]
    for k in ("psnr", "ssim"):
        assert res[k].shape == (2,) and res[k].dtype == torch.float64 and res[k].is_cuda and res["mean_" + k].shape == ()
    assert np.isposinf(host(res["psnr"])).all() and (host(res["ssim"]) == 1.0).all() and float(res["mean_ssim"]) == 1.0
    # perturbed images: every entry has the bits of the direct call on the same pair
    noise = dev(MR.pair("indep", 2, H, W, 3)[0])
    for v, r, nz in zip(views, renders, noise):
        v.Image = (r + 0.1 * (nz - 0.5)).clamp(0.0, 1.0)
    res = M.EvaluateViews(sc["renderer"], views, rp, metrics=("psnr", "ssim", "mse"))
    for i, (v, r) in enumerate(zip(views, renders)):
        assert bits(host(res["psnr"][i])) == bits(host(M.PSNR(r, v.Image))) and bits(host(res["ssim"][i])) == bits(host(M.SSIM(r, v.Image)))
        assert bits(host(res["mse"][i])) == bits(host(M.MSE(r, v.Image)))
    assert 20.0 < float(res["mean_psnr"]) < 40.0 and 0.3 < float(res["mean_ssim"]) < 1.0
    assert bits(host(res["mean_psnr"])) == bits(host(res["psnr"].mean()))
    # quantize: what the written 8-bit image would score
    resq = M.EvaluateViews(sc["renderer"], views, rp, quantize=True)
    for i, (v, r) in enumerate(zip(views, renders)):
        q = R.TorchTensorToCVMat(r).to(torch.float32) / 255.0
        assert bits(host(resq["psnr"][i])) == bits(host(M.PSNR(q, v.Image))) and bits(host(resq["ssim"][i])) == bits(host(M.SSIM(q, v.Image)))
    assert (host(resq["psnr"]) != host(res["psnr"])).any()
    # a view without an image, an unknown metric
    views[1].Image = None
    with pytest.raises(api.L.NrfError):
        M.EvaluateViews(sc["renderer"], views, rp)
    with pytest.raises(api.L.NrfError):
        M.EvaluateViews(sc["renderer"], views[:1], rp, metrics=("lpips",))
