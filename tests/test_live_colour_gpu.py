"""GPU tests of the fine pass's colour launch over the coarse depths with sigma > 0 only (live_points.hip: nrf_live_points; mlp_small_mfma.hip:
k_mlp_small_colour_list; render.hip: the geo_reuse branch; the switch nrf_set_live_colour).

A coarse depth whose sigma is not positive has alpha = 0 and a weight of exactly 0 in the compositing kernel, so its colour cannot change a bit of any output: every
render here is compared bit for bit with the same render with the switch off, which runs the colour net at every coarse depth as before."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

host = lambda t: t.detach().cpu().numpy()
P = lambda t: None if t is None else t.data_ptr()


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from types import SimpleNamespace
    from nerfpp_amd import _lib as L, modules as M, renderer as R, scene as S
    return SimpleNamespace(L=L, M=M, R=R, S=S, lib=L.lib())


# ------------------------------------------------------------------ the compaction on its own
SIZES = (1, 63, 64, 65, 511, 512, 513, 100003)          # around a wave's 64 and 512 points, a workgroup's 2 048 several times over, ragged


def patterns(p):
    rng = np.random.default_rng(p)
    pos = (rng.random(p, dtype=np.float32) + np.float32(0.5)).astype(np.float32)
    neg = -pos
    out = {"all positive": pos.copy(), "none positive": neg.copy()}
    alt = neg.copy(); alt[::2] = pos[::2]
    out["alternating"] = alt
    first = neg.copy(); first[0] = 3.0
    out["one live point, first"] = first
    last = neg.copy(); last[-1] = 3.0
    out["one live point, last"] = last
    mixed = rng.standard_normal(p).astype(np.float32)
    special = np.array([np.nan, 0.0, -0.0, np.float32(1e-42), -np.inf], np.float32)          # NaN, +0, -0 and -inf are dead; the positive denormal is live
    assert special[3] > 0 and special[3] < np.finfo(np.float32).tiny
    where = rng.random(p) < 0.3
    mixed[where] = special[rng.integers(0, special.size, int(where.sum()))]
    mixed[:min(p, special.size)] = special[:min(p, special.size)]          # each at least once where the size allows
    out["random with NaN, +0, -0, a denormal and -inf"] = mixed
    return out


@pytest.mark.parametrize("p", SIZES)
def test_live_points_equals_numpy_nonzero(api, p):
    """nrf_live_points against numpy.nonzero(sigma > 0): the list and the count bit for bit; the rows of the dead points (0, 0, 0, sigma) with the sigma word compared
    as uint32 (a NaN keeps its bits); rows of live points untouched; entries of the list beyond the count are not looked at."""
    lib = api.lib
    need = lib.nrf_live_points_workspace_bytes(p)
    ws = torch.empty((max(int(need), 1),), device="cuda", dtype=torch.uint8)
    for name, sg in patterns(p).items():
        d_sigma = torch.from_numpy(sg).cuda()
        d_list = torch.full((p,), -7, device="cuda", dtype=torch.int32)
        d_count = torch.full((1,), -7, device="cuda", dtype=torch.int32)
        fill = np.float32(123.5)
        d_rows = torch.full((p, 4), float(fill), device="cuda", dtype=torch.float32)
        api.L.check(lib.nrf_live_points(P(d_sigma), p, P(d_list), P(d_count), P(d_rows), P(ws), int(need), None))
        torch.cuda.synchronize()
        ref = np.nonzero(sg > 0)[0].astype(np.int32)
        count = int(host(d_count)[0])
        assert count == ref.size, (p, name, count, ref.size)
        assert np.array_equal(host(d_list)[:count], ref), (p, name)
        rows = host(d_rows).view(np.uint32)
        want = np.full((p, 4), fill, np.float32).view(np.uint32)
        dead = ~(sg > 0)
        want[dead, :3] = 0
        want[dead, 3] = sg.view(np.uint32)[dead]
        assert np.array_equal(rows, want), (p, name)
        # without the rows: the same list
        d_list2 = torch.full((p,), -7, device="cuda", dtype=torch.int32)
        api.L.check(lib.nrf_live_points(P(d_sigma), p, P(d_list2), P(d_count), None, P(ws), int(need), None))
        torch.cuda.synchronize()
        assert int(host(d_count)[0]) == ref.size and np.array_equal(host(d_list2)[:ref.size], ref), (p, name, "no rows")


# ------------------------------------------------------------------ renders, switch on against off
@pytest.fixture(scope="module")
def cu_scene(api):
    return api.S.make_hash_scene(mode="cu", log2_t=14)


def rays_of(api, n):
    rows = (n + 199) // 200
    o, d, _ = api.R.GetRays(200, 200, api.S.lego_K(200, 200), api.S.pose_spherical(10.0, -30.0, 4.0), row0=min(90, 200 - rows), rows=rows)
    return o.reshape(-1, 3)[:n].contiguous(), d.reshape(-1, 3)[:n].contiguous()


def render(api, renderer, bbox, o, d, on, chunk=4096, lanes=0, **kw):
    """one NRF_PREC_F16_SPLIT render at 32 + 32 samples (the smallest the geo hand-over path takes) -> dict of host arrays"""
    lib = api.lib
    before = lib.nrf_get_live_colour()
    api.L.check(lib.nrf_set_live_colour(int(on)))
    api.L.check(lib.nrf_renderer_set_lanes(renderer._r, lanes))
    try:
        assert lib.nrf_get_live_colour() == int(on)
        rp = api.S.lego_render_params(bbox, 32, 32, chunk, api.L.NRF_PREC_F16_SPLIT, ReturnWeights=True, **kw)
        res = renderer.Render(0, 0, None, rp, rays=(o, d, None))
        torch.cuda.synchronize()
    finally:
        api.L.check(lib.nrf_set_live_colour(before))
        api.L.check(lib.nrf_renderer_set_lanes(renderer._r, 0))
    out = dict(rgb=host(res.Outputs.RGBMap), depth=host(res.Outputs.DepthMap), disp=host(res.Outputs.DispMap), acc=host(res.Outputs.AccMap),
               weights=host(res.Outputs.Weights))
    if res.Raw is not None:
        out["raw"] = host(res.Raw)
    return out


def equal_maps(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), f"{what}: {k} differs between the switch on and off"


@pytest.mark.parametrize("n", (1, 37, 513))
def test_render_equals_switch_off(api, cu_scene, n):
    """RGB, depth, disparity, acc and the weights of a CuHash scene's split render, bit for bit, with the live-column colour launch and without.  The scene has dead
    coarse depths and live ones (asserted on the weights), so the listed launch really runs on a proper subset."""
    o, d = rays_of(api, n)
    r = cu_scene["renderer"]
    off = render(api, r, cu_scene["bbox"], o, d, 0)
    on = render(api, r, cu_scene["bbox"], o, d, 1)
    assert np.isfinite(on["rgb"]).all() and (on["weights"] > 0).any() and (on["weights"] == 0).any()
    equal_maps(on, off, f"n {n}")


def test_render_in_chunks_on_two_lanes(api, cu_scene):
    """300 rays in chunks of 128 (128, 128, 44) with two lanes asked for -- a batch this small stays on the caller's stream, so this is the ragged Chunk loop -- and
    33 000 rays in chunks of 9 000, which do run on two lanes, each lane with its own list, count and block sums in its slice of the workspace."""
    r = cu_scene["renderer"]
    for n, chunk in ((300, 128), (33000, 9000)):
        o, d = rays_of(api, n)
        off = render(api, r, cu_scene["bbox"], o, d, 0, chunk=chunk, lanes=2)
        on = render(api, r, cu_scene["bbox"], o, d, 1, chunk=chunk, lanes=2)
        equal_maps(on, off, f"n {n} chunk {chunk} lanes 2")
        one = render(api, r, cu_scene["bbox"], o, d, 1, chunk=chunk, lanes=1)
        equal_maps(on, one, f"n {n} chunk {chunk} lanes 2 vs 1")


def test_all_dead_scene(api, cu_scene):
    """Row 0 of the sigma net's last layer zeroed: sigma is 0 at every point, every coarse column is dead and the listed launch gets count == 0 -- it must run no
    iteration.  Equal to the switch off; a finite white-background image; nothing reported non-finite."""
    blob = cu_scene["mlp_blob"].copy()
    at = 64 * 32 + 64 * 64          # sigma_net_0 [64, 32], sigma_net_1 [64, 64], then sigma_net_2 [1 + 15, 64]: its row 0 is sigma
    blob[at:at + 64] = 0.0
    mlp = api.M.NeRFSmall(3, 64, 15, 4, 64, False, 3, 64, 32, 16, "model", params=blob)
    r = api.R.NeRFRenderer(cu_scene["embedder"], cu_scene["embeddirs"], mlp)
    o, d = rays_of(api, 513)
    off = render(api, r, cu_scene["bbox"], o, d, 0)
    on = render(api, r, cu_scene["bbox"], o, d, 1)
    equal_maps(on, off, "all dead")
    assert (on["weights"] == 0).all() and (on["acc"] == 0).all()
    assert np.array_equal(on["rgb"], np.ones_like(on["rgb"])), "white background where nothing absorbs"
    assert r.nonfinite() == (0, 0)


def test_raw_requested_takes_the_unlisted_launch(api, cu_scene):
    """ReturnRaw=True: a caller of Raw keeps getting every colour, so the switch changes nothing -- Raw and the maps bit for bit equal to the switch off, and the rgb of
    Raw at dead coarse depths is the colour net's output, not the dead row's zeros."""
    o, d = rays_of(api, 513)
    r = cu_scene["renderer"]
    off = render(api, r, cu_scene["bbox"], o, d, 0, ReturnRaw=True)
    on = render(api, r, cu_scene["bbox"], o, d, 1, ReturnRaw=True)
    equal_maps(on, off, "Raw requested")
    dead = ~(on["raw"][..., 3] > 0)
    assert dead.any() and (on["raw"][..., :3][dead] != 0).any()


def test_sigma_noise_takes_the_unlisted_launch(api, cu_scene):
    """RawNoiseStd > 0 can lift a dead sigma above zero in the compositing kernel, so such a render evaluates every colour: equal to the switch off."""
    o, d = rays_of(api, 37)
    r = cu_scene["renderer"]
    off = render(api, r, cu_scene["bbox"], o, d, 0, RawNoiseStd=1.0, Seed=11)
    on = render(api, r, cu_scene["bbox"], o, d, 1, RawNoiseStd=1.0, Seed=11)
    equal_maps(on, off, "sigma noise")
