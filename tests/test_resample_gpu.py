"""GPU tests of the renderer's one-kernel resampling (composite.hip: k_resample; live_points.hip: k_ray_scan, k_mask_scatter; render.hip: the default HashNeRF
path; the switch nrf_set_fused_resample).

The fused pair moves the arithmetic of three stages as the device functions those stages have, so nothing here has a tolerance: the debug entry must equal the
composition of the stage entries (nrf_raw2weights -> nrf_fine_depths_merge / nrf_fine_depths_rand / nrf_sample_pdf_rand -> nrf_live_points) bit for bit, and a render
must not change a bit with the switch."""
import numpy as np
import pytest
import torch

import per_ray_ref as PR

pytestmark = pytest.mark.gpu

host = lambda t: t.detach().cpu().numpy()
P = lambda t: None if t is None else t.data_ptr()
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)

N = 257                                              # 64 full workgroups of four rays and one with a single ray
S_ALL = (2, 3, 5, 63, 64, 65, 128, 129, 256)         # both sides of every 64-sample block edge; 64 | 65 is also the edge between the two instantiations
NS_ALL = (1, 2, 64, 128, 129, 256)                   # 128 | 129 likewise
SEED, RAY_BASE = 77, 1000


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from types import SimpleNamespace
    from nerfpp_amd import _lib as L, modules as M, renderer as R, scene as S
    return SimpleNamespace(L=L, M=M, R=R, S=S, lib=L.lib())


def stage_inputs(s):
    """z [N, s], dirs [N, 3], sigma [N, s]: densities as per_ray_ref.composite_case draws them, then the rows the fused kernel could get wrong."""
    rng = np.random.default_rng(9000 + s)
    z, d = PR._depths(rng, N, s), PR._dirs(rng, N)
    sg = ((rng.standard_normal((N, s)) + 0.3) * 10.0 ** rng.uniform(-1.0, 1.3, (N, 1))).astype(np.float32)
    sg[0] = -np.abs(sg[0]) - 0.01                    # all dead
    sg[1] = np.abs(sg[1]) + 0.01                     # all live
    sg[2, ::2] = -0.0                                # -0.0: dead, alpha 0
    sg[3, s // 2] = np.inf                           # +inf: live, alpha 1
    sg[4, s // 2] = np.nan                           # NaN: dead under sigma > 0; the row keeps its bits
    sg[5, s - 1] = np.nan
    sg[6, 0] = 0.0                                   # a keep-masked sample as the exact coarse kernel stores it
    sg[6, s - 1] = 0.0
    sg[7] = np.float32(1e-42)                        # positive denormals: live
    z[8] = (np.float32(2.0) + np.float32(1e-6) * np.linspace(0.0, 1.0, s)).astype(np.float32)          # near and far 1e-6 apart: every depth ties
    if s >= 4:
        a = s // 2
        z[9, a + 1] = np.nextafter(z[9, a], np.float32(-np.inf), dtype=np.float32)          # one ulp out of order: the exhaustive-rank fallback
        z[10, [a, a + 1]] = z[10, [a + 1, a]]
    return z, d, sg


def counts_len(n):
    """int32 words of nrf_dbg_resample's d_counts: the per-ray counts, then (16-byte aligned) the list offsets of the groups of 64 rays"""
    return (n + 3) // 4 * 4 + (n + 63) // 64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("s", S_ALL)
def test_stage_equals_composition(api, s):
    """nrf_dbg_resample against the stage entries at every (ns, sum_vec, draw kind): z_fine, src, z_new, the coarse weights, list, count and the dead rows, as uint32."""
    lib, L = api.lib, api.L
    z, d, sg = stage_inputs(s)
    d_z, d_d, d_sg = dev(z), dev(d), dev(sg)
    p = N * s
    # ---- the references that do not depend on ns: weights and the live list (computed once per s)
    d_w = torch.empty((N, s), device="cuda")
    L.check(lib.nrf_raw2weights(P(d_sg), 1, 0, P(d_z), P(d_d), 3, N, s, P(d_w), None, None, None, None))
    need = lib.nrf_live_points_workspace_bytes(p)
    ws = torch.empty((max(int(need), 1),), device="cuda", dtype=torch.uint8)
    fill = 123.5
    r_list = torch.full((p,), -7, device="cuda", dtype=torch.int32); r_count = torch.full((1,), -7, device="cuda", dtype=torch.int32)
    r_rows = torch.full((p, 4), fill, device="cuda")
    L.check(lib.nrf_live_points(P(d_sg), p, P(r_list), P(r_count), P(r_rows), P(ws), int(need), None))
    torch.cuda.synchronize()
    w_ref, cnt_ref, list_ref, rows_ref = host(d_w), int(host(r_count)[0]), host(r_list), host(r_rows)
    live = sg > 0
    assert cnt_ref == int(live.sum()) and np.array_equal(list_ref[:cnt_ref], np.nonzero(live.reshape(-1))[0])
    assert not live[0].any() and live[1].all() and live[7].all() and np.isnan(sg[4]).any()
    bins = dev((np.float32(0.5) * (z[:, 1:] + z[:, :-1])).astype(np.float32))
    wmid = d_w[:, 1:-1].contiguous() if s > 2 else None
    for ns in NS_ALL:
        sf = s + ns
        u_tab = dev(PR.linspace(ns))
        u_gen = torch.empty((N, ns), device="cuda")
        L.check(lib.nrf_rng_fill(SEED, L.NRF_RNG_U_PDF, RAY_BASE * ns, N * ns, 0, P(u_gen), None))
        for sum_vec in PR.SUM_VECS:
            # the stage chain with the shared table
            zf_t = torch.empty((N, sf), device="cuda"); src_t = torch.empty((N, sf), device="cuda", dtype=torch.int32); zn_t = torch.empty((N, ns), device="cuda")
            L.check(lib.nrf_fine_depths_merge(P(d_z), P(d_w), N, s, P(u_tab), ns, sum_vec, P(zf_t), P(src_t), P(zn_t), None))
            # ... and with per-ray draws: sorted depths from nrf_fine_depths_rand, the new samples from nrf_sample_pdf_rand on z_mid and weights[1:-1], and the merge
            # map from a stable sort of cat(z, z_new) (per_ray_ref.merge_sorted)
            zf_g = torch.empty((N, sf), device="cuda"); zn_g = torch.empty((N, ns), device="cuda")
            L.check(lib.nrf_fine_depths_rand(P(d_z), P(d_w), N, s, P(u_gen), ns, sum_vec, P(zf_g), None))
            L.check(lib.nrf_sample_pdf_rand(P(bins), P(wmid), N, s - 1, P(u_gen), ns, sum_vec, P(zn_g), None, None))
            torch.cuda.synchronize()
            vals, order = PR.merge_sorted(z, host(zn_g))
            src_g = np.where(order < s, np.arange(N)[:, None] * s + order, N * s + np.arange(N)[:, None] * ns + (order - s)).astype(np.int32)
            # the merge map of the ulp-swapped rows 9 and 10 is defined by rank counting (ties and order as the sort's), which a stable sort equals
            assert np.array_equal(bits(vals), bits(host(zf_g))), (s, ns, sum_vec, "the composed reference itself")
            want = {"table": (host(zf_t), host(src_t), host(zn_t)), "generated": (host(zf_g), src_g, host(zn_g))}
            for kind, (zf_w, src_w, zn_w) in want.items():
                tag = (s, ns, sum_vec, kind)
                zf = torch.full((N, sf), -1.0, device="cuda"); src = torch.full((N, sf), -1, device="cuda", dtype=torch.int32); zn = torch.full((N, ns), -1.0, device="cuda")
                w = torch.full((N, s), -1.0, device="cuda"); counts = torch.full((counts_len(N),), -7, device="cuda", dtype=torch.int32)
                lst = torch.full((p,), -7, device="cuda", dtype=torch.int32); count = torch.full((1,), -7, device="cuda", dtype=torch.int32)
                rows = torch.full((p, 4), fill, device="cuda")
                L.check(lib.nrf_dbg_resample(P(d_sg), P(d_z), P(d_d), 3, N, s, P(u_tab) if kind == "table" else None, 0, SEED, RAY_BASE, ns, sum_vec,
                                             P(zf), P(src), P(zn), P(w), P(counts), P(lst), P(count), P(rows), None))
                torch.cuda.synchronize()
                assert np.array_equal(bits(host(zf)), bits(zf_w)), (tag, "z_fine")
                assert np.array_equal(host(src), src_w), (tag, "src")
                assert np.array_equal(bits(host(zn)), bits(zn_w)), (tag, "z_new")
                assert np.array_equal(bits(host(w)), bits(w_ref)), (tag, "coarse weights")
                assert int(host(count)[0]) == cnt_ref, (tag, "count")
                assert np.array_equal(host(lst)[:cnt_ref], list_ref[:cnt_ref]), (tag, "list")
                dead = ~live.reshape(-1)
                assert np.array_equal(bits(host(rows))[dead], bits(rows_ref)[dead]), (tag, "dead rows")
                per_ray = live.sum(1).astype(np.int32)
                off = np.concatenate([[0], np.cumsum(per_ray)[:-1]]).astype(np.int32)
                assert np.array_equal(host(counts)[:N], per_ray) and np.array_equal(host(counts)[(N + 3) // 4 * 4:], off[::64]), (tag, "per-ray counts, group offsets")
            # per-ray rows of draws through the entry's u_stride equal the generated ones; without weights and the live part the depths are the same
            zf = torch.empty((N, sf), device="cuda"); src = torch.empty((N, sf), device="cuda", dtype=torch.int32); zn = torch.empty((N, ns), device="cuda")
            L.check(lib.nrf_dbg_resample(P(d_sg), P(d_z), P(d_d), 3, N, s, P(u_gen), ns, 0, 0, ns, sum_vec, P(zf), P(src), P(zn), None, None, None, None, None, None))
            torch.cuda.synchronize()
            assert np.array_equal(bits(host(zf)), bits(want["generated"][0])) and np.array_equal(host(src), src_g) and np.array_equal(bits(host(zn)), bits(want["generated"][2])), \
                (s, ns, sum_vec, "per-ray draw rows, no live part")


def test_stage_ray_stride_and_many_rays(api):
    """Directions read at the renderer's stride (11 floats, offset 3) and 70 001 rays: 1 094 groups of 64 rays, so the count scan walks its 1 024-group piece twice and ends in a partial group."""
    lib, L = api.lib, api.L
    n, s, ns = 70001, 5, 2
    rng = np.random.default_rng(31)
    z = PR._depths(rng, n, s)
    rays = rng.standard_normal((n, 11)).astype(np.float32)
    sg = rng.standard_normal((n, s)).astype(np.float32)
    d_z, d_rays, d_sg, u = dev(z), dev(rays), dev(sg), dev(PR.linspace(ns))
    d_dirs = d_rays.view(-1)[3:]
    p = n * s
    d_w = torch.empty((n, s), device="cuda")
    L.check(lib.nrf_raw2weights(P(d_sg), 1, 0, P(d_z), P(d_dirs), 11, n, s, P(d_w), None, None, None, None))
    zf_w = torch.empty((n, s + ns), device="cuda"); src_w = torch.empty((n, s + ns), device="cuda", dtype=torch.int32); zn_w = torch.empty((n, ns), device="cuda")
    L.check(lib.nrf_fine_depths_merge(P(d_z), P(d_w), n, s, P(u), ns, 8, P(zf_w), P(src_w), P(zn_w), None))
    zf = torch.empty((n, s + ns), device="cuda"); src = torch.empty((n, s + ns), device="cuda", dtype=torch.int32); zn = torch.empty((n, ns), device="cuda")
    w = torch.empty((n, s), device="cuda"); counts = torch.empty((counts_len(n),), device="cuda", dtype=torch.int32)
    lst = torch.full((p,), -7, device="cuda", dtype=torch.int32); count = torch.full((1,), -7, device="cuda", dtype=torch.int32); rows = torch.full((p, 4), 5.0, device="cuda")
    L.check(lib.nrf_dbg_resample(P(d_sg), P(d_z), P(d_dirs), 11, n, s, P(u), 0, 0, 0, ns, 8, P(zf), P(src), P(zn), P(w), P(counts), P(lst), P(count), P(rows), None))
    torch.cuda.synchronize()
    assert torch.equal(zf.view(torch.int32), zf_w.view(torch.int32)) and torch.equal(src, src_w) and torch.equal(zn.view(torch.int32), zn_w.view(torch.int32))
    assert torch.equal(w.view(torch.int32), d_w.view(torch.int32))
    ref = np.nonzero(sg.reshape(-1) > 0)[0].astype(np.int32)
    assert int(host(count)[0]) == ref.size and np.array_equal(host(lst)[:ref.size], ref)
    dead = ~(sg.reshape(-1) > 0)
    got = host(rows)
    assert (got[dead, :3] == 0).all() and np.array_equal(bits(got[:, 3])[dead], bits(sg.reshape(-1))[dead])


# ------------------------------------------------------------------ renders, switch on against off
@pytest.fixture(scope="module")
def small_scene(api):
    return api.S.make_hash_scene(mode="cu", log2_t=14, dense_budget=1 << 20)


def rays_of(api, n):
    rows = (n + 199) // 200
    o, d, _ = api.R.GetRays(200, 200, api.S.lego_K(200, 200), api.S.pose_spherical(10.0, -30.0, 4.0), row0=min(90, 200 - rows), rows=rows)
    return o.reshape(-1, 3)[:n].contiguous(), d.reshape(-1, 3)[:n].contiguous()


def render(api, sc, o, d, on, s=64, ni=128, chunk=32768, **kw):
    lib = api.lib
    before = lib.nrf_get_fused_resample()
    api.L.check(lib.nrf_set_fused_resample(int(on)))
    try:
        assert lib.nrf_get_fused_resample() == int(on)
        rp = api.S.lego_render_params(sc["bbox"], s, ni, chunk, api.L.NRF_PREC_F16_SPLIT, ReturnWeights=True, KeepIntermediates="depths", **kw)
        res = sc["renderer"].Render(0, 0, None, rp, rays=(o, d, None))
        torch.cuda.synchronize()
    finally:
        api.L.check(lib.nrf_set_fused_resample(before))
    out = dict(rgb=host(res.Outputs.RGBMap), depth=host(res.Outputs.DepthMap), disp=host(res.Outputs.DispMap), acc=host(res.Outputs.AccMap),
               weights=host(res.Outputs.Weights))
    for k in ("z_fine", "weights_coarse"):
        if k in res.Extras:
            out[k] = host(res.Extras[k])
    if res.Raw is not None:
        out["raw"] = host(res.Raw)
    return out


def equal_maps(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(bits(a[k]), bits(b[k])), f"{what}: {k} differs"


CONFIGS = {"default": dict(), "ReturnRaw": dict(ReturnRaw=True), "Perturb": dict(Perturb=1.0, Seed=11), "N_importance 0": dict(ni=0), "37 + 53": dict(s=37, ni=53)}


@pytest.mark.parametrize("n,chunk", ((300, 32768), (33000, 8192)))
@pytest.mark.parametrize("config", list(CONFIGS))
def test_render_equals_switch_off(api, small_scene, n, chunk, config):
    """RGB, depth, disparity, acc, z_fine, the weights and the coarse weights of a default split-precision HashNeRF render with the fused pair and with the stage-wise
    chain: 300 rays on one stream, 33 000 rays in five chunks on two lanes."""
    o, d = rays_of(api, n)
    kw = CONFIGS[config]
    off = render(api, small_scene, o, d, 0, chunk=chunk, **kw)
    on = render(api, small_scene, o, d, 1, chunk=chunk, **kw)
    assert np.isfinite(on["rgb"]).all() and (on["weights"] > 0).any() and (on["weights"] == 0).any()
    if kw.get("ni", 1):
        assert "z_fine" in on and "weights_coarse" in on
    equal_maps(on, off, f"{config}, n {n}")


@pytest.mark.parametrize("n", (1, 2, 5))
def test_render_one_new_sample(api, small_scene, n):
    """64 + 1 samples on one, two and five rays: one ray's single new sample leaves no room for the per-ray counts behind the coarse columns' rows, so that chunk
    counts by launch; from two rays on the masks are used.  Equal to the switch off either way."""
    o, d = rays_of(api, n)
    equal_maps(render(api, small_scene, o, d, 1, ni=1), render(api, small_scene, o, d, 0, ni=1), f"64 + 1, n {n}")


def test_ten_identical_frames(api, small_scene):
    """Ten renders with the switch on (two lanes, five chunks): every frame equals the first."""
    o, d = rays_of(api, 33000)
    first = render(api, small_scene, o, d, 1, chunk=8192)
    for i in range(9):
        equal_maps(render(api, small_scene, o, d, 1, chunk=8192), first, f"frame {i + 1}")
