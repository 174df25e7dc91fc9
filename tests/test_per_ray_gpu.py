"""GPU tests of the one-wave-per-ray kernels (composite.hip: k_raw2outputs, k_sample_pdf, k_fine_depths, aten_row_sum; train.hip: k_raw2outputs_bwd; rays.hip: k_z_vals) at
every sample count the library accepts: both sides of each 64-sample block edge, partial last blocks, single samples, 512 merged samples.  The cases are
tests/per_ray_ref.py's; the yardstick is the C oracle, bit for bit, which tests/test_per_ray_host.py pins against ATen and against the float64 restatements on the same
cases -- so the float64 bars recorded there hold for the kernels too.  Every GPU step runs once."""
import copy

import numpy as np
import pytest
import torch

from conftest import load_golden
from nerfpp_amd import synth
from oracle import capi as O
import per_ray_ref as PR

pytestmark = pytest.mark.gpu

NAN = float("nan")
P = lambda t: None if t is None else t.data_ptr()
host = lambda t: t.detach().cpu().numpy()
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
nans = lambda *shape: torch.full(shape, NAN, device="cuda")


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from types import SimpleNamespace
    from nerfpp_amd import _lib as L, modules as M, renderer as R, scene as S
    return SimpleNamespace(L=L, M=M, R=R, S=S, lib=L.lib())


def dev(a, dtype=np.float32, misalign=False):
    """-> the array on the device; misalign: a view one float into a larger buffer (4 bytes past a 16-byte boundary)"""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype))
    if not misalign:
        return t.cuda()
    v = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def same(got, want, what):
    got, want = np.asarray(host(got) if torch.is_tensor(got) else got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((bits(got) if got.dtype == np.float32 else got).reshape(-1) != (bits(want) if want.dtype == np.float32 else want).reshape(-1))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[:5]}: {got.reshape(-1)[bad[:3]]} vs {want.reshape(-1)[bad[:3]]}"


def dirs_on_device(c):
    """-> (pointer to ray 0's direction, stride): compact [n,3], or columns 3:6 of an [n,11] ray batch whose other columns are NaN"""
    if c["d_stride"] == 3:
        t = dev(c["d"])
        return t, t.data_ptr(), 3
    rays = np.full((c["n"], c["d_stride"]), np.nan, np.float32)
    rays[:, 3:6] = c["d"]
    t = dev(rays)
    return t, t.data_ptr() + 12, c["d_stride"]


# ------------------------------------------------------------------ (a) bit for bit against the oracle
@pytest.mark.parametrize("spec", PR.z_vals_specs(), ids=lambda sp: f"n{sp[1]}-s{sp[2]}-stride{sp[3]}-lindisp{int(sp[4])}")
def test_z_vals(api, spec):
    c = PR.z_vals_case(*spec)
    rays, t, z = dev(c["rays"]), dev(c["t"]), nans(c["n"], c["s"])
    api.L.check(api.lib.nrf_z_vals(P(rays), c["stride"], c["n"], P(t), c["s"], int(c["lindisp"]), P(z), None))
    same(z, O.z_vals(c["rays"][:, 6], c["rays"][:, 7], c["t"], c["lindisp"]), c["tag"])


def composite_call(api, c, raw, z, dptr, stride, want, noise=None, noise_std=0.0):
    """nrf_raw2outputs (noise None) or nrf_raw2outputs_noise with the outputs named in want, NaN-prefilled -> dict of host arrays"""
    n, s = c["n"], c["s"]
    out = {k: nans(*sh) for k, sh in (("rgb", (n, 3)), ("disp", (n,)), ("acc", (n,)), ("weights", (n, s)), ("depth", (n,))) if k in want}
    o = lambda k: P(out.get(k))
    if noise is None:
        api.L.check(api.lib.nrf_raw2outputs(P(raw), P(z), dptr, stride, n, s, c["c"], int(c["white"]), o("rgb"), o("disp"), o("acc"), o("weights"), o("depth"), None))
    else:
        nz = dev(noise)
        api.L.check(api.lib.nrf_raw2outputs_noise(P(raw), P(z), dptr, stride, n, s, c["c"], int(c["white"]), P(nz), noise_std, o("rgb"), o("disp"), o("acc"), o("weights"),
                                                  o("depth"), None))
    torch.cuda.synchronize()
    return {k: host(v) for k, v in out.items()}


def weights_call(api, c, raw, sigma_ch, z, dptr, stride, want, src=None):
    n, s = c["n"], c["s"]
    out = {k: nans(*sh) for k, sh in (("weights", (n, s)), ("depth", (n,)), ("disp", (n,)), ("acc", (n,))) if k in want}
    o = lambda k: P(out.get(k))
    if src is None:
        api.L.check(api.lib.nrf_raw2weights(P(raw), c["c"], sigma_ch, P(z), dptr, stride, n, s, o("weights"), o("depth"), o("disp"), o("acc"), None))
    else:
        api.L.check(api.lib.nrf_raw2weights_gather(P(raw), c["c"], sigma_ch, P(src), P(z), dptr, stride, n, s, o("weights"), o("depth"), o("disp"), o("acc"), None))
    torch.cuda.synchronize()
    return {k: host(v) for k, v in out.items()}


@pytest.mark.parametrize("spec", PR.composite_specs(), ids=lambda sp: f"{sp[4]}-n{sp[1]}-s{sp[2]}-c{sp[3]}")
def test_compositing_entries(api, spec):
    """nrf_raw2outputs on every case, nrf_raw2outputs_noise on every case with draws (all but zero_sigma), nrf_raw2weights (sigma_ch 0 and c - 1) and nrf_raw2weights_gather (rows shuffled by a random permutation per ray, read back through the map):
    every output equals the oracle's bit for bit; with only the weights or only the maps asked for (NULL for the rest) the same bits come back."""
    c = PR.composite_case(*spec)
    n, s, ch = c["n"], c["s"], c["c"]
    raw, z = dev(c["raw"], misalign=c["misalign"]), dev(c["z"])
    keep, dptr, stride = dirs_on_device(c)
    for noise, std in PR.noise_modes(c):
        name = "nrf_raw2outputs" if noise is None else "nrf_raw2outputs_noise"
        ref = O.raw2outputs(c["raw"], c["z"], c["d"], c["white"]) if noise is None else O.raw2outputs_noise(c["raw"], c["z"], c["d"], noise, std, c["white"])
        for want in (("rgb", "disp", "acc", "weights", "depth"), ("weights",), ("rgb", "disp", "acc", "depth")):
            got = composite_call(api, c, raw, z, dptr, stride, want, noise, std)
            for k in want:
                same(got[k], ref[k], f"{c['tag']}: {name} {k} with outputs {want}")
    rng = np.random.default_rng(c["seed"] + 1)
    perm = np.argsort(rng.random((n, s)), axis=1)
    src = (np.arange(n)[:, None] * s + perm).astype(np.int32)                  # sample (ray, j) reads row src[ray, j]
    shuffled = np.empty((n * s, ch), np.float32)
    shuffled[src.reshape(-1)] = c["raw"].reshape(n * s, ch)
    d_src, d_shuffled = dev(src, np.int32), dev(shuffled, misalign=c["misalign"])
    for sigma_ch in sorted({0, ch - 1}):
        refw = O.raw2weights(c["raw"], sigma_ch, c["z"], c["d"])
        for want in (("weights", "depth", "disp", "acc"), ("weights",), ("depth", "disp", "acc")):
            got = weights_call(api, c, raw, sigma_ch, z, dptr, stride, want)
            for k in want:
                same(got[k], refw[k], f"{c['tag']}: nrf_raw2weights sigma_ch {sigma_ch} {k} with outputs {want}")
        got = weights_call(api, c, d_shuffled, sigma_ch, z, dptr, stride, ("weights", "depth", "disp", "acc"), src=d_src)
        for k, v in got.items():
            same(v, refw[k], f"{c['tag']}: nrf_raw2weights_gather sigma_ch {sigma_ch} {k}")
        got = weights_call(api, c, d_shuffled, sigma_ch, z, dptr, stride, ("weights",), src=d_src)
        same(got["weights"], refw["weights"], f"{c['tag']}: nrf_raw2weights_gather sigma_ch {sigma_ch}, weights only")


def pdf_call(api, c, fn, u, sum_vec, with_inds=True):
    n, nb, ns = c["n"], c["nb"], c["ns"]
    bins, w, du = dev(c["bins"]), dev(c["weights"]), dev(u)
    smp = nans(n, ns)
    inds = torch.full((n, ns), -1, dtype=torch.int64, device="cuda") if with_inds else None
    api.L.check(fn(P(bins), P(w), n, nb, P(du), ns, sum_vec, P(smp), P(inds), None))
    torch.cuda.synchronize()
    return host(smp), None if inds is None else host(inds)


@pytest.mark.parametrize("nb", PR.PDF_NB)
def test_sample_pdf_entries(api, nb):
    """nrf_sample_pdf (shared linspace draws, u = 0 and u = 1 among them) and nrf_sample_pdf_rand (a row of draws per ray) at sum_vec 0, 4, 8, 16 and every draw count:
    samples and indices equal the oracle's bit for bit; without the index output (NULL) the samples are the same."""
    for spec in [sp for sp in PR.pdf_specs() if sp[2] == nb]:
        c = PR.pdf_case(*spec)
        for name, u, orc in (("nrf_sample_pdf", c["u"], O.sample_pdf), ("nrf_sample_pdf_rand", c["u_rand"], O.sample_pdf_rand)):
            for sum_vec in PR.SUM_VECS:
                ref = orc(c["bins"], c["weights"], u, sum_vec)
                smp, inds = pdf_call(api, c, getattr(api.lib, name), u, sum_vec)
                same(inds, ref[1], f"{c['tag']}: {name} sum_vec {sum_vec} indices")
                same(smp, ref[0], f"{c['tag']}: {name} sum_vec {sum_vec} samples")
            smp, _ = pdf_call(api, c, getattr(api.lib, name), u, 8, with_inds=False)
            same(smp, orc(c["bins"], c["weights"], u, 8)[0], f"{c['tag']}: {name} without indices")


def fine_call(api, c, name, u, sum_vec):
    """-> (z_fine, src | None, z_new | None)"""
    n, s, ns = c["n"], c["s"], c["ns"]
    z, w, du = dev(c["z"]), dev(c["weights"]), dev(u)
    zf = nans(n, s + ns)
    if name == "nrf_fine_depths_merge":
        src, zn = torch.full((n, s + ns), -1, dtype=torch.int32, device="cuda"), nans(n, ns)
        api.L.check(api.lib.nrf_fine_depths_merge(P(z), P(w), n, s, P(du), ns, sum_vec, P(zf), P(src), P(zn), None))
        torch.cuda.synchronize()
        return host(zf), host(src), host(zn)
    api.L.check(getattr(api.lib, name)(P(z), P(w), n, s, P(du), ns, sum_vec, P(zf), None))
    torch.cuda.synchronize()
    return host(zf), None, None


@pytest.mark.parametrize("spec", PR.fine_specs(), ids=lambda sp: f"n{sp[1]}-s{sp[2]}-ns{sp[3]}")
def test_fine_depth_entries(api, spec):
    """nrf_fine_depths, nrf_fine_depths_rand and nrf_fine_depths_merge at sum_vec 0, 4, 8, 16: z_fine equals the oracle's z_mid -> SamplePDF(weights[1:-1]) -> sort(cat)
    bit for bit.  The merge map's properties: each ray's src row is a permutation of its s coarse and its ns new column ids; decoding src through cat(z, z_new) gives
    z_fine exactly; z_new equals nrf_sample_pdf's samples on the same bins and weights; z_fine does not decrease; equal depths keep the order of cat(z, samples), so
    on a tie the coarse depth comes first."""
    c = PR.fine_case(*spec)
    n, s, ns = c["n"], c["s"], c["ns"]
    mid, wmid = O.z_mid(c["z"]), np.ascontiguousarray(c["weights"][:, 1:-1])
    for sum_vec in PR.SUM_VECS:
        smp = O.sample_pdf(mid, wmid, c["u"], sum_vec)[0]
        want = O.merge_sorted(c["z"], smp)
        same(fine_call(api, c, "nrf_fine_depths", c["u"], sum_vec)[0], want, f"{c['tag']}: nrf_fine_depths sum_vec {sum_vec}")
        smp_r = O.sample_pdf_rand(mid, wmid, c["u_rand"], sum_vec)[0]
        same(fine_call(api, c, "nrf_fine_depths_rand", c["u_rand"], sum_vec)[0], O.merge_sorted(c["z"], smp_r), f"{c['tag']}: nrf_fine_depths_rand sum_vec {sum_vec}")
        zf, src, zn = fine_call(api, c, "nrf_fine_depths_merge", c["u"], sum_vec)
        same(zf, want, f"{c['tag']}: nrf_fine_depths_merge sum_vec {sum_vec}")
        same(zn, smp, f"{c['tag']}: z_new == the oracle's samples")
        if s >= 3:          # (one bin edge has no weight: nrf_sample_pdf wants a weight pointer only from two edges on)
            pc = dict(bins=mid, weights=wmid, n=n, nb=s - 1, ns=ns)
            same(zn, pdf_call(api, pc, api.lib.nrf_sample_pdf, c["u"], sum_vec, with_inds=False)[0], f"{c['tag']}: z_new == nrf_sample_pdf's samples")
        ray = np.arange(n)[:, None]
        ids = np.concatenate([ray * s + np.arange(s), n * s + ray * ns + np.arange(ns)], 1)          # the column ids of cat(z, z_new), per ray
        assert np.array_equal(np.sort(src, axis=1), np.sort(ids, axis=1)), f"{c['tag']}: src rows are permutations of the ray's column ids"
        table = np.concatenate([c["z"].reshape(-1), zn.reshape(-1)])
        same(table[src], zf, f"{c['tag']}: cat(z, z_new)[src] == z_fine")
        assert (np.diff(zf, axis=1) >= 0).all(), f"{c['tag']}: z_fine does not decrease"
        tie = zf[:, 1:] == zf[:, :-1]
        assert (src[:, 1:] > src[:, :-1])[tie].all(), f"{c['tag']}: ties keep the order of cat(z, samples): coarse depths first"
        _, order = PR.merge_sorted(c["z"], zn)
        assert np.array_equal(src, np.take_along_axis(ids, order, 1)), f"{c['tag']}: src == the stable sort's order"
        if s <= 3 and n >= 3:
            assert tie[0].all(), f"{c['tag']}: the tie rows tie at sum_vec {sum_vec}"


# ------------------------------------------------------------------ (c) the backward
@pytest.mark.parametrize("spec", PR.composite_specs(), ids=lambda sp: f"{sp[4]}-n{sp[1]}-s{sp[2]}-c{sp[3]}")
def test_raw2outputs_backward(api, spec):
    """nrf_raw2outputs_backward on every case and nrf_raw2outputs_backward_noise on every case with draws (all but zero_sigma) against the oracle at test_raw2outputs_backward_with_noise_vs_oracle's bar: rtol
    1e-5, atol 1e-7 of the largest entry; columns 4.. exactly zero; nothing left at the NaN prefill."""
    c = PR.composite_case(*spec)
    n, s, ch = c["n"], c["s"], c["c"]
    raw, z, g_rgb = dev(c["raw"], misalign=c["misalign"]), dev(c["z"]), dev(c["g_rgb"])
    keep, dptr, stride = dirs_on_device(c)
    for noise, std in PR.noise_modes(c):
        out = nans(n, s, ch)
        if noise is None:
            name = "nrf_raw2outputs_backward"
            api.L.check(api.lib.nrf_raw2outputs_backward(P(raw), P(z), dptr, stride, n, s, ch, int(c["white"]), P(g_rgb), P(out), None))
            ref = O.raw2outputs_backward(c["raw"], c["z"], c["d"], c["g_rgb"], c["white"])
        else:
            name, nz = "nrf_raw2outputs_backward_noise", dev(noise)
            api.L.check(api.lib.nrf_raw2outputs_backward_noise(P(raw), P(z), dptr, stride, n, s, ch, int(c["white"]), P(nz), std, P(g_rgb), P(out), None))
            ref = O.raw2outputs_backward_noise(c["raw"], c["z"], c["d"], c["g_rgb"], noise, std, c["white"])
        torch.cuda.synchronize()
        got = host(out)
        assert not np.isnan(got).any(), (c["tag"], name)
        assert not got[..., 4:].any(), (c["tag"], name)
        err = np.abs(got.astype(np.float64) - ref)
        print(f"{c['tag']} {name}: max |got - oracle| = {err.max():.3e}, max |oracle| = {np.abs(ref).max():.3e}")
        np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-7 * np.abs(ref).max(), err_msg=f"{c['tag']} {name}")


# ------------------------------------------------------------------ (d) the FAST compositing kernel, through the renderer
FAST_COUNTS = ((37, 53), (64, 128), (128, 128), (129, 128), (64, 256), (255, 256), (256, 256))          # merged 90, 192, 256 | 257, 320, 511, 512: both branches, the 256 edge


@pytest.fixture(scope="module")
def fast_scene(api):
    sc = api.S.make_hash_scene(mode="cu", log2_t=14)
    o, d, _ = api.R.GetRays(64, 64, api.S.lego_K(64, 64), api.S.pose_spherical(10.0, -30.0, 4.0))
    pick = slice(64 * 27, 64 * 27 + 301)          # 301 rays across the middle rows: a partial last block of four
    return sc, o.reshape(-1, 3)[pick].contiguous(), d.reshape(-1, 3)[pick].contiguous()


def maps_of(res):
    return {k: host(getattr(res.Outputs, k)) for k in ("RGBMap", "AccMap", "DepthMap", "DispMap", "Weights")}


@pytest.mark.parametrize("s,ni", FAST_COUNTS)
def test_fast_compositing_through_the_renderer(api, fast_scene, s, ni):
    """k_raw2outputs<FAST> (fp32 scan, hardware exp / log / rcp; the prefetch branch up to 256 merged samples, the block-by-block branch above) as NRF_PREC_F16_SPLIT
    renders use it: the returned Raw, z_fine and directions composited in float64 -> RGBMap and AccMap within 1e-4 (the pixel bar, BASELINE.json north_star), Weights
    within 2e-5 (the bar test_edge_cases_empty_ragged_and_limits holds split weights to); the same Raw through the exact nrf_raw2outputs -> DepthMap and DispMap within
    rtol 1e-4 on rays with acc >= 0.1.  A second render without ReturnRaw composites through the merge map: identical maps."""
    sc, o, d = fast_scene
    rp = api.S.lego_render_params(sc["bbox"], n_samples=s, n_importance=ni, precision=api.L.NRF_PREC_F16_SPLIT, ReturnRaw=True, ReturnWeights=True, KeepIntermediates="depths")
    res = sc["renderer"].Render(0, 0, None, rp, rays=(o, d, None))
    got = maps_of(res)
    n, sf = o.shape[0], s + ni
    raw, zf, dirs = host(res.Raw).reshape(n, sf, -1), host(res.Extras["z_fine"]), host(res.Extras["rays_flat"][:, 3:6])
    assert zf.shape == (n, sf) and raw.shape[-1] == 4 and got["Weights"].shape == (n, sf)
    ref = {k: v.numpy() for k, v in PR.raw2outputs(raw, zf, dirs, white=True).items() if k != "raw"}
    for k, r, bar in (("RGBMap", "rgb", 1e-4), ("AccMap", "acc", 1e-4), ("Weights", "weights", 2e-5)):
        err = np.abs(got[k].reshape(ref[r].shape) - ref[r]).max()
        print(f"{s} + {ni}: {k} max |FAST - float64| = {err:.3e} (bar {bar})")
        assert err <= bar, (k, err)
    exact = O.raw2outputs(raw, zf, dirs, True)
    c = dict(n=n, s=sf, c=4, white=True, noise=None)
    d_raw, d_zf, d_dirs = dev(raw), dev(zf), dev(dirs)
    on_gpu = composite_call(api, c, d_raw, d_zf, d_dirs.data_ptr(), 3, ("rgb", "disp", "acc", "weights", "depth"))
    for k in on_gpu:
        same(on_gpu[k], exact[k], f"{s} + {ni}: nrf_raw2outputs on the render's Raw == oracle, {k}")
    keep = on_gpu["acc"] >= 0.1
    assert keep.mean() > 0.5, keep.mean()
    for k, r in (("DepthMap", "depth"), ("DispMap", "disp")):
        rel = np.abs(got[k].reshape(-1)[keep] - on_gpu[r][keep]) / np.abs(on_gpu[r][keep])
        print(f"{s} + {ni}: {k} max relative |FAST - exact| = {rel.max():.3e} over {keep.sum()} rays (bar 1e-4)")
        assert rel.max() <= 1e-4, (k, rel.max())
    rp_n = copy.copy(rp)
    rp_n.ReturnRaw = False
    again = maps_of(sc["renderer"].Render(0, 0, None, rp_n, rays=(o, d, None)))
    for k in got:
        same(again[k], got[k], f"{s} + {ni}: {k}, merge-map read == gathered rows")


@pytest.mark.parametrize("s,ni", [(64, 256), (129, 128)])
def test_fast_compositing_two_array_read(api, fast_scene, s, ni):
    """NRF_COARSE_FULL keeps the coarse pass's network outputs: without ReturnRaw the compositing kernel reads raw | raw2 through the merge map, with it the gathered rows --
    identical maps above 256 merged samples (the block-by-block branch) too."""
    sc, o, d = fast_scene
    outs = []
    for ret in (True, False):
        rp = api.S.lego_render_params(sc["bbox"], n_samples=s, n_importance=ni, precision=api.L.NRF_PREC_F16_SPLIT, ReturnRaw=ret, ReturnWeights=True,
                                      CoarseMode=api.L.NRF_COARSE_FULL)
        outs.append(maps_of(sc["renderer"].Render(0, 0, None, rp, rays=(o, d, None))))
    for k in outs[0]:
        assert np.isfinite(outs[0][k]).all()
        same(outs[1][k], outs[0][k], f"{s} + {ni} NRF_COARSE_FULL: {k}")


# ------------------------------------------------------------------ (e) NRF_PREC_F32 end to end at ragged counts
@pytest.fixture(scope="module")
def golden_scene(api, manifest):
    """The scene and oracle model of test_render_hash_vs_reference"""
    g = load_golden("render_hash")
    ent = manifest["render_hash"]
    table = synth.blob_from_manifest([x for x in ent if "embeddings" in x[0]])
    blob = synth.blob_from_manifest([x for x in ent if "embeddings" not in x[0]])
    e = api.M.HashEmbedder("embedder", g["bbox"], 16, 2, 19, 16, 512)
    e.set_table(table)
    m = api.M.NeRFSmall(3, 64, 15, 4, 64, False, 3, 64, 32, 16, "model", params=blob)
    return g, api.R.NeRFRenderer(e, api.M.SHEncoder("embeddirs", 3, 4), m), O.Model(0, blob, bbox=g["bbox"], table_f32=table)


@pytest.mark.parametrize("s,ni", [(37, 53), (65, 5), (129, 128), (256, 256)])
def test_f32_render_equals_the_oracle_at_ragged_counts(api, golden_scene, s, ni):
    """DESIGN section 2's claim away from 64 + 128: the NRF_PREC_F32 render of the golden hash scene (8 x 8 rays) equals orc_render_rays bit for bit -- RGB, depth, acc,
    weights and the fine sample set.  (The oracle's render_rays accepts every one of these counts.)"""
    g, r, model = golden_scene
    rp = api.R.NeRFRenderParams(NSamples=s, NImportance=ni, Chunk=64, ReturnRaw=True, LinDisp=False, Perturb=0.0, WhiteBkgr=True, RawNoiseStd=0.0, Ndc=False, UseViewdirs=True,
                                ReturnWeights=True, ThinRay=True, BoundingBox=g["bbox"], KeepIntermediates=True)
    res = r.Render(8, 8, g["k"], rp, c2w=g["c2w"])
    rays = host(res.Extras["rays_flat"])
    oc = O.render_rays(model, rays, s, ni, O.linspace(0, 1, s), O.linspace(0, 1, ni), white_bkgr=True, want_intermediates=True)
    same(res.Extras["z_coarse"], oc["z_coarse"], f"{s} + {ni}: z_coarse")
    same(res.Extras["weights_coarse"], oc["weights_coarse"], f"{s} + {ni}: coarse weights")
    same(res.Extras["z_fine"], oc["z_fine"], f"{s} + {ni}: z_fine")
    same(host(res.Outputs.Weights).reshape(64, s + ni), oc["weights"], f"{s} + {ni}: weights")
    same(host(res.Outputs.RGBMap).reshape(-1, 3), oc["rgb"], f"{s} + {ni}: RGB")
    same(host(res.Outputs.DepthMap).reshape(-1), oc["depth"], f"{s} + {ni}: depth")
    same(host(res.Outputs.AccMap).reshape(-1), oc["acc"], f"{s} + {ni}: acc")
    assert oc["acc"].max() > 0.05 and (np.diff(oc["z_fine"], axis=1) >= 0).all()


# ------------------------------------------------------------------ (f) limits are answered, not run
def test_limits_are_refused(api):
    """Counts outside the built range and a sum_vec other than 0, 4, 8, 16 come back as errors that name the limit; the output buffers keep their prefill (argument checks:
    nothing is launched)."""
    z, w, u = torch.zeros((4, 257), device="cuda"), torch.ones((4, 257), device="cuda"), torch.zeros((4, 513), device="cuda")
    zf, smp = nans(4, 514), nans(4, 513)
    inds = torch.full((4, 513), -1, dtype=torch.int64, device="cuda")
    src = torch.full((4, 514), -1, dtype=torch.int32, device="cuda")

    def refused(rc, match):
        assert rc != api.L.NRF_OK
        with pytest.raises(api.L.NrfError, match=match):
            api.L.check(rc)
        torch.cuda.synchronize()
        assert bool(torch.isnan(zf).all()) and bool(torch.isnan(smp).all()) and bool((inds == -1).all()) and bool((src == -1).all()), "a refused call writes nothing"

    for s, ns in ((1, 64), (257, 64), (64, 257)):
        refused(api.lib.nrf_fine_depths(P(z), P(w), 4, s, P(u), ns, 8, P(zf), None), "outside the built range")
        refused(api.lib.nrf_fine_depths_rand(P(z), P(w), 4, s, P(u), ns, 8, P(zf), None), "outside the built range")
        refused(api.lib.nrf_fine_depths_merge(P(z), P(w), 4, s, P(u), ns, 8, P(zf), P(src), P(smp), None), "outside the built range")
    for nb, ns in ((257, 64), (64, 513)):
        refused(api.lib.nrf_sample_pdf(P(z), P(w), 4, nb, P(u), ns, 8, P(smp), P(inds), None), "outside the built range")
        refused(api.lib.nrf_sample_pdf_rand(P(z), P(w), 4, nb, P(u), ns, 8, P(smp), P(inds), None), "outside the built range")
    refused(api.lib.nrf_sample_pdf(P(z), P(w), 4, 64, P(u), 64, 5, P(smp), P(inds), None), "sum_vec must be 0, 4, 8 or 16")
    refused(api.lib.nrf_fine_depths(P(z), P(w), 4, 64, P(u), 64, 5, P(zf), None), "sum_vec must be 0, 4, 8 or 16")
    api.L.check(api.lib.nrf_fine_depths(P(z), P(w), 4, 64, P(u), 64, 8, P(zf), None))          # a valid call right afterwards
    torch.cuda.synchronize()
    assert not bool(torch.isnan(zf.view(-1)[:4 * 128]).any())
