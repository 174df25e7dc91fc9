"""Density normals on the MI355X: nrf_density_grad against RunNetwork(F32) (sigma, bit for bit) and the float64 restatement (tests/normals_ref.py), a known-answer
field, RenderedNormals / RenderedPredNormals against float64 compositions of the render's own weights, bit-identity of every other output, determinism, the
unsupported renderers, and ExtractMesh(normals="field")."""
import ctypes as C

import numpy as np
import pytest
import torch

from normals_ref import SigmaRef

pytestmark = pytest.mark.gpu

PRECS = ("F32", "F16_SPLIT", "F16_MFMA")


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from nerfpp_amd import _lib as L, mesh, renderer, scene
    return L, mesh, renderer, scene


_SCENES = {}


def _scene(scene, kind):
    if kind not in _SCENES:
        _SCENES[kind] = scene.make_hash_scene(mode=kind)
    return _SCENES[kind]


def _prec(L, name):
    return getattr(L, "NRF_PREC_" + name)


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.uint32)


def _run_network_sigma(sc, pts):
    p = torch.from_numpy(np.ascontiguousarray(pts, np.float32).reshape(-1, 1, 3)).cuda()
    vd = torch.zeros((p.shape[0], 3), device="cuda", dtype=torch.float32)
    return sc["renderer"].RunNetwork(p, vd)[:, 0, 3]


def _test_points(n, seed):
    rng = np.random.default_rng(seed)
    inside = rng.uniform(-1.5, 1.5, (n, 3))
    outside = rng.uniform(-2.0, 2.0, (n, 3))
    faces = rng.uniform(-1.5, 1.5, (n, 3))
    faces[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-1.5, 1.5], n)
    return np.concatenate([inside, outside, faces]).astype(np.float32)


@pytest.mark.parametrize("mode", ["cu", "ngp"])
def test_sigma_equals_run_network_f32(api, mode):
    L, mesh, R, scene = api
    sc = _scene(scene, mode)
    pts = _test_points(4096, 1)
    sig, grad = mesh.DensityGradient(sc["renderer"], torch.from_numpy(pts).cuda())
    ref = _run_network_sigma(sc, pts)
    assert (_bits(sig) == _bits(ref)).all()
    g = grad.cpu().numpy()
    assert np.isfinite(g).all()
    outside = (np.abs(pts) > 1.5).any(1)
    assert outside.any() and (g[outside] == 0).all()          # the keep mask: sigma = 0 there, and its gradient with it


@pytest.mark.parametrize("mode", ["cu", "ngp"])
def test_gradient_matches_float64_restatement(api, mode):
    L, mesh, R, scene = api
    sc = _scene(scene, mode)
    pts = np.random.default_rng(7).uniform(-1.5, 1.5, (1 << 16, 3)).astype(np.float32)
    _, g = mesh.DensityGradient(sc["renderer"], torch.from_numpy(pts).cuda())
    g = g.cpu().numpy().astype(np.float64)
    _, gr, kink = SigmaRef(sc).grad(pts)
    gn = np.linalg.norm(gr, axis=1)
    sel = gn > 1e-3 * np.median(gn)
    near = kink < 1e-5                     # a pre-activation within fp32 rounding of 0: the masks may legitimately differ
    use = sel & ~near
    print(f"{mode}: {int((sel & near).sum())} of {int(sel.sum())} points excluded near a ReLU kink")
    assert use.sum() > 0.95 * sel.sum()
    err = np.linalg.norm(g[use] - gr[use], axis=1)
    assert (err <= 1e-4 * gn[use]).all(), float(np.max(err / gn[use]))


def test_known_answer_affine_level0(api):
    L, mesh, R, scene = api
    from nerfpp_amd.modules import CuHashEmbedder, CuSHEncoder, NeRFSmall
    nl, F, T = 16, 2, 19
    bbox = scene.LEGO_BBOX
    emb = CuHashEmbedder("embedder", bbox, nl, F, T, 16, 512)
    primes = np.array(scene.CU_PRIMES[:3 * nl], np.int32)
    emb.set_primes(primes)
    out = (C.c_float * nl)()
    L.check(L.lib().nrf_hash_get_level_scales(emb._h, out))
    mul = np.float32(out[0])
    alpha, beta = np.array([0.25, 0.5, -0.125]), 8.0
    # a 4 x 4 x 4 block of level-0 cells: its 5^3 corners must land on distinct rows (collision-free)
    c0 = np.array([6, 7, 5])
    table = np.zeros((nl << T) * F, np.float32)
    used = {}
    for cx in range(c0[0], c0[0] + 5):
        for cy in range(c0[1], c0[1] + 5):
            for cz in range(c0[2], c0[2] + 5):
                e = ((cx * int(primes[0])) ^ (cy * int(primes[1])) ^ (cz * int(primes[2]))) & 0xFFFFFFFF & ((1 << T) - 1)
                assert e not in used
                used[e] = 1
                table[e * F] = alpha @ np.array([cx, cy, cz]) + beta          # exact in fp16: multiples of 1/8 below 32
    emb.set_table(table)
    # sigma net: sigma = relu(relu(feature 0)) (features stay positive here)
    shapes = scene.small_shapes(32, 16, 3, 64, 15, 4, 64)
    parts = []
    for name, o, i, _ in shapes:
        w = np.zeros((o, i), np.float32)
        if name.startswith("model_sigma_net"):
            w[0, 0] = 1.0
        parts.append(w.reshape(-1))
    mlp = NeRFSmall(3, 64, 15, 4, 64, False, 3, 64, 32, 16, "model", params=np.concatenate(parts))
    r = R.NeRFRenderer(emb, CuSHEncoder("embeddirs", 3, 4), mlp)
    ext = np.float32(bbox[3] - bbox[0])
    rng = np.random.default_rng(3)
    q = c0 + 0.02 + rng.uniform(0, 3.96, (4096, 3))                          # level-0 coordinates inside the block
    pts = (q / np.float64(mul) * np.float64(ext) + np.float64(bbox[0])).astype(np.float32)
    sig, g = mesh.DensityGradient(r, torch.from_numpy(pts).cuda())
    want = alpha * np.float64(np.float32(mul / ext))
    g = g.cpu().numpy().astype(np.float64)
    assert np.allclose(g, want[None, :], rtol=1e-6, atol=0), np.abs(g - want).max()
    assert (sig.cpu().numpy() > 0).all()


def _camera(scene, h=800, w=800):
    return scene.lego_K(h, w), scene.pose_spherical(30.0, -30.0, 4.0)


def _render(R, sc, scene, L, prec, h, w, normals=True, rows=None, row0=0, chunk=32768, lanes=None, **kw):
    K, c2w = _camera(scene, h, w)
    if lanes is not None:
        L.check(L.lib().nrf_renderer_set_lanes(sc["renderer"]._r, int(lanes)))
    p = scene.lego_render_params(precision=_prec(L, prec), chunk=chunk, CalculateNormals=normals, **kw)
    try:
        return sc["renderer"].Render(h, w, K, p, c2w=c2w, row0=row0, rows=rows)
    finally:
        if lanes is not None:
            L.check(L.lib().nrf_renderer_set_lanes(sc["renderer"]._r, 0))


@pytest.mark.parametrize("prec", PRECS)
def test_rendered_normals_match_float64_composition(api, prec):
    L, mesh, R, scene = api
    sc = _scene(scene, "cu")
    res = _render(R, sc, scene, L, prec, 800, 800, ReturnWeights=True, KeepIntermediates="depths")
    w = res.Outputs.Weights
    z = res.Extras["z_fine"]
    rays = res.Extras["rays_flat"]
    o, d = rays[:, None, 0:3], rays[:, None, 3:6]
    pts = o + d * z[..., None]                        # o + d z as the encoders form it: one rounding per operation
    _, g = mesh.DensityGradient(sc["renderer"], pts)
    g = g.double()
    nrm = -g / torch.linalg.vector_norm(g, dim=-1, keepdim=True).clamp_min(1e-8)
    ref = (w.double()[..., None] * nrm).sum(1)
    got = res.Outputs.RenderedNormals.reshape(-1, 3).double()
    assert res.Outputs.RenderedNormals.shape == res.Outputs.RGBMap.shape
    err = (got - ref).abs().max().item()
    assert err <= 2e-6, err
    del pts, g, nrm


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("lanes", [1, 2])
def test_other_outputs_unchanged_by_normals(api, prec, lanes):
    L, mesh, R, scene = api
    sc = _scene(scene, "cu")
    kw = dict(ReturnWeights=True, chunk=8192, lanes=lanes)
    a = _render(R, sc, scene, L, prec, 200, 200, normals=False, **kw)
    b = _render(R, sc, scene, L, prec, 200, 200, normals=True, **kw)
    assert a.Outputs.RenderedNormals is None and b.Outputs.RenderedNormals is not None
    for k in ("RGBMap", "DispMap", "AccMap", "DepthMap", "Weights"):
        assert (_bits(getattr(a.Outputs, k)) == _bits(getattr(b.Outputs, k))).all(), k
    # the ray-batch branch (nrf_batchify_rays)
    K, c2w = _camera(scene, 200, 200)
    ro, rd, _ = R.GetRays(200, 200, K, c2w)
    for on in (False, True):
        p = scene.lego_render_params(precision=_prec(L, prec), chunk=8192, ReturnWeights=True, CalculateNormals=on)
        L.check(L.lib().nrf_renderer_set_lanes(sc["renderer"]._r, lanes))
        try:
            r = sc["renderer"].Render(200, 200, K, p, rays=(ro, rd, None))
        finally:
            L.check(L.lib().nrf_renderer_set_lanes(sc["renderer"]._r, 0))
        if not on:
            ref = r
            continue
        for k in ("RGBMap", "DispMap", "AccMap", "DepthMap", "Weights"):
            assert (_bits(getattr(ref.Outputs, k)) == _bits(getattr(r.Outputs, k))).all(), k
        assert r.Outputs.RenderedNormals.shape == r.Outputs.RGBMap.shape and torch.isfinite(r.Outputs.RenderedNormals).all()


@pytest.mark.parametrize("mode", ["cu", "ngp"])
def test_rendered_normals_deterministic_across_chunks_lanes_tiles(api, mode):
    L, mesh, R, scene = api
    sc = _scene(scene, mode)
    prec = "F16_SPLIT"
    base = _bits(_render(R, sc, scene, L, prec, 200, 200, chunk=40000, lanes=1).Outputs.RenderedNormals)
    assert (_bits(_render(R, sc, scene, L, prec, 200, 200, chunk=40000, lanes=1).Outputs.RenderedNormals) == base).all()
    assert (_bits(_render(R, sc, scene, L, prec, 200, 200, chunk=4096, lanes=2).Outputs.RenderedNormals) == base).all()
    assert (_bits(_render(R, sc, scene, L, prec, 200, 200, chunk=7000, lanes=4).Outputs.RenderedNormals) == base).all()
    top = _bits(_render(R, sc, scene, L, prec, 200, 200, rows=120, row0=0).Outputs.RenderedNormals)
    bot = _bits(_render(R, sc, scene, L, prec, 200, 200, rows=80, row0=120).Outputs.RenderedNormals)
    assert (np.concatenate([top, bot]) == base).all()
    n = base.view(np.float32).reshape(-1, 3)
    assert np.isfinite(n).all() and (np.linalg.norm(n, axis=1) <= 1 + 1e-5).all() and np.abs(n).max() > 0.1


def test_rendered_pred_normals_match_composite(api):
    L, mesh, R, scene = api
    from nerfpp_amd.modules import NeRFSmall
    sc = _scene(scene, "cu")
    blob = sc["mlp_blob"]
    n_params = NeRFSmall(3, 64, 15, 4, 64, True, 3, 64, 32, 16, "model").n_params
    extra = scene.synth_sym(9100, (n_params - blob.size,), np.float32(0.3))
    mlp = NeRFSmall(3, 64, 15, 4, 64, True, 3, 64, 32, 16, "model", params=np.concatenate([blob, extra]))
    r = R.NeRFRenderer(sc["embedder"], sc["embeddirs"], mlp)
    K, c2w = _camera(scene, 120, 160)
    p = scene.lego_render_params(n_importance=0, precision=L.NRF_PREC_F32, ReturnWeights=True, ReturnRaw=True, UsePredNormal=True, CalculateNormals=True)
    res = r.Render(120, 160, K, p, c2w=c2w)
    v = res.Raw[..., 4:7].double()
    ref = (res.Outputs.Weights.double()[..., None] * (v / torch.linalg.vector_norm(v, dim=-1, keepdim=True).clamp_min(1e-8))).sum(1)
    got = res.Outputs.RenderedPredNormals.reshape(-1, 3).double()
    assert res.Outputs.RenderedPredNormals.shape == res.Outputs.RGBMap.shape
    assert (got - ref).abs().max().item() <= 2e-6
    assert res.Outputs.RenderedNormals is not None and torch.isfinite(res.Outputs.RenderedNormals).all()
    with pytest.raises(L.NrfError, match="NRF_PREC_F32"):
        r.Render(120, 160, K, scene.lego_render_params(n_importance=0, precision=L.NRF_PREC_F16_MFMA, UsePredNormal=True), c2w=c2w)
    with pytest.raises(L.NrfError, match="unsupported"):
        sc["renderer"].Render(120, 160, K, scene.lego_render_params(n_importance=0, UsePredNormal=True), c2w=c2w)


def test_unsupported_renderers_and_null_outputs(api):
    L, mesh, R, scene = api
    K, c2w = _camera(scene, 32, 32)
    classic = scene.make_classic_scene()
    with pytest.raises(L.NrfError, match="unsupported"):
        classic["renderer"].Render(32, 32, K, scene.lego_render_params(CalculateNormals=True), c2w=c2w)
    with pytest.raises(L.NrfError, match="unsupported"):
        mesh.DensityGradient(classic["renderer"], torch.zeros((4, 3), device="cuda"))
    lerf = scene.make_lerf_scene(log2_t=14)
    with pytest.raises(L.NrfError, match="unsupported"):
        lerf["renderer"].Render(32, 32, K, scene.lego_render_params(CalculateNormals=True), c2w=c2w)
    # a set bit with a NULL output, or an unknown bit, fails before any launch
    sc = _scene(scene, "cu")
    rp = L.RenderParams()
    rp.n_samples = 8
    ro = L.RenderOutputs()
    nm = L.RenderNormals(L.NRF_NORMALS_DENSITY, None, None)
    fake = C.c_void_p(1 << 20)
    lib = L.lib()
    assert lib.nrf_render_rays_normals(sc["renderer"]._r, fake, 11, C.c_int64(4), C.byref(rp), fake, None, C.byref(ro), C.byref(nm), fake, C.c_size_t(1 << 30), None) == 1
    assert b"d_normals" in lib.nrf_last_error()
    assert lib.nrf_batchify_rays_normals(sc["renderer"]._r, fake, 11, C.c_int64(4), 4, C.byref(rp), fake, None, C.byref(ro), C.byref(nm), fake, C.c_size_t(1 << 30),
                                         None) == 1
    nm.bits = 4
    assert lib.nrf_render_rays_normals(sc["renderer"]._r, fake, 11, C.c_int64(4), C.byref(rp), fake, None, C.byref(ro), C.byref(nm), fake, C.c_size_t(1 << 30), None) == 1


def test_plain_entries_read_only_the_structs_they_are_given(api):
    """A caller compiled against the previous header hands structs of exactly the sizes below; what lies behind them in its memory is not the library's to read.
    Both structs are placed at the end of buffers filled with stray bytes: the plain entries render exactly what they rendered with clean memory."""
    L, mesh, R, scene = api
    sc = _scene(scene, "cu")
    r = sc["renderer"]
    K, c2w = _camera(scene, 48, 64)
    ro_, rd_, _ = R.GetRays(48, 64, K, c2w)
    rays = torch.empty((48 * 64, 11), device="cuda")
    bb = np.ascontiguousarray(scene.LEGO_BBOX, np.float32)
    o, d = ro_.reshape(-1, 3).contiguous(), rd_.reshape(-1, 3).contiguous()
    L.check(L.lib().nrf_pack_rays(R._ptr(o), R._ptr(d), bb.ctypes.data_as(C.c_void_p), C.c_int64(o.shape[0]), 1, R._ptr(rays), R._stream()))
    ref = r.Render(48, 64, K, scene.lego_render_params(chunk=1024), rays=(ro_, rd_, None)).Outputs.RGBMap.reshape(-1, 3).clone()

    def run(stray):
        rp = r._params(64, 128, None, False, 0.0, True, 0.0, 0.0, scene.LEGO_BBOX, L.NRF_PREC_F32, 0, 0, L.NRF_COARSE_AUTO)
        rgb = torch.empty((o.shape[0], 3), device="cuda")
        disp, acc, depth = (torch.empty((o.shape[0],), device="cuda") for _ in range(3))
        ro = L.RenderOutputs(R._ptr(rgb), R._ptr(disp), R._ptr(acc), R._ptr(depth), None, None, None, None, None, None)
        bufs = []
        for st in (rp, ro):
            b = (C.c_uint8 * (C.sizeof(st) + 64))(*([stray] * (C.sizeof(st) + 64)))
            C.memmove(b, C.byref(st), C.sizeof(st))
            bufs.append(b)
        lib = L.lib()
        t, u = R._ptr(r._linspace(64, "cuda")), R._ptr(r._linspace(128, "cuda"))
        n = o.shape[0]
        ws = torch.empty((lib.nrf_batchify_rays_workspace_bytes(r._r, C.c_int64(n), 1024, bufs[0]),), dtype=torch.uint8, device="cuda")
        L.check(lib.nrf_batchify_rays(r._r, R._ptr(rays), 11, C.c_int64(n), 1024, bufs[0], t, u, bufs[1], R._ptr(ws), C.c_size_t(ws.numel()), R._stream()))
        return rgb
    for stray in (0x00, 0x10, 0xFF):
        assert (_bits(run(stray)) == _bits(ref)).all(), stray


def test_extract_mesh_field_normals(api):
    L, mesh, R, scene = api
    sc = _scene(scene, "cu")
    r = sc["renderer"]
    g = mesh.DensityGrid(r, None, 128).cpu().numpy()
    iso = float(np.quantile(g, 0.7))
    m = mesh.ExtractMesh(r, iso, resolution=128, normals="field")
    _, grad = mesh.DensityGradient(r, m.Vertices)
    want = -grad / torch.linalg.vector_norm(grad, dim=-1, keepdim=True).clamp_min(1e-8)
    assert (_bits(m.Normals) == _bits(want)).all()
    nn = torch.linalg.vector_norm(m.Normals.double(), dim=-1)
    nz = torch.linalg.vector_norm(grad.double(), dim=-1) > 0
    assert nz.float().mean().item() > 0.99 and ((nn[nz] - 1).abs() < 1e-6).all()
    # the default is the lattice's, unchanged
    d = mesh.ExtractMesh(r, iso, resolution=128)
    v, f, n = mesh.Isosurface(mesh.DensityGrid(r, None, 128), sc["bbox"], iso)
    assert (_bits(d.Vertices) == _bits(v)).all() and (d.Faces == f).all() and (_bits(d.Normals) == _bits(n)).all()
    raw = r.RunNetwork(v[:1000, None, :], (-n[:1000]).contiguous())
    assert (_bits(d.Colors[:1000]) == _bits(torch.sigmoid(raw[:, 0, :3]))).all()
    assert (m.Vertices.shape == d.Vertices.shape) and (_bits(m.Vertices) == _bits(d.Vertices)).all()
