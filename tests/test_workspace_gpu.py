"""Every caller-owned workspace at exactly the size its *_workspace_bytes twin reports, on the MI355X.

A case asks the size function for B bytes and calls the entry through nerfpp_amd._lib.lib() (the Python mirror over-allocates and would hide a slip) with one
uint8 tensor of B + 1 MiB filled with 0xA5 and workspace_bytes = B: the call returns NRF_OK, the last 1 MiB is still 0xA5 (an overrun of the layout shows here, inside
the test's own allocation), and every output equals the same call on a 4 B workspace bit for bit.  With workspace_bytes = B - 1 the call returns
NRF_ERR_WORKSPACE and leaves its outputs as they were.  The size functions that take a ray or point count do not decrease over n = 1..130."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NRF_OK, NRF_ERR_WORKSPACE = 0, 4
GUARD = 1 << 20
FILL = 0xA5
LOG2_T = 12          # tiny tables: 16 levels x 2^12 entries


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from types import SimpleNamespace
    from nerfpp_amd import _lib as L, modules as M, renderer as R, scene as S, synth
    return SimpleNamespace(L=L, M=M, R=R, S=S, synth=synth, lib=L.lib())


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def bits(t):
    return t.detach().contiguous().view(torch.uint8).cpu().numpy()


def guarded(api, B, make_outs, run, what, refused_at=None):
    """The per-case checks.  make_outs() -> {name: tensor} freshly pre-filled; run(ws_ptr, ws_bytes, outs) -> status.  refused_at: the largest byte count the entry
    must refuse (B - 1 unless the entry adapts to what it is given)."""
    B = int(B)
    assert B > 0, what
    ws = torch.full((B + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    outs = make_outs()
    rc = run(P(ws), B, outs)
    torch.cuda.synchronize()
    assert rc == NRF_OK, (what, rc, api.lib.nrf_last_error())
    assert bool((ws[B:] == FILL).all()), f"{what}: the entry wrote past the {B} bytes its size function reports"
    big = torch.full((4 * B,), FILL, dtype=torch.uint8, device="cuda")
    ref = make_outs()
    rc = run(P(big), 4 * B, ref)
    torch.cuda.synchronize()
    assert rc == NRF_OK, (what, rc, api.lib.nrf_last_error())
    for k in outs:
        assert np.array_equal(bits(outs[k]), bits(ref[k])), f"{what}: {k} differs between the exact and the 4x workspace"
    untouched = make_outs()
    before = {k: bits(v) for k, v in untouched.items()}
    rc = run(P(ws), B - 1 if refused_at is None else int(refused_at), untouched)
    torch.cuda.synchronize()
    assert rc == NRF_ERR_WORKSPACE, (what, rc)
    for k in untouched:
        assert np.array_equal(bits(untouched[k]), before[k]), f"{what}: {k} was written by a call that returned NRF_ERR_WORKSPACE"
    return outs


def sentinel(*shape):
    return torch.full(shape, -123.5, device="cuda", dtype=torch.float32)


# ------------------------------------------------------------------------------------------------ scenes
_CACHE = {}


def scene_of(api, kind):
    """'cu' / 'ngp': hash grid of 16 levels x F 2, log2_hashmap_size 12, + NeRFSmall; 'classic': PE(10) / PE(4) + NeRF 8 x 256; 'pn': the 'cu' grid with the 7-column
    NeRFSmall (predicted-normals head); 'sh3': a hash renderer the fast paths do not serve; 'lerf': L16 F8 language grid + the LeRF head."""
    if kind in _CACHE:
        return _CACHE[kind]
    S = api.S
    if kind in ("cu", "ngp"):
        sc = S.make_hash_scene(mode=kind, log2_t=LOG2_T)
    elif kind == "sh3":          # SH degree 3: 9 direction features, outside the matrix-core family -- the generic row-major network in every precision
        sc = S.make_hash_scene(mode="cu", log2_t=LOG2_T, sh_degree=3)
    elif kind == "classic":
        sc = S.make_classic_scene()
    elif kind == "pn":
        base = scene_of(api, "cu")
        d = api.L.MlpSmallDesc(32, 16, 3, 64, 15, 4, 64, 1, 3, 64)
        n_pn = int(api.lib.nrf_mlp_small_param_count(C.byref(d)))
        blob = np.concatenate([base["mlp_blob"], api.synth.synth_sym(91, (n_pn - base["mlp_blob"].size,), np.float32(0.1))]).astype(np.float32)
        mlp = api.M.NeRFSmall(3, 64, 15, 4, 64, True, 3, 64, 32, 16, "model", params=blob)
        sc = dict(renderer=api.R.NeRFRenderer(base["embedder"], base["embeddirs"], mlp), mlp=mlp, mlp_blob=blob, bbox=base["bbox"])
    elif kind == "lerf":
        sc = S.make_lerf_scene(log2_t=LOG2_T)
        rng = np.random.RandomState(86)
        pos = rng.randn(1, 768).astype(np.float32); pos /= np.linalg.norm(pos)
        neg = rng.randn(3, 768).astype(np.float32); neg /= np.linalg.norm(neg, axis=1, keepdims=True)
        sc["renderer"].SetLeRFPrompts(pos, neg)
    _CACHE[kind] = sc
    return sc


def packed_rays(api, n, viewdirs=True):
    """n packed rays [n, 11 | 8] across the object (nrf_pack_rays: o, d, near, far, viewdirs)."""
    key = ("rays", n, viewdirs)
    if key not in _CACHE:
        K = api.S.lego_K(16, 16)
        o, d, _ = api.R.GetRays(16, 16, K, api.S.pose_spherical(30.0, -30.0, 4.0))
        o = o.reshape(-1, 3)[40:40 + n].contiguous(); d = d.reshape(-1, 3)[40:40 + n].contiguous()
        assert o.shape[0] == n
        out = torch.empty((n, 11 if viewdirs else 8), device="cuda")
        bb = np.ascontiguousarray(api.S.LEGO_BBOX, np.float32).reshape(6)
        api.L.check(api.lib.nrf_pack_rays(P(o), P(d), bb.ctypes.data_as(C.c_void_p), n, int(viewdirs), P(out), None))
        torch.cuda.synchronize()
        _CACHE[key] = out
    return _CACHE[key]


def lin(steps):
    key = ("lin", steps)
    if key not in _CACHE:
        _CACHE[key] = torch.linspace(0.0, 1.0, steps, dtype=torch.float32).cuda()
    return _CACHE[key]


def params(api, s, ni, prec, coarse=0, **kw):
    rp = api.L.RenderParams(s, ni, 0, 1, prec, api.R.ATEN_SUM_VEC)
    rp.coarse_mode = coarse
    rp.seed = 7
    bb = np.asarray(api.S.LEGO_BBOX, np.float32).reshape(6)
    rp.has_bbox, rp.bbox = 1, (C.c_float * 6)(*bb.tolist())
    for k, v in kw.items():
        setattr(rp, k, v)
    return rp


def render_outs(n, s, ni, c, supplied, normals=0):
    """make_outs of the NeRF render entries: the four maps always, every optional output when supplied."""
    so = s + ni if ni > 0 else s

    def make():
        o = dict(rgb=sentinel(n, 3), disp=sentinel(n), acc=sentinel(n), depth=sentinel(n))
        if supplied:
            o.update(weights=sentinel(n, so), raw=sentinel(n, so, c), z_coarse=sentinel(n, s), raw_coarse=sentinel(n, s, c), weights_coarse=sentinel(n, s))
            if ni > 0:
                o["z_fine"] = sentinel(n, s + ni)
        if normals & 1:
            o["normals"] = sentinel(n, 3)
        if normals & 2:
            o["pred_normals"] = sentinel(n, 3)
        return o
    return make


def outputs_struct(api, o):
    ro = api.L.RenderOutputs()
    for k in ("rgb", "disp", "acc", "depth", "weights", "raw", "z_coarse", "raw_coarse", "weights_coarse", "z_fine"):
        setattr(ro, "d_" + k, o[k].data_ptr() if k in o else None)
    return ro


def normals_struct(api, o, normals):
    return api.L.RenderNormals(normals, o["normals"].data_ptr() if "normals" in o else None, o["pred_normals"].data_ptr() if "pred_normals" in o else None)


def render_rays_case(api, kind, n, s, ni, prec, coarse=0, supplied=False, normals=0, **kw):
    sc = scene_of(api, kind)
    r = sc["renderer"]._r
    c = sc["mlp"].GetOutputDims()
    rays = packed_rays(api, n)
    rp = params(api, s, ni, prec, coarse, **kw)
    t, u = lin(s), (lin(ni) if ni > 0 else None)
    lib = api.lib
    if normals:
        B = lib.nrf_render_rays_normals_workspace_bytes(r, n, C.byref(rp), normals)
    else:
        B = lib.nrf_render_rays_workspace_bytes(r, n, C.byref(rp))

    def run(ws, nb, o):
        ro = outputs_struct(api, o)
        if normals:
            nm = normals_struct(api, o, normals)
            return lib.nrf_render_rays_normals(r, P(rays), 11, n, C.byref(rp), P(t), P(u), C.byref(ro), C.byref(nm), ws, nb, None)
        return lib.nrf_render_rays(r, P(rays), 11, n, C.byref(rp), P(t), P(u), C.byref(ro), ws, nb, None)
    what = f"nrf_render_rays {kind} n {n} s {s}+{ni} prec {prec} coarse {coarse} supplied {supplied} normals {normals} {kw}"
    outs = guarded(api, B, render_outs(n, s, ni, c, supplied, normals), run, what)
    assert torch.isfinite(outs["rgb"]).all() and float(outs["rgb"].max()) > -100.0, what          # (written: the sentinel is -123.5)
    return outs


COUNTS = ((4, 0), (4, 3), (7, 1), (8, 24))


# ------------------------------------------------------------------------------------------------ nrf_run_network
@pytest.mark.parametrize("kind", ["cu", "ngp", "classic", "sh3"])
def test_run_network(api, kind):
    sc = scene_of(api, kind)
    r, c = sc["renderer"]._r, sc["mlp"].GetOutputDims()
    rng = np.random.default_rng(3)
    for n, s in ((5, 3), (70, 7)):
        pts = dev(rng.uniform(-1.4, 1.4, (n, s, 3)))
        vd = dev(rng.standard_normal((n, 3)))
        B = api.lib.nrf_run_network_workspace_bytes(r, n, s)
        for prec in ((0,) if kind == "sh3" else (0, 1, 2)):          # ('sh3' is outside the matrix-core family: NRF_PREC_F32 only)
            run = lambda ws, nb, o: api.lib.nrf_run_network(r, P(pts), P(vd), n, s, prec, P(o["raw"]), ws, nb, None)
            guarded(api, B, lambda: dict(raw=sentinel(n, s, c)), run, f"nrf_run_network {kind} {n}x{s} prec {prec}")


# ------------------------------------------------------------------------------------------------ nrf_render_rays
@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("kind", ["cu", "ngp", "classic"])
def test_render_rays_grid(api, kind, prec):
    """n = 5 and 67 rays x the four sample-count pairs x coarse_mode AUTO / FULL / SIGMA_F32: every strategy of the chunk layout (generic, raw reuse, feature reuse,
    geo hand-over, sigma only; exact and plain classic), with no optional output supplied (the largest layout)."""
    for n in (5, 67):
        for s, ni in COUNTS:
            for coarse in (0, 1, 2):
                render_rays_case(api, kind, n, s, ni, prec, coarse)


@pytest.mark.parametrize("prec", [0, 2])
@pytest.mark.parametrize("kind", ["cu", "ngp", "classic"])
def test_render_rays_extras(api, kind, prec):
    """Every optional output supplied (raw_coarse selects the full coarse pass), Perturb > 0, cone rays, stochastic preconditioning with a box."""
    for s, ni in COUNTS:
        render_rays_case(api, kind, 67, s, ni, prec, supplied=True)
    for s, ni in ((4, 3), (8, 24)):
        render_rays_case(api, kind, 67, s, ni, prec, perturb=1.0)
        render_rays_case(api, kind, 67, s, ni, prec, has_cone=1, cone_angle=0.01)
        render_rays_case(api, kind, 67, s, ni, prec, precond_alpha=0.02)
        render_rays_case(api, kind, 5, s, ni, prec, supplied=True, perturb=1.0, has_cone=1, cone_angle=0.01, precond_alpha=0.02)


def test_render_rays_normals(api):
    """The normals entries with each bit on the 7-column network in NRF_PREC_F32 (the only precision the predicted-normals head has), and the density bit on the
    4-column network in NRF_PREC_F16_SPLIT."""
    for s, ni in ((4, 0), (4, 3)):
        for bits_ in (1, 2, 3):
            for supplied in (False, True):
                render_rays_case(api, "pn", 67, s, ni, 0, supplied=supplied, normals=bits_)
        for kind in ("cu", "ngp"):
            for supplied in (False, True):
                render_rays_case(api, kind, 67, s, ni, 2, supplied=supplied, normals=1)


# ------------------------------------------------------------------------------------------------ nrf_batchify_rays / nrf_render_rows
def batchify(api, kind, n, chunk, s, ni, prec, lanes, supplied=False):
    sc = scene_of(api, kind)
    r, c = sc["renderer"]._r, sc["mlp"].GetOutputDims()
    lib = api.lib
    api.L.check(lib.nrf_renderer_set_lanes(r, lanes))
    try:
        rays = packed_rays(api, n) if n <= 216 else _CACHE[("bigrays", n)]
        rp = params(api, s, ni, prec)
        t, u = lin(s), (lin(ni) if ni > 0 else None)
        B = lib.nrf_batchify_rays_workspace_bytes(r, n, chunk, C.byref(rp))

        def run(ws, nb, o):
            ro = outputs_struct(api, o)
            return lib.nrf_batchify_rays(r, P(rays), 11, n, chunk, C.byref(rp), P(t), P(u), C.byref(ro), ws, nb, None)
        return guarded(api, B, render_outs(n, s, ni, c, supplied), run, f"nrf_batchify_rays {kind} n {n} chunk {chunk} {s}+{ni} prec {prec} lanes {lanes}")
    finally:
        api.L.check(lib.nrf_renderer_set_lanes(r, 0))


@pytest.mark.parametrize("prec", [0, 2])
@pytest.mark.parametrize("kind", ["cu", "classic"])
def test_batchify_rays(api, kind, prec):
    """150 rays in chunks of 64 (two whole chunks and a tail) and a batch below one chunk, on a 1-lane and a 2-lane renderer; the 2-lane result equals the 1-lane one.
    (Below 32 768 rays the loop stays on the caller's stream whatever the lane count: the lanes themselves are the next test's.)"""
    for s, ni in ((4, 3), (8, 24)):
        one = batchify(api, kind, 150, 64, s, ni, prec, 1, supplied=True)
        two = batchify(api, kind, 150, 64, s, ni, prec, 2, supplied=True)
        for k in one:
            assert np.array_equal(bits(one[k]), bits(two[k])), (kind, prec, s, ni, k)
        batchify(api, kind, 50, 64, s, ni, prec, 2)


@pytest.mark.parametrize("prec", [0, 2])
def test_batchify_rays_on_lanes(api, prec):
    """33 000 rays (above the 32 768 from which the loop forks) at 4 + 3 samples in chunks of 9 000 -- no multiple of 64 -- on 2 lanes: the staggered first chunks and the
    balanced tail, each chunk in a lane slice of exactly the reported size; equal to the 1-lane loop bit for bit.  And one chunk cut in two (n <= Chunk)."""
    n = 33000
    if ("bigrays", n) not in _CACHE:
        base = packed_rays(api, 200)
        _CACHE[("bigrays", n)] = base.repeat((n + 199) // 200, 1)[:n].contiguous()
    one = batchify(api, "cu", n, 9000, 4, 3, prec, 1)
    two = batchify(api, "cu", n, 9000, 4, 3, prec, 2)
    for k in one:
        assert np.array_equal(bits(one[k]), bits(two[k])), (prec, k)
    batchify(api, "cu", n, 40000, 4, 3, prec, 2)


def view_of(api, w, rows, chunk, use_viewdirs=1):
    v = api.L.View()
    v.h, v.w, v.row0, v.rows = rows, w, 0, rows
    v.K = (C.c_float * 9)(*api.S.lego_K(rows, w).reshape(-1).tolist())
    v.c2w = (C.c_float * 12)(*np.asarray(api.S.pose_spherical(30.0, -30.0, 4.0), np.float32).reshape(-1).tolist())
    v.use_viewdirs, v.ndc, v.chunk = use_viewdirs, 0, chunk
    v.bbox = (C.c_float * 6)(*np.asarray(api.S.LEGO_BBOX, np.float32).reshape(-1).tolist())
    return v


@pytest.mark.parametrize("prec", [0, 2])
@pytest.mark.parametrize("kind", ["cu", "classic"])
def test_render_rows(api, kind, prec):
    """A 9 x 7 view in chunks of 16, with and without d_rays_out (without: the rays are one more piece of the workspace)."""
    sc = scene_of(api, kind)
    r, c = sc["renderer"]._r, sc["mlp"].GetOutputDims()
    lib = api.lib
    v = view_of(api, 9, 7, 16)
    n, s, ni = 63, 4, 3
    rp = params(api, s, ni, prec)
    B = lib.nrf_render_rows_workspace_bytes(r, C.byref(v), C.byref(rp))
    for keep_rays in (False, True):
        def make():
            o = render_outs(n, s, ni, c, False)()
            o["near_far"] = sentinel(2)
            if keep_rays:
                o["rays"] = sentinel(n, 11)
            return o

        def run(ws, nb, o):
            ro = outputs_struct(api, o)
            return lib.nrf_render_rows(r, C.byref(v), C.byref(rp), P(lin(s)), P(lin(ni)), C.byref(ro), P(o.get("rays")), P(o["near_far"]), ws, nb, None)
        guarded(api, B, make, run, f"nrf_render_rows {kind} prec {prec} d_rays_out {keep_rays}")


# ------------------------------------------------------------------------------------------------ LeRF
def lerf_outs(n, s, ni, which):
    def make():
        o = {}
        if which in ("embedding", "all"):
            o["embedding"] = sentinel(n, 768)
        if which in ("relevancy", "all"):
            o["relevancy"] = sentinel(n, 2)
        if which == "all":
            o.update(disp=sentinel(n), acc=sentinel(n), depth=sentinel(n), weights=sentinel(n, s + ni), z_coarse=sentinel(n, s), weights_coarse=sentinel(n, s),
                     z_fine=sentinel(n, s + ni))
        return o
    return make


def lerf_struct(api, o):
    ro = api.L.LerfOutputs()
    for k in ("embedding", "disp", "acc", "depth", "weights", "relevancy", "z_coarse", "weights_coarse", "z_fine"):
        setattr(ro, "d_" + k, o[k].data_ptr() if k in o else None)
    return ro


@pytest.mark.parametrize("ni", [32, 64])
def test_lerf_render_entries(api, ni):
    """nrf_lerf_render_rays / _batchify_rays / _render_rows at 32 + 32 and 32 + 64 samples (the smallest the pass accepts), 3 and 40 rays in chunks of 16, on 1 and 2
    lanes (the LeRF loop forks whenever the batch is more than one chunk); embedding only, relevancy only, all outputs."""
    sc = scene_of(api, "lerf")
    rr = sc["renderer"]
    r, lib, s = rr._r, api.lib, 32
    rp = api.L.RenderParams(s, ni, 0, 0, rr.precision, api.R.ATEN_SUM_VEC)
    t, u = lin(s), lin(ni)
    try:
        for which in ("embedding", "relevancy", "all"):
            for n in (3, 40):
                rays = packed_rays(api, n, viewdirs=False)
                B = lib.nrf_lerf_render_rays_workspace_bytes(r, n, C.byref(rp))
                run = lambda ws, nb, o: lib.nrf_lerf_render_rays(r, P(rays), 8, n, C.byref(rp), P(t), P(u), C.byref(lerf_struct(api, o)), ws, nb, None)
                guarded(api, B, lerf_outs(n, s, ni, which), run, f"nrf_lerf_render_rays n {n} {s}+{ni} {which}")
                res = {}
                for lanes in (1, 2):
                    api.L.check(lib.nrf_lerf_renderer_set_lanes(r, lanes))
                    B = lib.nrf_lerf_batchify_rays_workspace_bytes(r, n, 16, C.byref(rp))
                    run = lambda ws, nb, o: lib.nrf_lerf_batchify_rays(r, P(rays), 8, n, 16, C.byref(rp), P(t), P(u), C.byref(lerf_struct(api, o)), ws, nb, None)
                    res[lanes] = guarded(api, B, lerf_outs(n, s, ni, which), run, f"nrf_lerf_batchify_rays n {n} {s}+{ni} {which} lanes {lanes}")
                for k in res[1]:
                    assert np.array_equal(bits(res[1][k]), bits(res[2][k])), (n, ni, which, k)
        for w, rows in ((3, 1), (8, 5)):
            v = view_of(api, w, rows, 16, use_viewdirs=0)
            n = w * rows
            for lanes in (1, 2):
                api.L.check(lib.nrf_lerf_renderer_set_lanes(r, lanes))
                B = lib.nrf_lerf_render_rows_workspace_bytes(r, C.byref(v), C.byref(rp))
                for keep_rays in (False, True):
                    def make():
                        o = lerf_outs(n, s, ni, "all")()
                        o["near_far"] = sentinel(2)
                        if keep_rays:
                            o["rays"] = sentinel(n, 8)
                        return o
                    run = lambda ws, nb, o: lib.nrf_lerf_render_rows(r, C.byref(v), C.byref(rp), P(t), P(u), C.byref(lerf_struct(api, o)), P(o.get("rays")), P(o["near_far"]),
                                                                     ws, nb, None)
                    guarded(api, B, make, run, f"nrf_lerf_render_rows {w}x{rows} {s}+{ni} lanes {lanes} d_rays_out {keep_rays}")
    finally:
        api.L.check(lib.nrf_lerf_renderer_set_lanes(r, int(rr.lanes)))


def test_lerf_backward_entries(api):
    """nrf_lerf_head_backward and nrf_lerf_backward_points at 3 rays x 32 samples.  The gradient buffers are accumulated into (they start at zero) by float atomics
    whose order is not fixed, so a sum of three or more non-zero addends has no bits of its own to compare.  The inputs leave every accumulator at most two: only the
    middle ray carries a gradient, and only two of its samples lie inside the box (keep mask 0 / a point outside: sigma_le is masked, the weight and with it every
    gradient of that sample is exactly 0).  All 96 points still go through every buffer of the layout."""
    sc = scene_of(api, "lerf")
    lerf, rr, lib = sc["lerf"], sc["renderer"], api.lib
    n, s, E, in_ch = 3, 32, 768, 128
    rng = np.random.default_rng(5)
    emb = dev(rng.uniform(-0.5, 0.5, (n * s, in_ch)))
    live = np.zeros((n, s), bool); live[1, 5] = live[1, 20] = True
    keep = np.ones((n, s), np.uint8); keep[1] = live[1]
    keep = dev(keep.reshape(-1), np.uint8)
    z = dev(np.sort(rng.uniform(2.0, 6.0, (n, s)), axis=1))
    d = dev(rng.standard_normal((n, 3)))
    g = rng.standard_normal((n, E)) * 1e-2; g[0] = 0; g[2] = 0
    g = dev(g)
    n_params = int(lerf.n_params)
    make = lambda: dict(g_params=torch.zeros((n_params,), device="cuda"), g_emb=sentinel(n * s, in_ch), rendered=sentinel(n, E), weights=sentinel(n, s))
    run = lambda ws, nb, o: lib.nrf_lerf_head_backward(lerf._m, P(emb), P(keep), P(z), P(d), 3, n, s, None, 0.0, P(g), P(o["g_params"]), P(o["g_emb"]), P(o["rendered"]),
                                                       P(o["weights"]), ws, nb, None)
    guarded(api, lib.nrf_lerf_head_backward_workspace_bytes(lerf._m, n, s), make, run, "nrf_lerf_head_backward")
    pts = rng.uniform(-1.4, 1.4, (n, s, 3)); pts[1][~live[1]] += 5.0          # (outside the box)
    pts = dev(pts.reshape(-1, 3))
    n_table = int(sc["embedder"].table_elems())
    make = lambda: dict(g_params=torch.zeros((n_params,), device="cuda"), g_table=torch.zeros((n_table,), device="cuda"))
    run = lambda ws, nb, o: lib.nrf_lerf_backward_points(rr._r, P(pts), P(z), P(d), 3, n, s, None, 0.0, P(g), P(o["g_params"]), P(o["g_table"]), ws, nb, None)
    guarded(api, lib.nrf_lerf_backward_points_workspace_bytes(rr._r, n, s), make, run, "nrf_lerf_backward_points")


def test_lerf_query_entries(api):
    """The 3D relevancy entries (their workspaces became layouts with the rest): the head on 37 rows, 37 points, a 5 x 4 x 3 lattice; NRF_PREC_F32 and split."""
    sc = scene_of(api, "lerf")
    lerf, r, lib = sc["lerf"], sc["renderer"]._r, api.lib
    rng = np.random.default_rng(9)
    p = 37
    x = dev(rng.uniform(-0.5, 0.5, (p, 128)))
    unit = lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)
    pos, neg = dev(unit(rng.standard_normal((1, 768)))), dev(unit(rng.standard_normal((3, 768))))
    pts = dev(rng.uniform(-1.4, 1.4, (p, 3)))
    bb = np.ascontiguousarray(api.S.LEGO_BBOX, np.float32).reshape(6)
    for prec in (0, 2):
        make = lambda: dict(sigma=sentinel(p), rel=sentinel(p, 2))
        run = lambda ws, nb, o: lib.nrf_lerf_head_relevancy(lerf._m, P(x), p, P(pos), 1, P(neg), 3, 0, prec, P(o["sigma"]), P(o["rel"]), ws, nb, None)
        guarded(api, lib.nrf_lerf_head_relevancy_workspace_bytes(lerf._m, p, 3, prec), make, run, f"nrf_lerf_head_relevancy prec {prec}")
        run = lambda ws, nb, o: lib.nrf_lerf_point_relevancy(r, P(pts), p, 0, prec, P(o["sigma"]), P(o["rel"]), 7, ws, nb, None)
        guarded(api, lib.nrf_lerf_point_relevancy_workspace_bytes(r, p, prec, 7), make, run, f"nrf_lerf_point_relevancy prec {prec}")
        make = lambda: dict(sigma=sentinel(60), rel=sentinel(60, 2))
        run = lambda ws, nb, o: lib.nrf_lerf_relevancy_grid(r, bb.ctypes.data_as(C.c_void_p), 5, 4, 3, 0, prec, P(o["sigma"]), P(o["rel"]), 7, ws, nb, None)
        guarded(api, lib.nrf_lerf_relevancy_grid_workspace_bytes(r, 5, 4, 3, prec, 7), make, run, f"nrf_lerf_relevancy_grid prec {prec}")


def test_pyramid_relevancy_preview(api):
    """nrf_pyramid_relevancy_preview on a 48 x 40 view of 37-wide embeddings (a row of neither buffer is a multiple of 256 bytes).  The entry takes as many rows at a
    time as the bytes it is given hold, so it is run at the size of 7 rows, of all 40, and of 3 rows and a half (a non-integral number: it must take 3); only a buffer
    below one row is refused."""
    from test_pyramid_host import random_pyramid
    from nerfpp_amd.pyramid import PyramidEmbedding, PyramidEmbedderProperties, MaxZoomOut

    class View:
        def __init__(self, W, H):
            self.W, self.H = W, H
    wh, clip, overlap, d = [(160, 96), (48, 40)], 32, 0.5, 37
    views = [View(w, h) for w, h in wh]
    props = PyramidEmbedderProperties(ImgSize=(clip, clip), Overlap=overlap, MaxZoomOut=MaxZoomOut(views, clip))
    pyr = PyramidEmbedding(props, random_pyramid(wh, clip, overlap, d, 50)).to_device(views)
    try:
        lib, h = api.lib, pyr._handle()
        rng = np.random.RandomState(51)
        unit = lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)
        pos, neg = dev(unit(rng.randn(2, d))), dev(unit(rng.randn(3, d)))
        make = lambda: dict(gray=torch.full((40, 48), 0x5A, dtype=torch.uint8, device="cuda"), bgr=torch.full((40, 48, 3), 0x5A, dtype=torch.uint8, device="cuda"))
        run = lambda ws, nb, o: lib.nrf_pyramid_relevancy_preview(h, 1, 0.5, P(pos), 2, P(neg), 3, 1, P(o["gray"]), P(o["bgr"]), ws, nb, None)
        size = lambda rows: int(lib.nrf_pyramid_relevancy_preview_workspace_bytes(h, 1, rows))
        one = size(1)
        assert size(3) < 3 * one and size(400) == size(40)          # (rows share the 256-byte rounding; more rows than the view has are the view's)
        got = [guarded(api, B, make, run, f"nrf_pyramid_relevancy_preview {B} bytes", refused_at=one - 1) for B in (size(7), size(40), size(3) + one // 2, one)]
        for g in got[1:]:
            assert np.array_equal(bits(g["gray"]), bits(got[0]["gray"])) and np.array_equal(bits(g["bgr"]), bits(got[0]["bgr"]))
        assert len(np.unique(bits(got[0]["gray"]))) > 4
    finally:
        pyr.close()


# ------------------------------------------------------------------------------------------------ density
@pytest.mark.parametrize("kind", ["cu", "ngp", "classic", "sh3"])
def test_density_grid(api, kind):
    """A 5 x 4 x 3 lattice in slabs of 7 points: the hash-exact ('cu', 'ngp'), classic-exact and generic ('sh3') renderers."""
    r, lib = scene_of(api, kind)["renderer"]._r, api.lib
    bb = np.ascontiguousarray(api.S.LEGO_BBOX, np.float32).reshape(6)
    run = lambda ws, nb, o: lib.nrf_density_grid(r, bb.ctypes.data_as(C.c_void_p), 5, 4, 3, P(o["sigma"]), 7, ws, nb, None)
    guarded(api, lib.nrf_density_grid_workspace_bytes(r, 5, 4, 3, 7), lambda: dict(sigma=sentinel(3, 4, 5)), run, f"nrf_density_grid {kind}")


def test_density_grad_takes_no_workspace(api):
    """nrf_density_grad at 37 points: its size is 0, it runs with 0 bytes and leaves the guard band alone (there is no B - 1 to pass)."""
    r, lib = scene_of(api, "cu")["renderer"]._r, api.lib
    p = 37
    assert lib.nrf_density_grad_workspace_bytes(r, p) == 0
    pts = dev(np.random.default_rng(2).uniform(-1.4, 1.4, (p, 3)))
    ws = torch.full((GUARD,), FILL, dtype=torch.uint8, device="cuda")
    got = []
    for w, nb in ((ws, 0), (None, 0)):
        sig, grad = sentinel(p), sentinel(p, 3)
        assert lib.nrf_density_grad(r, P(pts), p, P(sig), P(grad), P(w), nb, None) == NRF_OK
        torch.cuda.synchronize()
        got.append((bits(sig), bits(grad)))
    assert bool((ws == FILL).all())
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])


# ------------------------------------------------------------------------------------------------ training backwards
def test_mlp_backward_families(api):
    """nrf_mlp_backward on NeRFSmall and on the classic NeRF at 33 rows, nrf_mlp_backward_f16 at 64, nrf_mlp_backward_pn at 33 (7 gradient columns).  The parameter
    gradients are sums by float atomics in no fixed order (the bias sums: one addend per wave), which have bits of their own only up to two non-zero addends: the output
    gradient is non-zero in the first and the last row alone.  Every row still goes through every buffer of the layout."""
    lib = api.lib
    rng = np.random.default_rng(13)
    for kind, fn, wsfn, p, gcols in (("cu", lib.nrf_mlp_backward, lib.nrf_mlp_backward_workspace_bytes, 33, 4),
                                     ("classic", lib.nrf_mlp_backward, lib.nrf_mlp_backward_workspace_bytes, 33, 4),
                                     ("cu", lib.nrf_mlp_backward_f16, lib.nrf_mlp_backward_f16_workspace_bytes, 64, 4),
                                     ("pn", lib.nrf_mlp_backward_pn, lib.nrf_mlp_backward_pn_workspace_bytes, 33, 7)):
        m = scene_of(api, kind)["mlp"]
        in_dims, in_ch = (90, 63) if kind == "classic" else (48, 32)
        x = dev(rng.uniform(-1, 1, (p, in_dims)))
        go = rng.standard_normal((p, gcols)); go[1:-1] = 0
        go = dev(go)
        n_params = int(m.n_params)
        make = lambda: dict(g_params=torch.zeros((n_params,), device="cuda"), g_x=sentinel(p, in_ch))
        run = lambda ws, nb, o: fn(m._m, P(x), P(go), p, P(o["g_params"]), P(o["g_x"]), ws, nb, None)
        guarded(api, wsfn(m._m, p), make, run, f"{fn.__name__} {kind} p {p}")


@pytest.mark.parametrize("mode", ["cu", "ngp"])
def test_hash_backward_packed_and_binned(api, mode):
    """nrf_hash_backward_rays_packed, and nrf_hash_backward_rays_binned at the worst-case size (records for a whole pass) and at the size for this batch (40 rays, far
    below one group of 2^18 points: the record buffer is sized by the rays held).  The table gradient is a sum of integers: the three agree bit for bit."""
    e, lib = scene_of(api, mode)["embedder"], api.lib
    rng = np.random.default_rng(17)
    n, s = 40, 7
    bb = np.asarray(api.S.LEGO_BBOX, np.float32)
    pts = rng.uniform(bb[:3], bb[3:], (n * s, 3)).astype(np.float32); pts[:s] = pts[0]; pts[s:2 * s] += np.float32(3.0 if mode == "cu" else 2e-3)
    g = (rng.standard_normal((n * s, 32)) * 1e-4).astype(np.float32); g[rng.random(n * s) < 0.1] = 0
    dp, dg = dev(pts), dev(g)
    elems = int(e.table_elems())
    make = lambda: dict(g_table=torch.zeros((elems,), device="cuda"))
    got = []
    for name, fn, B in (("packed", lib.nrf_hash_backward_rays_packed, lib.nrf_hash_backward_packed_workspace_bytes(e._h)),
                        ("binned", lib.nrf_hash_backward_rays_binned, lib.nrf_hash_backward_binned_workspace_bytes_for(e._h, n, s)),
                        ("binned, worst case", lib.nrf_hash_backward_rays_binned, lib.nrf_hash_backward_binned_workspace_bytes(e._h, s))):
        run = lambda ws, nb, o: fn(e._h, P(dp), n, s, P(dg), P(o["g_table"]), ws, nb, None)
        # (the binned entry is sized by THIS call's rays: the batch-sized count is its B whatever the buffer holds)
        refused = lib.nrf_hash_backward_binned_workspace_bytes_for(e._h, n, s) - 1 if name.startswith("binned") else None
        got.append(guarded(api, B, make, run, f"nrf_hash_backward_rays {name} {mode}", refused_at=refused))
    assert float(got[0]["g_table"].abs().max()) > 0
    for o in got[1:]:
        assert np.array_equal(bits(o["g_table"]), bits(got[0]["g_table"]))


def test_normal_losses_and_ray_regularizers(api):
    """nrf_normal_losses at n = 257, s = 64 and nrf_ray_regularizers at n = 64, s = 64: the shapes of their own tests."""
    lib = api.lib
    rng = np.random.default_rng(11)
    n, s = 257, 64
    w = dev(rng.uniform(0, 1, (n, s))); g = dev(rng.standard_normal((n, s, 3))); raw = dev(rng.standard_normal((n, s, 7))); rays = dev(rng.standard_normal((n, 11)))
    make = lambda: dict(g_raw=sentinel(n, s, 7), losses=sentinel(2))
    run = lambda ws, nb, o: lib.nrf_normal_losses(P(w), P(g), P(raw), 7, C.c_void_p(rays.data_ptr() + 12), 11, n, s, 0.7, 0.3, P(o["g_raw"]), P(o["losses"]), ws, nb, None)
    guarded(api, lib.nrf_normal_losses_workspace_bytes(n, s), make, run, "nrf_normal_losses")
    n, s, c = 64, 64, 4
    raw = dev(rng.standard_normal((n, s, c))); z = dev(np.sort(rng.uniform(2.0, 6.0, (n, s)), axis=1)); d = dev(rng.standard_normal((n, 3)))
    make = lambda: dict(g_raw=torch.zeros((n, s, c), device="cuda"), losses=sentinel(2), weights=sentinel(n, s))
    run = lambda ws, nb, o: lib.nrf_ray_regularizers(P(raw), P(z), P(d), 3, n, s, c, None, 0.0, 0.01, 0.001, P(o["g_raw"]), P(o["losses"]), P(o["weights"]), ws, nb, None)
    guarded(api, lib.nrf_ray_regularizers_workspace_bytes(n, s), make, run, "nrf_ray_regularizers")


# ------------------------------------------------------------------------------------------------ sizes
def test_sizes_do_not_decrease_with_the_count(api):
    """Every size function that takes a ray or point count, n = 1..130 at two sample-count pairs: non-decreasing (a lane slice sized for lane_chunk rays holds every
    shorter chunk the loop cuts).  Host arithmetic on created handles."""
    lib = api.lib
    fns = {}
    for kind in ("cu", "ngp", "classic", "pn"):
        r = scene_of(api, kind)["renderer"]._r
        m = scene_of(api, kind)["mlp"]._m
        for s, ni in ((7, 1), (8, 24)):
            fns[f"run_network {kind} {s}"] = lambda n, r=r, s=s: lib.nrf_run_network_workspace_bytes(r, n, s)
            for prec in (0, 1, 2):
                for coarse in (0, 1, 2):
                    rp = params(api, s, ni, prec, coarse)
                    fns[f"render_rays {kind} {s}+{ni} {prec} {coarse}"] = lambda n, r=r, rp=rp: lib.nrf_render_rays_workspace_bytes(r, n, C.byref(rp))
                    fns[f"render_rays_normals {kind} {s}+{ni} {prec} {coarse}"] = lambda n, r=r, rp=rp: lib.nrf_render_rays_normals_workspace_bytes(r, n, C.byref(rp), 3)
                    fns[f"batchify {kind} {s}+{ni} {prec} {coarse}"] = lambda n, r=r, rp=rp: lib.nrf_batchify_rays_workspace_bytes(r, n, 64, C.byref(rp))
        fns[f"mlp_backward {kind}"] = lambda n, m=m: lib.nrf_mlp_backward_workspace_bytes(m, n)
        if kind in ("cu", "ngp"):
            for s in (7, 32):
                fns[f"hash_backward_binned_for {kind} {s}"] = lambda n, h=scene_of(api, kind)["embedder"]._h, s=s: lib.nrf_hash_backward_binned_workspace_bytes_for(h, n, s)
        fns[f"density_grad {kind}"] = lambda n, r=r: lib.nrf_density_grad_workspace_bytes(r, n)
    fns["mlp_backward_f16"] = lambda n: lib.nrf_mlp_backward_f16_workspace_bytes(scene_of(api, "cu")["mlp"]._m, n)
    fns["mlp_backward_pn"] = lambda n: lib.nrf_mlp_backward_pn_workspace_bytes(scene_of(api, "pn")["mlp"]._m, n)
    sc = scene_of(api, "lerf")
    lr, lm = sc["renderer"]._r, sc["lerf"]._m
    for s, ni in ((32, 32), (32, 64)):
        rp = api.L.RenderParams(s, ni, 0, 0, sc["renderer"].precision, api.R.ATEN_SUM_VEC)
        fns[f"lerf_render_rays {s}+{ni}"] = lambda n, rp=rp: lib.nrf_lerf_render_rays_workspace_bytes(lr, n, C.byref(rp))
        fns[f"lerf_batchify_rays {s}+{ni}"] = lambda n, rp=rp: lib.nrf_lerf_batchify_rays_workspace_bytes(lr, n, 16, C.byref(rp))
        fns[f"lerf_head_backward {s + ni}"] = lambda n, sf=s + ni: lib.nrf_lerf_head_backward_workspace_bytes(lm, n, sf)
        fns[f"lerf_backward_points {s + ni}"] = lambda n, sf=s + ni: lib.nrf_lerf_backward_points_workspace_bytes(lr, n, sf)
        fns[f"normal_losses {s + ni}"] = lambda n, sf=s + ni: lib.nrf_normal_losses_workspace_bytes(n, sf)
        fns[f"ray_regularizers {s + ni}"] = lambda n, sf=s + ni: lib.nrf_ray_regularizers_workspace_bytes(n, sf)
    for prec in (0, 2):
        fns[f"lerf_head_relevancy {prec}"] = lambda n, prec=prec: lib.nrf_lerf_head_relevancy_workspace_bytes(lm, n, 3, prec)
        fns[f"lerf_point_relevancy {prec}"] = lambda n, prec=prec: lib.nrf_lerf_point_relevancy_workspace_bytes(lr, n, prec, 0)
    for name, fn in fns.items():
        sizes = [int(fn(n)) for n in range(1, 131)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])), (name, sizes)
        assert sizes[-1] > 0 or name.startswith("density_grad"), name
