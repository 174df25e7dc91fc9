"""Density normals without a GPU: the float64 restatement of the density gradient (tests/normals_ref.py) against its own central differences, the ctypes
mirrors of the render structs against the header, and argument validation of the new entries."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from normals_ref import SigmaRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_scene(mode, n_levels=16, n_feat=2, log2_t=12, base=16, finest=512):
    """A make_hash_scene-shaped dict built on the host only (the library's level scales recomputed in numpy)."""
    from nerfpp_amd import scene
    table = scene.synth_hash_table(n_levels, log2_t, n_feat, 5000, 0.5)
    params = scene.synth_linear_stack(scene.small_shapes(n_levels * n_feat, 16, 3, 64, 15, 4, 64), 6000, 1.6, 0.0, {"sigma_net_2": 30.0})
    blob = np.concatenate([a.reshape(-1) for _, a in params])
    if mode == "cu":
        f = np.float32
        scales = np.array([np.exp2((np.log2(f(finest)) - np.log2(f(base))) * f(l) / f(n_levels - 1) + np.log2(f(base))) for l in range(n_levels)], np.float32)
    else:
        b = np.exp((np.log(finest) - np.log(base)) / (n_levels - 1))
        scales = np.array([np.floor(np.float32(base * b ** l)) for l in range(n_levels)], np.float32)
    primes = np.array(scene.CU_PRIMES[:3 * n_levels], np.int32) if mode == "cu" else None
    sc = dict(table=table, primes=primes, mlp_blob=blob, bbox=scene.LEGO_BBOX, mode=mode,
              cfg=dict(n_levels=n_levels, n_feat=n_feat, log2_t=log2_t, base=base, finest=finest))
    return sc, scales


def _face_distance(ref, pts):
    """smallest distance (in x units) from any point to a cell face of any level"""
    d = np.full(len(pts), np.inf)
    for l in range(ref.L):
        if ref.mode == "cu":
            fl, slope, wconst, _, _ = ref._cell(pts, l)
            ext = np.float64(ref.bbox[3] - ref.bbox[0])
            frac = np.minimum(wconst, 1 - wconst) / (np.float64(ref.scales[l]) / ext)
        else:
            fl, vmin, span, _, _ = ref._cell(pts, l)
            w = (pts - vmin) / span
            frac = np.minimum(w, 1 - w) * span
        d = np.minimum(d, frac.min(1))
    return d


@pytest.mark.parametrize("mode", ["cu", "ngp"])
def test_restatement_autograd_matches_central_differences(mode):
    import torch
    sc, scales = _host_scene(mode)
    ref = SigmaRef(sc, scales=scales)
    rng = np.random.default_rng(11)
    pts = rng.uniform(-1.45, 1.45, (400, 3)).astype(np.float32)
    pts = pts[_face_distance(ref, pts) > 1e-6][:128]
    assert len(pts) >= 32
    _, g, kink = ref.grad(pts, exact=False)
    h = 1e-9
    fd = np.zeros_like(g)
    x = pts.astype(np.float64)
    for a in range(3):
        e = np.zeros(3); e[a] = h
        sp = ref.sigma(torch.from_numpy(x + e), False)[0].numpy()
        sm = ref.sigma(torch.from_numpy(x - e), False)[0].numpy()
        fd[:, a] = (sp - sm) / (2 * h)
    ok = kink > 1e-6                  # a ReLU kink within the step would make the difference quotient meaningless
    assert ok.sum() >= 0.9 * len(pts)
    gn = np.linalg.norm(g[ok], axis=1)
    err = np.linalg.norm(fd[ok] - g[ok], axis=1)
    assert (gn > 0).all()
    assert (err <= 1e-5 * gn + 1e-6).all(), np.max(err / gn)


def _header_struct_fields(name):
    src = open(os.path.join(ROOT, "include", "nerfpp_hip.h")).read()
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [m.group(1) for m in re.finditer(r"(\w+)(?:\[\d+\])?;", body)]


def test_render_structs_keep_their_layout():
    """nrf_render_params / nrf_render_outputs are what callers compiled against the previous header hand the library: unchanged.  The normals request travels in
    nrf_render_normals beside them, through the *_normals entries."""
    from nerfpp_amd import _lib as L
    for cls, name in ((L.RenderParams, "nrf_render_params"), (L.RenderOutputs, "nrf_render_outputs"), (L.RenderNormals, "nrf_render_normals")):
        assert [f[0] for f in cls._fields_] == _header_struct_fields(name)
    assert L.RenderParams._fields_[-1] == ("overflow_policy", C.c_int)
    assert L.RenderOutputs._fields_[-1][0] == "d_z_fine" and C.sizeof(L.RenderOutputs) == 10 * 8
    assert [f[0] for f in L.RenderNormals._fields_] == ["bits", "d_normals", "d_pred_normals"] and C.sizeof(L.RenderNormals) == 24
    assert L.RenderNormals().bits == 0 and L.RenderNormals().d_normals is None
    for sym in ("nrf_density_grad", "nrf_density_grad_workspace_bytes", "nrf_render_rays_normals", "nrf_render_rays_normals_workspace_bytes",
                "nrf_batchify_rays_normals", "nrf_batchify_rays_normals_workspace_bytes", "nrf_render_rows_normals", "nrf_render_rows_normals_workspace_bytes"):
        assert sym in L.SYMBOLS, sym


def test_render_params_defaults_off():
    from nerfpp_amd.renderer import NeRFRenderer, NeRFRendererOutputs, NeRFRenderParams
    p = NeRFRenderParams()
    assert p.CalculateNormals is False and p.UsePredNormal is False
    assert NeRFRenderer._normal_bits(p) == 0
    assert NeRFRenderer._normal_bits(NeRFRenderParams(CalculateNormals=True, UsePredNormal=True)) == 3
    o = NeRFRendererOutputs()
    assert o.RenderedNormals is None and o.RenderedPredNormals is None


def test_entries_reject_bad_arguments():
    from nerfpp_amd import _lib as L
    lib = L.lib()
    fake = C.c_void_p(1 << 20)
    # a renderer needs a device, so a NULL one is the argument error to see here
    assert lib.nrf_density_grad(None, fake, C.c_int64(4), fake, fake, None, C.c_size_t(0), None) == 1
    assert b"nrf_density_grad" in lib.nrf_last_error()
    assert lib.nrf_density_grad_workspace_bytes(None, C.c_int64(1 << 20)) == 0
    p, o = L.RenderParams(), L.RenderOutputs()
    p.n_samples = 8
    nm = L.RenderNormals(L.NRF_NORMALS_DENSITY, None, None)
    assert lib.nrf_render_rays_normals(None, fake, 11, C.c_int64(4), C.byref(p), fake, None, C.byref(o), C.byref(nm), fake, C.c_size_t(1 << 30), None) == 1
    assert lib.nrf_batchify_rays_normals(None, fake, 11, C.c_int64(4), 4, C.byref(p), fake, None, C.byref(o), C.byref(nm), fake, C.c_size_t(1 << 30), None) == 1
    assert lib.nrf_render_rows_normals(None, None, C.byref(p), fake, None, C.byref(o), C.byref(nm), None, None, fake, C.c_size_t(1 << 30), None) == 1
    assert b"nrf_render_rows_normals" in lib.nrf_last_error()


def test_extract_mesh_rejects_unknown_normals():
    from nerfpp_amd import _lib as L
    from nerfpp_amd.mesh import ExtractMesh
    with pytest.raises(L.NrfError, match="lattice"):
        ExtractMesh(object(), 0.0, normals="sobel")
