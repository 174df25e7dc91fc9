"""The Chunk loop both renderers share, on the MI355X: the LeRF loop on 2 and 4 lanes against its single-stream loop, and the feature-view protocol
(nrf_renderer_last_features / nrf_lerf_renderer_last_features: serial, valid after one chunk, none after several) on both renderers at the same shapes."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NRF_OK, NRF_ERR_UNSUPPORTED = 0, 3
# the smallest sample counts nrf_lerf_batchify_rays accepts (lerf_plan: n_samples and n_samples + n_importance are multiples of 32, n_samples >= 32); 8 + 8 is
# refused with NRF_ERR_INVALID_ARG before any chunk is issued
S, NI = 32, 32
CHUNK = 64


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from nerfpp_amd import _lib as L, renderer as R, scene
    return L, R, scene


@pytest.fixture(scope="module")
def rays(api):
    _, R, scene = api
    K = scene.lego_K(800, 800); c2w = scene.pose_spherical(30.0, -30.0, 4.0)
    o, d, _ = R.GetRays(800, 800, K, c2w, row0=400, rows=1)
    return o.reshape(-1, 3)[200:520].contiguous(), d.reshape(-1, 3)[200:520].contiguous()          # 320 rays across the object


@pytest.fixture(scope="module")
def lerf_scene(api):
    sc = api[2].make_lerf_scene(log2_t=14)
    rng = np.random.RandomState(86)
    pos = rng.randn(1, 768).astype(np.float32); pos /= np.linalg.norm(pos)
    neg = rng.randn(3, 768).astype(np.float32); neg /= np.linalg.norm(neg, axis=1, keepdims=True)
    sc["renderer"].SetLeRFPrompts(pos, neg)
    return sc


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.uint32)


def _last_features(fn, r):
    """(status, view, serial) of nrf_renderer_last_features / nrf_lerf_renderer_last_features on the renderer's handle."""
    fp, kp, sp = C.c_void_p(), C.c_void_p(), C.c_void_p()
    cols, nn, sf, ser = C.c_int64(), C.c_int64(), C.c_int(), C.c_uint64()
    rc = fn(r._r, C.byref(fp), C.byref(cols), C.byref(kp), C.byref(sp), C.byref(nn), C.byref(sf), C.byref(ser))
    return rc, dict(feats=fp.value, cols=int(cols.value), keep=kp.value, src=sp.value, n=int(nn.value), sf=int(sf.value)), int(ser.value)


def _lerf_params(R, sc, chunk=CHUNK):
    return R.NeRFRenderParams(NSamples=S, NImportance=NI, Chunk=chunk, Perturb=0.0, Ndc=False, UseViewdirs=False, ReturnWeights=True, ThinRay=True, BoundingBox=sc["bbox"],
                              KeepIntermediates=True)


def _lerf_fields(res):
    o = res.Outputs
    return dict(embedding=o.RenderedLangEmbedding, relevancy=o.Relevancy, depth=o.DepthMapLE, disp=o.DispMapLE, acc=o.AccMapLE, weights=o.WeightsLE, z_fine=res.Extras["z_fine"])


def test_lerf_chunk_loop_lanes_reproduce_the_single_stream_loop(api, rays, lerf_scene):
    """nrf_lerf_batchify_rays on 2 and 4 lanes against 1 lane, 320 rays (five chunks of 64: the lanes get 3 + 2 chunks, with 4 lanes one lane wraps) and 300 rays (a
    short last chunk): embedding, relevancy, depth / disp / acc, weights and z_fine bit for bit -- the same kernels on the same slices.  After each of these calls
    nrf_lerf_renderer_last_features answers NRF_ERR_UNSUPPORTED; after a one-chunk call NRF_OK with n == 64 and a larger serial.  32 + 32 samples: the smallest counts
    the entry accepts (8 + 8 is NRF_ERR_INVALID_ARG in lerf_plan)."""
    L, R, _ = api
    sc = lerf_scene
    r = sc["renderer"]
    fn = L.lib().nrf_lerf_renderer_last_features
    p = _lerf_params(R, sc)
    assert r._single_call_ok(p), "the batch must go through nrf_lerf_batchify_rays"
    o, d = rays
    lanes0 = r.lanes
    try:
        for n in (320, 300):
            ref = None
            for lanes in (1, 2, 4):
                r.lanes = lanes
                res = r.Render(0, 0, None, p, rays=(o[:n], d[:n], None))
                torch.cuda.synchronize()
                rc, _, _ = _last_features(fn, r)
                assert rc == NRF_ERR_UNSUPPORTED, (n, lanes, rc)
                assert res.FeatureView is None
                got = {k: _bits(v) for k, v in _lerf_fields(res).items()}
                if ref is None:
                    ref = got
                    assert got["embedding"].shape == (n, 768) and got["weights"].shape == (n, S + NI) and got["z_fine"].shape == (n, S + NI)
                    assert np.isfinite(got["embedding"].view(np.float32)).all() and float(np.abs(got["weights"].view(np.float32)).max()) > 0
                    continue
                for k in ref:
                    assert np.array_equal(got[k], ref[k]), (k, n, lanes)
        for lanes in (1, 4):
            r.lanes = lanes
            _, _, before = _last_features(fn, r)
            r.Render(0, 0, None, p, rays=(o[:64], d[:64], None))
            rc, v, after = _last_features(fn, r)
            assert rc == NRF_OK and v["n"] == 64 and after > before, (lanes, rc, v, before, after)
    finally:
        r.lanes = lanes0


def test_feature_view_protocol_is_the_same_on_both_renderers(api, rays, lerf_scene):
    """The NeRF renderer (CuHashEmbedder grid, the feature-reusing fast path) and the LeRF renderer at the same shapes: each chunk rendered advances the serial by exactly
    one, a one-chunk call leaves a valid view with cols == n * sf, a two-chunk call leaves none."""
    L, R, scene = api
    lib = L.lib()
    o, d = rays
    hs = scene.make_hash_scene(mode="cu", log2_t=14)
    p_nerf = R.NeRFRenderParams(NSamples=S, NImportance=NI, Chunk=CHUNK, Perturb=0.0, WhiteBkgr=False, Ndc=False, UseViewdirs=True, ThinRay=True, BoundingBox=hs["bbox"],
                                Precision=L.NRF_PREC_F16_SPLIT)
    cases = [("nerf", hs["renderer"], lib.nrf_renderer_last_features, p_nerf),
             ("lerf", lerf_scene["renderer"], lib.nrf_lerf_renderer_last_features, _lerf_params(R, lerf_scene))]
    for name, r, fn, p in cases:
        _, _, serial = _last_features(fn, r)
        for n, chunks in ((64, 1), (128, 2), (320, 5), (300, 5), (1, 1)):
            res = r.Render(0, 0, None, p, rays=(o[:n], d[:n], None))
            rc, v, now = _last_features(fn, r)
            assert now == serial + chunks, (name, n, serial, now)
            serial = now
            if chunks == 1:
                assert rc == NRF_OK and v["n"] == n and v["sf"] == S + NI and v["cols"] == n * (S + NI), (name, n, rc, v)
                assert v["feats"] and v["keep"] and v["src"]
                assert res.FeatureView is not None and res.FeatureView["serial"] == now
            else:
                assert rc == NRF_ERR_UNSUPPORTED, (name, n, rc)
                assert res.FeatureView is None
    torch.cuda.synchronize()
