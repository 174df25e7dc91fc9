"""LeRF relevancy in 3D on the MI355X: the head entry against the C oracle and the float64 restatement (tests/lerf_query_ref.py), points through the language grid,
lattice = points bit for bit, freshness of prompts and weights, interleaving with a training step's feature view, errors, and mesh labelling."""
import ctypes as C

import numpy as np
import pytest
import torch

import lerf_query_ref as Q
import mesh_ref as M

pytestmark = pytest.mark.gpu

BAR = {0: 1e-6, 1: 1e-2, 2: 1e-4}          # precision -> max abs error of the relevancy (F32 against the oracle chain, the fused modes against the float64 restatement)


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from nerfpp_amd import _lib as L, query, scene, mesh
    return L, query, scene, mesh


@pytest.fixture(scope="module")
def lerf_scene(api):
    L, query, scene, _ = api
    return scene.make_lerf_scene(log2_t=14)


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.uint32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _head(L, lerf, x, pos, neg, pid, prec, want_sigma=True, ws_bytes=None):
    lib = L.lib()
    p = x.shape[0]
    n_neg = neg.shape[0] if neg is not None else 0
    need = int(lib.nrf_lerf_head_relevancy_workspace_bytes(lerf._m, C.c_int64(p), n_neg, prec))
    ws = torch.empty((max(1, need if ws_bytes is None else ws_bytes),), device="cuda", dtype=torch.uint8)
    rel = torch.full((max(p, 1), 2), float("nan"), device="cuda")
    sig = torch.full((max(p, 1),), float("nan"), device="cuda") if want_sigma else None
    rc = lib.nrf_lerf_head_relevancy(lerf._m, C.c_void_p(x.data_ptr()), C.c_int64(p), C.c_void_p(pos.data_ptr()), int(pos.shape[0]),
                                     C.c_void_p(neg.data_ptr()) if n_neg else None, n_neg, pid, prec, C.c_void_p(sig.data_ptr()) if sig is not None else None,
                                     C.c_void_p(rel.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_size_t(ws.numel() if ws_bytes is None else ws_bytes), None)
    torch.cuda.synchronize()
    return rc, rel[:p], (sig[:p] if sig is not None else None)


def _prompts(n_pos, n_neg, seed):
    return Q.unit_prompts(n_pos, seed), Q.unit_prompts(n_neg, seed + 1)


# ------------------------------------------------------------------------------------ 1. the head against the oracle
@pytest.mark.parametrize("n_neg", [0, 1, 4, 31])
@pytest.mark.parametrize("positive_id", [0, 2])
@pytest.mark.parametrize("prec", [0, 1, 2])
def test_head_relevancy_against_oracle_and_restatement(api, manifest, prec, n_neg, positive_id):
    from oracle import capi as O
    from nerfpp_amd import synth
    from nerfpp_amd.modules import LeRF
    L = api[0]
    g = np.load(str(__import__("os").path.join(__import__("os").path.dirname(__file__), "golden", "lerf.npz")))
    blob = synth.blob_from_manifest(manifest["lerf"])
    lerf = LeRF(32, 2, 256, 768, 128, "lang_model", params=blob)
    pos, neg = _prompts(3, n_neg, 40 + n_neg)
    rc, rel, sig = _head(L, lerf, _dev(g["x"]), _dev(pos), _dev(neg), positive_id, prec)
    assert rc == 0, L.lib().nrf_last_error()
    rel = rel.cpu().numpy().astype(np.float64)
    if prec == 0:
        ref = O.relevancy(O.lerf(blob, g["x"])[:, :768], pos, neg.reshape(-1, 768), positive_id)
    else:
        ref = Q.relevancy_projection(blob, g["x"], pos, neg, positive_id).numpy()
    err = np.abs(rel - ref).max()
    print(f"head precision {prec} n_neg {n_neg} id {positive_id}: max abs error {err:.3e}")
    assert err <= BAR[prec]
    assert np.array_equal(_bits(sig), O.lerf_sigma_net(blob, g["x"])[:, 0].view(np.uint32))


# ------------------------------------------------------------------------------------ 2. points through the language grid
def _points(sc, p, seed):
    bb = np.asarray(sc["bbox"], np.float32)
    c, h = (bb[:3] + bb[3:]) / 2, (bb[3:] - bb[:3]) / 2
    return (c + 1.1 * h * np.random.default_rng(seed).uniform(-1, 1, (p, 3))).astype(np.float32)


@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("p", [0, 1, 31, 33, (1 << 16) + 5])
def test_point_relevancy_sigma_bits_and_relevancy_bars(api, lerf_scene, prec, p):
    L, query, _, _ = api
    sc = lerf_scene
    r = sc["renderer"]
    pos, neg = _prompts(2, 5, 7)
    r.SetLeRFPrompts(pos, neg)
    pts = _dev(_points(sc, p, 3 + p)) if p else torch.empty((0, 3), device="cuda")
    rel, sig = query.PointRelevancy(r, pts, positive_id=1, precision=prec, return_sigma=True)
    assert rel.shape == (p, 2) and sig.shape == (p,)
    if p == 0:
        return
    x, keep = r.LangEmbedFn.forward(pts)
    assert not bool(keep.all()), "some points must fall outside the box"
    raw = sc["lerf"].forward(x)
    ref_sig = torch.where(keep, raw[:, -1], torch.zeros_like(raw[:, -1]))
    assert np.array_equal(_bits(sig), _bits(ref_sig))
    ref = Q.relevancy_projection(sc["blob"], x.cpu().numpy(), pos, neg, 1).numpy()
    err = np.abs(rel.cpu().numpy().astype(np.float64) - ref).max()
    print(f"points precision {prec} p {p}: max abs error {err:.3e}")
    assert err <= (2e-6 if prec == 0 else BAR[prec])


# ------------------------------------------------------------------------------------ 3. lattice == points
@pytest.mark.parametrize("prec", [1, 2, 0])
def test_grid_equals_points_bit_for_bit(api, lerf_scene, prec):
    L, query, _, _ = api
    sc = lerf_scene
    r = sc["renderer"]
    r.SetLeRFPrompts(*_prompts(1, 4, 11))
    nx, ny, nz = 19, 13, 11
    bb = sc["bbox"] * np.float32(1.05)
    pts = _dev(M.lattice_points(bb, nx, ny, nz).reshape(-1, 3))
    rel_p, sig_p = query.PointRelevancy(r, pts, precision=prec, return_sigma=True)
    for slab in (None, 1, 997):
        rel, sig = query.RelevancyGrid(r, bb, (nx, ny, nz), precision=prec, slab_points=slab)
        assert rel.shape == (nz, ny, nx, 2) and sig.shape == (nz, ny, nx)
        assert np.array_equal(_bits(rel.reshape(-1, 2)), _bits(rel_p)), slab
        assert np.array_equal(_bits(sig.reshape(-1)), _bits(sig_p)), slab
    again = query.RelevancyGrid(r, bb, (nx, ny, nz), precision=prec)
    assert np.array_equal(_bits(again[0]), _bits(rel)) and np.array_equal(_bits(again[1]), _bits(sig))
    rel_s, _ = query.PointRelevancy(r, pts, precision=prec, return_sigma=True, slab_points=64)
    assert np.array_equal(_bits(rel_s), _bits(rel_p))


# ------------------------------------------------------------------------------------ 4. freshness
def test_results_follow_prompts_and_parameter_uploads(api):
    L, query, scene, _ = api
    from nerfpp_amd import train as T
    from nerfpp_amd.renderer import NeRFRenderParams, GetRays
    sc = scene.make_lerf_scene(log2_t=14)
    r = sc["renderer"]
    pts = _dev(_points(sc, 777, 5))
    x = r.LangEmbedFn.forward(pts)[0].cpu().numpy()
    pa, na = _prompts(1, 3, 100)
    pb, nb = _prompts(1, 6, 200)
    r.SetLeRFPrompts(pa, na)
    ra = query.PointRelevancy(r, pts).cpu().numpy()
    assert np.abs(ra - Q.relevancy_projection(sc["blob"], x, pa, na).numpy()).max() <= BAR[2]
    r.SetLeRFPrompts(pb, nb)
    rb = query.PointRelevancy(r, pts).cpu().numpy()
    assert np.abs(rb - Q.relevancy_projection(sc["blob"], x, pb, nb).numpy()).max() <= BAR[2]
    assert np.abs(ra - rb).max() > 1e-3
    # one training step uploads new parameters (head and grid)
    K = scene.lego_K(800, 800); c2w = scene.pose_spherical(30.0, -30.0, 4.0)
    o, d, _ = GetRays(800, 800, K, c2w, row0=400, rows=1)
    o = o.reshape(-1, 3)[200:456].contiguous(); d = d.reshape(-1, 3)[200:456].contiguous()
    p = NeRFRenderParams(NSamples=32, NImportance=32, Chunk=4096, Perturb=0.0, Ndc=False, UseViewdirs=False, ThinRay=True, BoundingBox=sc["bbox"])
    tgt = np.random.RandomState(3).randn(o.shape[0], 768).astype(np.float32)
    tgt /= np.linalg.norm(tgt, axis=1, keepdims=True)
    tr = T.LeRFTrainer(r, sc["table"], sc["blob"], learning_rate=5e-2)
    tr.step(o, d, _dev(tgt), p)
    torch.cuda.synchronize()
    blob2 = tr.blob.cpu().numpy()
    assert not np.array_equal(blob2, sc["blob"])
    x2 = r.LangEmbedFn.forward(pts)[0].cpu().numpy()
    rc = query.PointRelevancy(r, pts).cpu().numpy()
    ref2 = Q.relevancy_projection(blob2, x2, pb, nb).numpy()
    assert np.abs(rc - ref2).max() <= BAR[2]
    rc32 = query.PointRelevancy(r, pts, precision=L.NRF_PREC_F32).cpu().numpy()
    assert np.abs(rc32 - ref2).max() <= 2e-6
    tr.close()


# ------------------------------------------------------------------------------------ 5. interleaving with a training step's feature view
def test_query_between_render_and_backward_keeps_the_feature_view(api):
    L, query, scene, _ = api
    from nerfpp_amd import train as T
    from nerfpp_amd.renderer import NeRFRenderParams, GetRays
    sc = scene.make_lerf_scene(log2_t=14)
    r = sc["renderer"]
    r.SetLeRFPrompts(*_prompts(1, 3, 9))
    K = scene.lego_K(800, 800); c2w = scene.pose_spherical(30.0, -30.0, 4.0)
    o, d, _ = GetRays(800, 800, K, c2w, row0=400, rows=1)
    o = o.reshape(-1, 3)[200:584].contiguous(); d = d.reshape(-1, 3)[200:584].contiguous()
    p = NeRFRenderParams(NSamples=32, NImportance=32, Chunk=4096, Perturb=0.0, Ndc=False, UseViewdirs=False, ReturnWeights=True, ThinRay=True, BoundingBox=sc["bbox"],
                         KeepIntermediates=True)
    tgt = np.random.RandomState(12).randn(o.shape[0], 768).astype(np.float32)
    tgt /= np.linalg.norm(tgt, axis=1, keepdims=True)
    tr = T.LeRFTrainer(r, sc["table"], sc["blob"], learning_rate=2e-3)
    got = []
    for with_query in (False, True):
        res = r.Render(0, 0, None, p, rays=(o, d, None))
        if with_query:
            query.RelevancyGrid(r, resolution=24)
        tr.backward(res, _dev(tgt), p)
        assert tr.reused_render_features is True
        got.append((tr.g_blob.clone(), tr.g_table.clone()))
    assert np.array_equal(_bits(got[0][0]), _bits(got[1][0])) and np.array_equal(_bits(got[0][1]), _bits(got[1][1]))
    tr.close()


# ------------------------------------------------------------------------------------ 6. errors
def test_errors(api, lerf_scene, manifest):
    L, query, scene, _ = api
    lib = L.lib()
    sc = scene.make_lerf_scene(log2_t=14)
    r = sc["renderer"]
    pts = _dev(_points(sc, 100, 1))
    rel = torch.empty((100, 2), device="cuda")
    ws = torch.empty((1 << 20,), device="cuda", dtype=torch.uint8)

    def point(pid=0, prec=2, out=rel, wsb=None, p=100):
        need = int(lib.nrf_lerf_point_relevancy_workspace_bytes(r._r, C.c_int64(p), prec, C.c_int64(0)))
        w = torch.empty((max(need, 1),), device="cuda", dtype=torch.uint8)
        return lib.nrf_lerf_point_relevancy(r._r, C.c_void_p(pts.data_ptr()), C.c_int64(p), pid, prec, None, C.c_void_p(out.data_ptr()) if out is not None else None,
                                            C.c_int64(0), C.c_void_p(w.data_ptr()), C.c_size_t(need if wsb is None else wsb), None)
    r.SetLeRFPrompts(None, None)
    assert point() == 1                                              # no prompts
    bb = np.ascontiguousarray(sc["bbox"], np.float32)
    assert lib.nrf_lerf_relevancy_grid(r._r, bb.ctypes.data_as(C.c_void_p), 4, 4, 4, 0, 2, None, C.c_void_p(rel.data_ptr()), C.c_int64(0),
                                       C.c_void_p(ws.data_ptr()), C.c_size_t(ws.numel()), None) == 1
    r.SetLeRFPrompts(*_prompts(2, 3, 5))
    assert point(pid=2) == 1 and point(pid=-1) == 1                  # positive_id out of range
    assert point(out=None) == 1                                      # NULL relevancy
    assert point(wsb=1024) == 4                                      # workspace too small
    assert point(p=0) == 0                                           # nothing to do
    assert point() == 0
    # 1 + n_neg = 33: unsupported in the fused modes, F32 still works
    r.SetLeRFPrompts(*_prompts(1, 32, 6))
    for prec in (1, 2):
        assert point(prec=prec) == 3, prec
    assert point(prec=0) == 0
    torch.cuda.synchronize()
    assert np.isfinite(rel.cpu().numpy()).all()
    # the head entry: the same rules
    from nerfpp_amd import synth
    from nerfpp_amd.modules import LeRF
    lerf = LeRF(32, 2, 256, 768, 128, "lang_model", params=synth.blob_from_manifest(manifest["lerf"]))
    x = torch.zeros((8, 128), device="cuda")
    pos, neg = _dev(Q.unit_prompts(2, 1)), _dev(Q.unit_prompts(32, 2))
    assert _head(L, lerf, x, pos, neg, 0, 2)[0] == 3
    assert _head(L, lerf, x, pos, neg, 0, 0)[0] == 0
    assert _head(L, lerf, x, pos, neg[:4], 2, 2)[0] == 1
    assert _head(L, lerf, x, pos, neg[:4], 0, 2, ws_bytes=256)[0] == 4
    assert _head(L, lerf, x[:0], pos, neg[:4], 0, 2)[0] == 0


# ------------------------------------------------------------------------------------ 7. meshes and LocateQuery
def test_vertex_relevancy_and_locate_query(api, lerf_scene):
    L, query, scene, mesh = api
    sc = lerf_scene
    r = sc["renderer"]
    r.SetLeRFPrompts(*_prompts(1, 4, 21))
    hs = scene.make_hash_scene(mode="cu", log2_t=14)
    dg = mesh.DensityGrid(hs["renderer"], resolution=40)
    m = mesh.ExtractMesh(hs["renderer"], float(dg.reshape(-1).quantile(0.7).item()), resolution=40, colors=False)
    assert m.Vertices.shape[0] > 0
    vr = query.VertexRelevancy(r, m)
    assert np.array_equal(_bits(vr), _bits(query.PointRelevancy(r, m.Vertices)))
    seg = query.SegmentMesh(m, vr, float(vr[:, 0].median()))
    assert seg.Faces.shape[0] <= m.Faces.shape[0] and seg.Relevancy.shape == (seg.Vertices.shape[0], 2)
    res = 32
    rel, sig = query.RelevancyGrid(r, resolution=res)
    thr = float(sig.reshape(-1).float().quantile(0.5).item())
    loc = query.LocateQuery(r, resolution=res, sigma_threshold=thr, top_k=5)
    want = Q.locate(rel.cpu().numpy(), sig.cpu().numpy(), thr, 5)
    assert loc["indices"].cpu().numpy().tolist() == want.tolist()
    assert np.array_equal(_bits(loc["relevancy"]), _bits(rel.reshape(-1, 2)[torch.from_numpy(want).cuda()]))
    grid_pts = M.lattice_points(sc["bbox"], res, res, res).reshape(-1, 3)
    assert np.array_equal(loc["positions"].cpu().numpy(), grid_pts[want])
    none = query.LocateQuery(r, resolution=res, sigma_threshold=float("inf"), top_k=5)
    assert none["indices"].numel() == 0 and none["positions"].shape == (0, 3)
