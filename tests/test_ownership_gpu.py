"""Who owns the library's device memory, on the MI355X: nrf_device_bytes_in_use() counts every device byte the library holds in handles and scratch blocks (owned.h,
scratch.hip), so a handle that is created, used and destroyed must leave the counter where it was, a re-pack of the same shape must not move it, and
nrf_scratch_trim() must give back exactly what the scratch takers left behind -- a block left busy on some return path would stay counted.  Every assertion is an
exact equality of byte counts.  Nothing here provokes an error on the device; the error paths are covered on the host (test_owned_host.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LOG2_T = 14
CYCLES = 4


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from types import SimpleNamespace
    from nerfpp_amd import _lib as L, modules as M, renderer as R, scene as S
    return SimpleNamespace(L=L, M=M, R=R, S=S, lib=L.lib())


@pytest.fixture(scope="module")
def scenes(api):
    """The smallest built shape of each family (NeRFSmall 2 + 2 layers; the classic 8 x 256; the LeRF head 2 x 256 -> 768), tables of 2^14 entries."""
    S = api.S
    return dict(small=S.make_hash_scene(mode="cu", log2_t=LOG2_T, num_layers=2, num_layers_color=2), classic=S.make_classic_scene(), lerf=S.make_lerf_scene(log2_t=LOG2_T))


def P(t):
    return C.c_void_p(t.data_ptr())


def H(a):
    return a.ctypes.data_as(C.c_void_p)


def held(api):
    """Device bytes the library holds once nothing is in flight and its idle scratch blocks are given back."""
    torch.cuda.synchronize()
    api.lib.nrf_scratch_trim()
    return api.lib.nrf_device_bytes_in_use()


def mlp_family(api, scenes, family):
    """(create, blob, device-repack images the family reports) for nrf_mlp_*_create of the scene's network."""
    lib = api.lib
    if family == "small":
        return lib.nrf_mlp_small_create, scenes["small"]["mlp"].desc, scenes["small"]["mlp_blob"], lambda k: k >= 5
    if family == "classic":
        return lib.nrf_mlp_nerf_create, scenes["classic"]["mlp"].desc, scenes["classic"]["mlp_blob"], lambda k: k == 7
    return lib.nrf_mlp_lerf_create, scenes["lerf"]["lerf"].desc, scenes["lerf"]["blob"], lambda k: k == 3


@pytest.mark.parametrize("family", ["small", "classic", "lerf"])
def test_an_mlp_handle_gives_back_every_byte_and_repacks_in_place(api, scenes, family):
    L, lib = api.L, api.lib
    create, desc, blob, images_ok = mlp_family(api, scenes, family)
    blob = np.ascontiguousarray(blob, np.float32)
    d_blob = torch.from_numpy(blob * np.float32(0.5)).cuda()
    before = held(api)
    for cycle in range(CYCLES):
        m = C.c_void_p()
        L.check(create(C.byref(desc), H(blob), 0, None, C.byref(m)))
        assert images_ok(lib.nrf_mlp_device_repack_images(m)), (family, lib.nrf_mlp_device_repack_images(m))
        with_handle = held(api)
        assert with_handle > before
        L.check(lib.nrf_mlp_set_params(m, P(d_blob), 1, None))
        L.check(lib.nrf_mlp_set_params(m, H(blob), 0, None))
        assert held(api) == with_handle, f"{family}: two parameter uploads of the same shape re-pack in place"
        lib.nrf_mlp_destroy(m)
        assert held(api) == before, f"{family}: cycle {cycle}"


def test_a_hash_grid_gives_back_every_byte(api, scenes):
    L, lib = api.L, api.lib
    emb = scenes["small"]["embedder"]
    table = np.ascontiguousarray(scenes["small"]["table"], np.float32)
    desc = L.HashDesc(emb.mode, emb.NLevels, emb.NFeaturesPerLevel, emb.Log2HashmapSize, emb.BaseResolution, emb.FinestResolution, (C.c_float * 6)(*emb.BoundingBox.tolist()))
    before = held(api)
    for cycle in range(CYCLES):
        h = C.c_void_p()
        L.check(lib.nrf_hash_create(C.byref(desc), C.byref(h)))
        L.check(lib.nrf_hash_set_table(h, H(table), 0, None))          # from the host: the fp32 staging copy of the fp16 table's conversion
        torch.cuda.synchronize()
        assert lib.nrf_device_bytes_in_use() > before
        lib.nrf_hash_destroy(h)
        assert held(api) == before, f"cycle {cycle}"


def test_the_renderers_give_back_every_byte(api, scenes):
    L, S, R = api.L, api.S, api.R
    sc, ls = scenes["small"], scenes["lerf"]
    K = S.lego_K(8, 8)
    c2w = S.pose_spherical(30.0, -30.0, 4.0)
    rp = S.lego_render_params(sc["bbox"], chunk=32, precision=L.NRF_PREC_F16_MFMA)          # a matrix-core precision: the renderer creates its non-finite words
    rng = np.random.default_rng(7)
    E = ls["lerf"].GetLangEmbedDim()
    sc["renderer"].Render(8, 8, K, rp, c2w=c2w)          # whatever the scene's own handles create on their first render exists before the count is taken
    before = held(api)
    for cycle in range(CYCLES):
        r = R.NeRFRenderer(sc["embedder"], sc["embeddirs"], sc["mlp"])
        r.Render(8, 8, K, rp, c2w=c2w)
        torch.cuda.synchronize()
        r.__del__(); del r
        q = R.LeRFRenderer(ls["embedder"], ls["lerf"])
        assert q._r, "the scene's LeRF renderer is the library's"
        for n_pos, n_neg in ((1, 2), (2, 3)):          # prompts set twice, other sizes the second time
            q.SetLeRFPrompts(rng.standard_normal((n_pos, E)).astype(np.float32), rng.standard_normal((n_neg, E)).astype(np.float32))
        torch.cuda.synchronize()
        assert api.lib.nrf_device_bytes_in_use() > before
        q.__del__(); del q
        assert held(api) == before, f"cycle {cycle}"


def test_every_scratch_taker_gives_its_block_back(api, scenes):
    """One entry point per translation unit that takes scratch, at the smallest legal sizes; afterwards nrf_scratch_trim() returns exactly what the counter rose by.  A
    block still marked busy could not be trimmed: trim would then return less than the rise."""
    L, lib = api.L, api.lib
    f32 = lambda *shape: torch.rand(shape, device="cuda", dtype=torch.float32)
    before = held(api)
    # gemm_bf16x3.hip, as in test_library_scratch_blocks_are_reused_and_can_be_given_back
    M_, N_, K_ = 4096, 256, 256
    a, b, c = f32(M_, K_), f32(N_, K_), f32(M_, N_)
    L.check(lib.nrf_gemm_nt_f16x3(P(a), K_, C.c_int64(M_), K_, P(b), K_, N_, P(c), N_, None, 0, None))
    # train.hip
    pred, target, loss, grad = f32(8), f32(8), f32(2), f32(8)
    L.check(lib.nrf_huber_loss(P(pred), P(target), C.c_int64(8), P(loss), P(grad), None))
    # lerf_train.hip
    rows, tgt, rloss, rgrad = f32(2, 4), f32(2, 4), f32(1), f32(2, 4)
    L.check(lib.nrf_huber_rows_nanmean(P(rows), P(tgt), C.c_int64(2), 4, C.c_float(1.0), P(rloss), P(rgrad), None))
    # mlp.hip
    mlp = scenes["small"]["mlp"]
    x = f32(1, mlp.desc.input_ch + mlp.desc.input_ch_views)
    out = f32(1, mlp.GetOutputDims())
    L.check(lib.nrf_mlp_forward(mlp._m, P(x), C.c_int64(1), L.NRF_PREC_F32, P(out), None))
    # mlp_lerf_mfma.hip and mlp_lerf_split_mfma.hip: one embedding pass of one 32-sample ray in each precision
    lerf = scenes["lerf"]["lerf"]
    feats, w, emb = f32(32, lerf.desc.input_ch), f32(1, 32), f32(1, lerf.GetLangEmbedDim())
    for prec in (L.NRF_PREC_F16_MFMA, L.NRF_PREC_F16_SPLIT):
        L.check(lib.nrf_lerf_set_precision(lerf._m, prec))
        L.check(lib.nrf_lerf_render_embedding(lerf._m, P(feats), P(w), C.c_int64(1), 32, P(emb), None))
    torch.cuda.synchronize()
    rise = lib.nrf_device_bytes_in_use() - before
    assert rise > 0
    assert lib.nrf_scratch_trim() == rise
    assert lib.nrf_device_bytes_in_use() == before
