"""The CLIP pyramid lookup on the MI355X (nrf_pyramid_*): pixel values bit for bit against the restatement of PyramidEmbedding::GetPixelValue in
tests/test_pyramid_host.py (NaN rows in the same places), the dataset's language targets, a LeRF training step fed them, the relevancy preview, and the
error paths."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_pyramid_host import Restated, geometry, max_zoom_out, random_pyramid, same_bits

pytestmark = pytest.mark.gpu

SCALES = (0.5, 1.0, 2.0, 0.25, 0.7, 3.0, 8.0)
BIG = dict(wh=[(800, 800)], clip=336, overlap=0.75)                     # 16 x 16 + 6 x 6 + 1 x 1 = 293 patches
SMALL = dict(wh=[(160, 96), (48, 40)], clip=32, overlap=0.5)             # non-square W 160 x H 96; the 48 x 40 view has no level 1 (MaxZoomOut is 1)


class _View:
    def __init__(self, W, H):
        self.W, self.H = W, H


def _device_pyramid(cfg, d, seed):
    from nerfpp_amd.pyramid import PyramidEmbedding, PyramidEmbedderProperties, MaxZoomOut
    emb = random_pyramid(cfg["wh"], cfg["clip"], cfg["overlap"], d, seed)
    views = [_View(w, h) for w, h in cfg["wh"]]
    props = PyramidEmbedderProperties(ImgSize=(cfg["clip"], cfg["clip"]), Overlap=cfg["overlap"], MaxZoomOut=MaxZoomOut(views, cfg["clip"]))
    pyr = PyramidEmbedding(props, emb).to_device(views)
    return pyr, Restated(emb, cfg["wh"], cfg["clip"], cfg["overlap"]), views


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from nerfpp_amd import _lib
    _lib.lib()
    return _lib


def _check_view(pyr, R, img, x, y, scales, lib):
    for scale in scales:
        got = pyr.GetPixelValue(_dev(x), _dev(y), scale, img).cpu().numpy()
        want = R.pixel_values(x, y, scale, img)
        assert same_bits(got, want), (img, scale, int(np.isnan(got).any(1).sum()), int(np.isnan(want).any(1).sum()))


@pytest.mark.parametrize("d", [768, 40])
def test_pixel_values_equal_the_restatement_bit_for_bit(gpu, d):
    rng = np.random.RandomState(d)
    # 800 x 800 at clip 336: random batches in get_batch's order (x = row, y = column) and every form of Interpolate
    pyr, R, _ = _device_pyramid(BIG, d, seed=10 + d)
    x, y = rng.randint(0, 800, 4096), rng.randint(0, 800, 4096)
    _check_view(pyr, R, 0, x, y, SCALES, gpu)
    for scale in (3.0, 8.0):                                      # both levels clamped to the top one, the scale above it: 0 / 0 in every row
        assert np.isnan(pyr.GetPixelValue(_dev(x[:64]), _dev(y[:64]), scale, 0).cpu().numpy()).all()
    pyr.close()
    # the non-square view: random batches and every pixel (the preview's x = column, y = row); the small view without level 1: the scales that do not need it
    pyr, R, _ = _device_pyramid(SMALL, d, seed=20 + d)
    x, y = rng.randint(0, 96, 3000), rng.randint(0, 160, 3000)
    _check_view(pyr, R, 0, x, y, SCALES, gpu)
    cols, rows = np.meshgrid(np.arange(160), np.arange(96))
    _check_view(pyr, R, 0, cols.reshape(-1), rows.reshape(-1), SCALES, gpu)
    cols, rows = np.meshgrid(np.arange(48), np.arange(40))
    _check_view(pyr, R, 1, cols.reshape(-1), rows.reshape(-1), (0.5, 0.25), gpu)
    # rows of a wider output (out_stride > D, an unaligned stride takes the scalar path)
    for extra in (4, 3):
        out = torch.full((500, d + extra), 7.0, device="cuda")
        pyr.GetPixelValue(_dev(x[:500]), _dev(y[:500]), 0.7, 0, out=out[:, :d])
        o = out.cpu().numpy()
        assert same_bits(o[:, :d], R.pixel_values(x[:500], y[:500], 0.7, 0)) and (o[:, d:] == 7.0).all()
    pyr.close()


def test_memory_bytes_is_the_sum_of_the_grids(gpu):
    for cfg, d in ((BIG, 768), (SMALL, 40)):
        pyr, _, _ = _device_pyramid(cfg, d, seed=1)
        mz = max_zoom_out(cfg["wh"], cfg["clip"])
        cells = 0
        for W, H in cfg["wh"]:
            for z in range(-1, mz + 1):
                _, nw, nh = geometry(W, H, cfg["clip"], cfg["overlap"], z)
                cells += nw * nh if nw > 0 and nh > 0 else 0
        assert pyr.memory_bytes() == cells * d * 4
        pyr.close()
    assert cells == 19 * 11 + 9 * 5 + 4 * 2 + 5 * 4 + 2 * 1      # SMALL: 160 x 96 levels -1, 0, 1 and 48 x 40 levels -1, 0 (its level 1 has no grid)


def _dataset(pyr_emb, d, batch, seed=3):
    from nerfpp_amd import scene
    from nerfpp_amd.dataset import View, NeRFDataset, LeRFDataParams
    views = [View(H=h, W=w, K=scene.lego_K(h, w), Pose=scene.pose_spherical(30.0 + 40 * i, -30.0, 4.0), Near=2.0, Far=6.0) for i, (w, h) in enumerate(SMALL["wh"])]
    lerf = LeRFDataParams(clip_input_img_size=SMALL["clip"], pyr_embedder_overlap=SMALL["overlap"], lang_embed_dim=d, pyramid=pyr_emb)
    return NeRFDataset(views, batch, seed=seed, lerf=lerf)


def test_get_batch_language_targets_follow_the_reference_argument_order(gpu):
    """get_batch passes x = rand_h, y = rand_w with img_size (W, H) (NeRFDataset.cpp:185-191): on the non-square view the swapped order reads other patches."""
    from nerfpp_amd.pyramid import PyramidEmbedding
    emb = random_pyramid(SMALL["wh"], SMALL["clip"], SMALL["overlap"], 40, seed=30)
    R = Restated(emb, SMALL["wh"], SMALL["clip"], SMALL["overlap"])
    ds = _dataset(PyramidEmbedding(embeddings=emb), 40, 2048)
    for it in (0, 2):                                             # iterations that use view 0 (the non-square one)
        ds.SetCurrentIter(it)
        b = ds.get_batch()
        rh, rw = b["rand_h"].cpu().numpy(), b["rand_w"].cpu().numpy()
        t = b["target_lang_embedding"]
        assert t.shape == (2048, 40) and t.dtype == torch.float32 and t.is_cuda
        got = t.cpu().numpy()
        assert same_bits(got, R.pixel_values(rh, rw, 0.5, 0))
        assert not same_bits(got, R.pixel_values(rw, rh, 0.5, 0))
    ds.SetCurrentIter(1)                                          # the 48 x 40 view at scale 0.5 needs levels -1 and 0 only
    b = ds.get_batch()
    assert same_bits(b["target_lang_embedding"].cpu().numpy(), R.pixel_values(b["rand_h"].cpu().numpy(), b["rand_w"].cpu().numpy(), 0.5, 1))
    # without LeRF parameters the batch is what it was
    from nerfpp_amd.dataset import NeRFDataset
    assert "target_lang_embedding" not in NeRFDataset(ds.Views, 16, seed=3).get_batch()


def test_lerf_training_step_fed_dataset_targets(gpu):
    """LeRFTrainer.step on a get_batch() ray batch: the loss of the dataset's device targets has the same bits as the loss of the restatement's targets."""
    from nerfpp_amd import scene, renderer as Rr, train as T
    from nerfpp_amd.pyramid import PyramidEmbedding
    emb = random_pyramid(SMALL["wh"], SMALL["clip"], SMALL["overlap"], 768, seed=40)
    R = Restated(emb, SMALL["wh"], SMALL["clip"], SMALL["overlap"])
    ds = _dataset(PyramidEmbedding(embeddings=emb), 768, 96)
    ds.SetCurrentIter(0)
    b = ds.get_batch()
    restated = _dev(R.pixel_values(b["rand_h"].cpu().numpy(), b["rand_w"].cpu().numpy(), 0.5, 0))
    losses = []
    for target in (b["target_lang_embedding"], restated):
        sc = scene.make_lerf_scene(log2_t=14, sigma_scale=20.0)
        p = Rr.NeRFRenderParams(NSamples=32, NImportance=32, Chunk=4096, Perturb=0.0, Ndc=False, UseViewdirs=False, ReturnWeights=True, ThinRay=True,
                                BoundingBox=sc["bbox"])
        tr = T.LeRFTrainer(sc["renderer"], sc["table"], sc["blob"], learning_rate=2e-3)
        loss, _ = tr.step(b["rays_o"], b["rays_d"], target, p)
        losses.append(loss.cpu().numpy().copy())
        tr.close()
    assert np.isfinite(losses[0]).all() and np.array_equal(losses[0].view(np.uint32), losses[1].view(np.uint32)), losses


def _cv_saturate_u8(v):
    """cv::saturate_cast<uchar>(float): cvRound = cvtss2si (round half to even; NaN and out-of-int32 values give INT_MIN), then clamp to [0, 255]."""
    v = np.asarray(v, np.float32)
    ok = (v >= np.float32(-2147483648.0)) & (v < np.float32(2147483648.0))
    iv = np.where(ok, np.rint(np.where(ok, v, 0)), -2147483648.0).astype(np.int64)
    return np.clip(iv, 0, 255).astype(np.uint8)


def test_relevancy_preview(gpu):
    """NeRFExecutor.h:803-831 for the non-square view: GetPixelValue(i, j, scale) -> Relevancy -> saturate_cast<uchar>(rel * 255) -> COLORMAP_JET."""
    from nerfpp_amd import renderer as Rr
    pyr, R, _ = _device_pyramid(SMALL, 768, seed=50)
    rng = np.random.RandomState(51)
    unit = lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)
    pos, neg = unit(rng.randn(2, 768)), unit(rng.randn(3, 768))
    cols, rows = np.meshgrid(np.arange(160), np.arange(96))
    lib = gpu.lib()
    assert cols[1, 2] == 2 and rows[1, 2] == 1                      # raster order: index j * W + i holds column i of row j
    for scale, chunk in ((0.5, 7), (0.7, 96), (8.0, 1)):
        gray, bgr = pyr.RelevancyPreview(0, pos, neg, scale=scale, positive_id=1, rows_per_chunk=chunk)
        emb = R.pixel_values(cols.reshape(-1), rows.reshape(-1), scale, 0)
        rel = Rr.Relevancy(_dev(emb), pos, neg, positive_id=1).cpu().numpy()
        want = _cv_saturate_u8(rel[:, 0] * np.float32(255)).reshape(96, 160)
        assert np.array_equal(gray.cpu().numpy(), want), scale
        ref_bgr = torch.empty((96 * 160, 3), device="cuda", dtype=torch.uint8)
        g = _dev(want.reshape(-1))
        gpu.check(lib.nrf_colormap_jet_u8(C.c_void_p(g.data_ptr()), C.c_int64(g.numel()), C.c_void_p(ref_bgr.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        assert np.array_equal(bgr.cpu().numpy().reshape(-1, 3), ref_bgr.cpu().numpy())
        if scale == 0.5:
            assert len(np.unique(want)) > 10
        if scale == 8.0:
            assert (want == 0).all()                                   # NaN rows -> NaN relevancy -> cvRound gives INT_MIN -> 0
    gray, bgr = pyr.RelevancyPreview(0, pos, neg, colored=False)
    assert bgr is None and gray.shape == (96, 160)
    pyr.close()


def test_invalid_calls_raise_and_leave_the_device_usable(gpu):
    from nerfpp_amd.pyramid import PyramidEmbedding
    L = gpu
    lib = L.lib()
    pyr, R, views = _device_pyramid(SMALL, 40, seed=60)
    x, y = _dev(np.arange(40, dtype=np.int64)), _dev(np.arange(40, dtype=np.int64)[::-1].copy())
    with pytest.raises(L.NrfError, match="level 1 of image 1"):
        pyr.GetPixelValue(x, y, 1.0, 1)                              # the 48 x 40 view has no level 1
    for bad in (2, -1):
        with pytest.raises(L.NrfError, match="outside"):
            pyr.GetPixelValue(x, y, 0.5, bad)
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(L.NrfError):
            pyr.GetPixelValue(x, y, scale, 0)
    with pytest.raises(L.NrfError, match="stride"):
        out = torch.empty((40, 40), device="cuda")
        L.check(lib.nrf_pyramid_pixel_values(pyr._p, 0, C.c_float(0.5), C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), C.c_int64(40), C.c_void_p(out.data_ptr()),
                                             C.c_int64(39), None))
    # D mismatch: entries of 40 floats for a pyramid of D = 768, and a raw call with the wrong width
    with pytest.raises(L.NrfError, match="D = 768"):
        PyramidEmbedding(pyr.Properties, R.emb).to_device(views, d=768)
    keys = np.array([[0, 0, 0, 0]], np.int32)
    row = np.zeros((1, 41), np.float32)
    with pytest.raises(L.NrfError, match="D = 40"):
        L.check(lib.nrf_pyramid_set_entries(pyr._p, C.c_int64(1), keys.ctypes.data_as(C.c_void_p), row.ctypes.data_as(C.c_void_p), 41, None))
    # keys outside an image's levels or grid
    for k in ([0, 0, 2, 0], [0, 0, 0, 2], [9, 0, 0, 0], [0, 3, 0, 1], [-1, 0, 0, 0]):
        with pytest.raises(L.NrfError):
            L.check(lib.nrf_pyramid_set_entries(pyr._p, C.c_int64(1), np.array([k], np.int32).ctypes.data_as(C.c_void_p), row[:, :40].copy().ctypes.data_as(C.c_void_p), 40, None))
    # a partly filled level is missing entries
    from test_pyramid_host import random_pyramid as rp
    part = {k: v for k, v in rp(SMALL["wh"], SMALL["clip"], SMALL["overlap"], 40, seed=61).items() if k != (1, 1, 0, 0)}
    p2 = PyramidEmbedding(pyr.Properties, part).to_device(views)
    with pytest.raises(L.NrfError, match="entries"):
        p2.GetPixelValue(x, y, 0.5, 0)
    p2.close()
    with pytest.raises(L.NrfError):
        pyr.RelevancyPreview(3, np.zeros((1, 40), np.float32), np.zeros((1, 40), np.float32))
    # the device still answers, and the pyramid is unchanged
    torch.cuda.synchronize()
    got = pyr.GetPixelValue(x, y, 0.7, 0).cpu().numpy()
    assert same_bits(got, R.pixel_values(np.arange(40), np.arange(40)[::-1], 0.7, 0))
    pyr.close()
