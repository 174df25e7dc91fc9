"""Ray-batch producer of the training loop -- NeRFDataset::get_batch / GetRayBatch (NeRFDataset.cpp:44-65, :109-208) and the Blender
camera / bounds helpers the executor calls once per dataset (load_blender.h:83-124) -- SURVEY section 8f, row N2.

Image decoding, COLMAP / Blender file parsing and building the CLIP pyramid are out of scope (loaders); a view here is the already
decoded record the reference keeps in NeRFDatasetParams::Views: H, W, K [3,3], Pose [3|4, 4] and the image as an fp32 [H, W, 3] tensor.  With LeRF
parameters the batch also carries its language targets, read on the device from the pyramid's cache (nerfpp_amd/pyramid.py).
"""
import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from .modules import _ptr, _stream, _dev_f32
from .pyramid import PyramidEmbedderProperties, PyramidEmbedding, MaxZoomOut


@dataclass
class View:                       # NeRFDatasetParams::Views[i]
    H: int
    W: int
    K: np.ndarray                 # [3,3]
    Pose: np.ndarray              # [3,4] or [4,4] camera-to-world
    Image: Optional[torch.Tensor] = None      # [H, W, 3] fp32 on the GPU
    Near: float = 0.0
    Far: float = 0.0


@dataclass
class LeRFDataParams:             # LeRFDatasetParams (NeRFDatasetParams.h:177), the fields get_batch reads
    clip_input_img_size: int
    pyr_embedder_overlap: float
    lang_embed_dim: int
    pyramid: PyramidEmbedding     # the cache the reference loads from pyramid_embeddings.pt (NeRFDataset.cpp:96-98)


def _k9(K):
    return np.ascontiguousarray(K.detach().cpu().numpy() if torch.is_tensor(K) else K, np.float32).reshape(9)


def _m12(c2w):
    m = c2w.detach().cpu().numpy() if torch.is_tensor(c2w) else np.asarray(c2w)
    return np.ascontiguousarray(m[:3, :4], np.float32).reshape(12)


def GetRayBatch(rand_h, rand_w, H, W, K, c2w):
    """NeRFDataset::GetRayBatch (NeRFDataset.cpp:109-145): rand_h / rand_w int64 device tensors [N] -> rays_o [N,3], rays_d [N,3], cone_angle."""
    rh = rand_h.to(torch.int64).contiguous(); rw = rand_w.to(torch.int64).contiguous()
    assert rh.is_cuda and rw.is_cuda and rh.shape == rw.shape
    n = rh.numel()
    o = torch.empty((n, 3), device=rh.device, dtype=torch.float32); d = torch.empty_like(o)
    cone = C.c_float(0)
    k, m = _k9(K), _m12(c2w)
    L.check(L.lib().nrf_ray_batch(k.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p), _ptr(rh), _ptr(rw), n, _ptr(o), _ptr(d), C.byref(cone), _stream()))
    return o, d, torch.tensor(cone.value, dtype=torch.float32)


def CalculateBounds(h, w, current_iter, precorp_iters, precorp_frac):
    """NeRFDataset::CalculateBounds (NeRFDataset.cpp:44-65) -> (h_start, h_end, w_start, w_end), inclusive."""
    out = (C.c_int * 4)()
    L.check(L.lib().nrf_precrop_bounds(int(h), int(w), int(current_iter), int(precorp_iters), precorp_frac, out))
    return tuple(out)


class NeRFDataset:
    """The get_batch() side of NeRFDataset (NeRFDataset.cpp:148-208) for already decoded views.  The reference draws pixel coordinates
    with torch::randint from the global generator; here they are a pure function of (seed, iteration, element) (include/nrf_rng.h), so
    a training run is reproducible and a batch can be regenerated from its iteration number alone."""

    def __init__(self, views, batch_size, precorp_iters=0, precorp_frac=0.5, seed=0, lerf: Optional[LeRFDataParams] = None, patch_size=0):
        self.Views, self.BatchSize, self.PrecorpIters, self.PrecorpFrac, self.Seed = list(views), int(batch_size), int(precorp_iters), float(precorp_frac), int(seed)
        # patch_size P > 0: the batch is BatchSize / P^2 square patches of P x P neighbouring pixels (nrf_rand_patches), what a loss over neighbourhoods needs
        # (Trainer(ssim_loss_weight, patch_size)); 0: independent pixels, as the reference draws them
        self.PatchSize = int(patch_size)
        if self.PatchSize < 0 or (self.PatchSize > 0 and (self.BatchSize % (self.PatchSize * self.PatchSize) != 0 or self.BatchSize == 0)):
            raise L.NrfError(f"NeRFDataset: batch_size {self.BatchSize} is not a positive multiple of patch_size^2 = {self.PatchSize * self.PatchSize}")
        self.CurrentIter, self.CurrentImageIdx = 0, 0
        self.LeRFParams = lerf
        if lerf is not None:
            # InitializePyramidClipEmbedding (NeRFDataset.cpp:67-105): the properties get_batch builds (:164-178), the cache uploaded once
            clip = int(lerf.clip_input_img_size)
            self.PyramidProperties = PyramidEmbedderProperties(ImgSize=(clip, clip), Overlap=float(lerf.pyr_embedder_overlap),
                                                               MaxZoomOut=MaxZoomOut(self.Views, clip))
            lerf.pyramid.to_device(self.Views, self.PyramidProperties, d=int(lerf.lang_embed_dim))

    def SetCurrentIter(self, i):
        self.CurrentIter = int(i)
        self.CurrentImageIdx = int(i) % len(self.Views)       # the reference cycles through prefetched images (PrefetchNextImage)

    def get_batch(self):
        v = self.Views[self.CurrentImageIdx]
        h0, h1, w0, w1 = CalculateBounds(v.H, v.W, self.CurrentIter, self.PrecorpIters, self.PrecorpFrac)
        n = self.BatchSize
        rh = torch.empty((n,), device="cuda", dtype=torch.int64); rw = torch.empty_like(rh)
        if self.PatchSize > 0:
            P = self.PatchSize
            L.check(L.lib().nrf_rand_patches(self.Seed, self.CurrentIter, h0, h1, w0, w1, n // (P * P), P, _ptr(rh), _ptr(rw), _stream()))
        else:
            L.check(L.lib().nrf_rand_pixels(self.Seed, self.CurrentIter, h0, h1, w0, w1, n, _ptr(rh), _ptr(rw), _stream()))
        target = None
        if v.Image is not None:
            img = _dev_f32(v.Image)
            c = img.shape[-1]
            target = torch.empty((n, c), device=img.device, dtype=torch.float32)
            L.check(L.lib().nrf_gather_pixels(_ptr(img), v.H, v.W, c, _ptr(rh), _ptr(rw), n, _ptr(target), _stream()))
        o, d, cone = GetRayBatch(rh, rw, v.H, v.W, v.K, v.Pose)
        out = dict(rays_o=o, rays_d=d, cone_angle=cone, Near=v.Near, Far=v.Far, target_s=target, rand_h=rh, rand_w=rw)
        if self.PatchSize > 0:
            out["patch_size"] = self.PatchSize
        if self.LeRFParams is not None:
            # :180-193: GetPixelValue(rand_h, rand_w, 0.5f, CurrentImageIdx, ..., Size(W, H)) per pixel -- the row as x, as the reference passes it
            out["target_lang_embedding"] = self.LeRFParams.pyramid.GetPixelValue(rh, rw, 0.5, self.CurrentImageIdx)
        return out


def GetBoundsForObj(views):
    """load_blender.h:83-96: (near, far) = (0.15, 0.6) x the diagonal of the box around the training cameras' origins."""
    org = np.stack([np.asarray(v.Pose, np.float32)[:3, 3] for v in views])
    diff = (org.max(0) - org.min(0)).astype(np.float32)
    d = np.float32(np.sqrt(np.float32(np.sum(diff * diff, dtype=np.float32))))
    return float(np.float32(0.15 * float(d))), float(np.float32(0.6 * float(d)))


def GetBbox3dForObj(views):
    """load_blender.h:99-124: the box around o + Near*d and o + Far*d of the four corner rays of every training view."""
    mn = np.full(3, 1e8, np.float32); mx = np.full(3, -1e8, np.float32)
    for v in views:
        rh = torch.tensor([0, 0, v.H - 1, v.H - 1], device="cuda"); rw = torch.tensor([0, v.W - 1, 0, v.W - 1], device="cuda")
        o, d, _ = GetRayBatch(rh, rw, v.H, v.W, v.K, v.Pose)
        o, d = o.cpu().numpy(), d.cpu().numpy()
        for t in (np.float32(v.Near), np.float32(v.Far)):
            p = o + t * d
            mn = np.minimum(mn, p.min(0)); mx = np.maximum(mx, p.max(0))
    return np.concatenate([mn, mx]).astype(np.float32)
