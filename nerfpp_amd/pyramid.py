"""Language targets of LeRF training from a cached CLIP pyramid -- PyramidEmbedding / PyramidEmbedderProperties (PyramidEmbedder.h:22-81, PyramidEmbedder.cpp:4-310).

The reference's dataset reads a per-pixel CLIP embedding out of `pyramid_embeddings.pt` on the host, one GetPixelValue call per batch pixel (NeRFDataset.cpp:180-193).
Here the cache is loaded once into device memory (nrf_pyramid_*) and a batch's targets are one library call.  Building a pyramid (RuCLIP over OpenCV tiles) is out of
scope: a PyramidEmbedding is read from the reference's file, or filled by the caller entry by entry.
"""
import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from .modules import _ptr, _stream


@dataclass
class PyramidEmbedderProperties:          # PyramidEmbedder.h:22-28
    ImgSize: Tuple[int, int] = (0, 0)    # the CLIP input size (clip_input_img_size, square: NeRFDataset.cpp:165)
    Overlap: float = 0.75
    MaxZoomOut: int = 1
    MinZoomOut: int = 1                   # carried as the reference does; the lookup does not read it


def _wh(views):
    return np.ascontiguousarray([[int(v.W), int(v.H)] for v in views], np.int32).reshape(-1, 2)


def MaxZoomOut(views, clip):
    """NeRFDataset.cpp:169-178: int(min(log2f(wmax / clip), log2f(hmax / clip))) with integer quotients over the views' sizes."""
    wh = _wh(views)
    out = C.c_int(0)
    L.check(L.lib().nrf_pyramid_max_zoom_out(wh.ctypes.data_as(C.c_void_p), len(wh), int(clip), C.byref(out)))
    return out.value


def LevelGeometry(img_w, img_h, clip, overlap, zoom):
    """(win, nw, nh) of one pyramid level (GetNearestPatchIndicesSingleScale, PyramidEmbedder.cpp:15-19); nw or nh <= 0: no grid at that level."""
    out = (C.c_int * 3)()
    L.check(L.lib().nrf_pyramid_level_geometry(int(img_w), int(img_h), int(clip), overlap, int(zoom), out))
    return tuple(out)


class PyramidEmbedding:
    """PyramidEmbedding (PyramidEmbedder.h:32-81).  Embeddings: {(hor_pos_idx, vert_pos_idx, zoom_out_idx, data_img_id): fp32 [1, D] host array}, the reference's
    std::map; to_device() uploads it, GetPixelValue() / RelevancyPreview() read it on the GPU."""

    def __init__(self, properties: Optional[PyramidEmbedderProperties] = None, embeddings=None):
        self.Embeddings = dict(embeddings or {})
        self.Properties = properties
        self._p, self._wh, self._d = None, None, 0

    # ---- the reference's cache file (PyramidEmbedder.cpp:199-223) ----
    def Save(self, path):
        """torch::save(std::vector<Tensor>): parameters "0", "1", ... alternating the int32 [4] key and the fp32 [1, D] embedding, in std::map key order."""
        from .checkpoint import save_tensor_list
        items = []
        for key in sorted(self.Embeddings):
            items.append(np.asarray(key, np.int32).reshape(4))
            items.append(np.asarray(self.Embeddings[key], np.float32).reshape(1, -1))
        save_tensor_list(path, items)

    def Load(self, path):
        """torch::load(std::vector<Tensor>) and the (key, embedding) pairs into Embeddings (a key read again replaces the earlier one, as the map assignment)."""
        from .checkpoint import load_tensor_list
        t = load_tensor_list(path)
        if len(t) % 2:
            raise ValueError(f"{path}: {len(t)} tensors, expected (key, embedding) pairs")
        for idx, emb in zip(t[0::2], t[1::2]):
            key = tuple(int(v) for v in np.asarray(idx).reshape(-1)[:4])
            self.Embeddings[key] = np.ascontiguousarray(emb, np.float32).reshape(1, -1)
        return self

    @property
    def D(self):
        return next(iter(self.Embeddings.values())).shape[-1] if self.Embeddings else 0

    # ---- device side ----
    def to_device(self, views, properties: Optional[PyramidEmbedderProperties] = None, d=None):
        """Upload Embeddings for `views` (records with .W, .H; data_img_id indexes this list) with `properties` (default: the constructor's) ImgSize, Overlap and
        MaxZoomOut.  d: the embedding width the caller expects (default: the entries'; entries of another width raise NrfError)."""
        if properties is None:
            properties = self.Properties
        assert properties is not None and properties.ImgSize[0] == properties.ImgSize[1] > 0, "a square CLIP input size is needed"
        self.close()
        wh = _wh(views)
        lib = L.lib()
        p = C.c_void_p()
        D = int(d if d is not None else self.D)
        L.check(lib.nrf_pyramid_create(D, int(properties.ImgSize[0]), properties.Overlap, int(properties.MaxZoomOut), len(wh), wh.ctypes.data_as(C.c_void_p), C.byref(p)))
        self._p, self.Properties, self._wh, self._d = p, properties, wh, D
        if self.Embeddings:
            keys = np.ascontiguousarray(list(self.Embeddings.keys()), np.int32).reshape(-1, 4)
            rows = [np.asarray(v, np.float32).reshape(-1) for v in self.Embeddings.values()]
            width = {r.size for r in rows}
            if len(width) != 1:
                raise L.NrfError(f"embeddings of several widths {sorted(width)}")
            emb = np.ascontiguousarray(np.stack(rows), np.float32)
            L.check(lib.nrf_pyramid_set_entries(p, len(keys), keys.ctypes.data_as(C.c_void_p), emb.ctypes.data_as(C.c_void_p), int(emb.shape[1]), _stream()))
        return self

    def memory_bytes(self):
        return int(L.lib().nrf_pyramid_memory_bytes(self._p))

    def close(self):
        if getattr(self, "_p", None):
            L.check(L.lib().nrf_pyramid_destroy(self._p))
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if not self._p:
            raise L.NrfError("PyramidEmbedding: call to_device() first")
        return self._p

    def GetPixelValue(self, x, y, scale, img_id, out=None):
        """GetPixelValue (PyramidEmbedder.cpp:230-310) for a batch: x, y int64 device tensors [n] (as the call site passes them: get_batch x = rand_h, y = rand_w;
        the preview x = column, y = row) -> [n, D] fp32 on the device (or into `out`, rows of any stride >= D)."""
        p = self._handle()
        xs, ys = x.to(torch.int64).contiguous(), y.to(torch.int64).contiguous()
        assert xs.is_cuda and ys.is_cuda and xs.shape == ys.shape, "x and y: int64 device tensors of one shape"
        n = xs.numel()
        D = self._d
        if out is None:
            out = torch.empty((n, D), device=xs.device, dtype=torch.float32)
        assert out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == n and out.stride(1) == 1
        L.check(L.lib().nrf_pyramid_pixel_values(p, int(img_id), scale, _ptr(xs), _ptr(ys), n, _ptr(out), out.stride(0), _stream()))
        return out

    def RelevancyPreview(self, img_id, positives, negatives, scale=0.5, positive_id=0, colored=True, rows_per_chunk=64):
        """The preview loop of NeRFExecutor::Train (NeRFExecutor.h:803-831) for view img_id -> (gray [H, W] uint8, bgr [H, W, 3] uint8 or None); the reference passes
        scale 0.5.  Phrase embeddings: [P, D] / [Q, D], host arrays or tensors.  Parity unpinned beyond the pixel values (OpenCV's cvRound and colormap, restated)."""
        p = self._handle()
        W, H = (int(v) for v in self._wh[int(img_id)]) if 0 <= int(img_id) < len(self._wh) else (0, 0)
        if not W:
            raise L.NrfError(f"image {img_id} is not a view of this pyramid")
        D = self._d

        def phrases(a):
            a = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, np.float32))
            a = a.to(device="cuda", dtype=torch.float32).contiguous()
            if a.shape[-1] != D:
                raise L.NrfError(f"phrase embeddings of width {a.shape[-1]} for a pyramid of D = {D}")
            return a.reshape(-1, D)
        pos, neg = phrases(positives), phrases(negatives)
        lib = L.lib()
        ws = torch.empty((int(lib.nrf_pyramid_relevancy_preview_workspace_bytes(p, int(img_id), int(rows_per_chunk))),), device="cuda", dtype=torch.uint8)
        gray = torch.empty((H, W), device="cuda", dtype=torch.uint8)
        bgr = torch.empty((H, W, 3), device="cuda", dtype=torch.uint8) if colored else None
        L.check(lib.nrf_pyramid_relevancy_preview(p, int(img_id), scale, _ptr(pos), int(pos.shape[0]), _ptr(neg), int(neg.shape[0]), int(positive_id),
                                                  _ptr(gray), _ptr(bgr), _ptr(ws), ws.numel(), _stream()))
        return gray, bgr
