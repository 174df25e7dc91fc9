"""The CLIP pyramid lookup on the host side (no GPU): level geometry and MaxZoomOut of the library against a restatement of the reference's arithmetic, the
pyramid_embeddings.pt round trip, and known answers of the restatement itself.

There is no golden of the compiled reference here (PyramidEmbedder.cpp needs OpenCV and RuCLIP), so the lookup is pinned by a RESTATEMENT of
PyramidEmbedding::GetPixelValue (PyramidEmbedder.cpp:4-310) with the reference's own types: index math in numpy float32 / float64 / int exactly where the C++
mixes them, log2f through the C library, and the interpolation as ATen fp32 ops on torch CPU tensors in the reference's order (ATen is the reference's arithmetic
substrate).  tests/test_pyramid_gpu.py holds the device kernel to it bit for bit."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest
import torch

F32 = np.float32
_libm = C.CDLL(ctypes.util.find_library("m"))
_libm.log2f.restype = C.c_float
_libm.log2f.argtypes = [C.c_float]


def log2f(v):
    return F32(_libm.log2f(float(F32(v))))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def geometry(img_w, img_h, clip, overlap, zoom):
    """(win, nw, nh): :15-19.  window = int(clip * pow(2, zoom)); n = int(float32(img - float32(win * Overlap)) / (win * (1. - Overlap)))."""
    win = int(clip * 2.0 ** zoom)
    ov = F32(overlap)

    def count(img):
        num = F32(F32(img) - F32(F32(win) * ov))
        return int(np.float64(num) / (np.float64(win) * (1.0 - np.float64(ov))))
    return win, count(img_w), count(img_h)


def max_zoom_out(wh, clip):
    """NeRFDataset.cpp:169-178 over views [(W, H), ...]: integer quotients, log2f, min, stored into an int."""
    wmax = max(w for w, _ in wh)
    hmax = max(h for _, h in wh)
    return int(min(log2f(wmax // clip), log2f(hmax // clip)))


def levels_for_scale(scale, mz):
    """:97-113 and :300-307 -> (z1, z2, zoom as float32, which: 1 = e1, 2 = e2, 3 = lerp)."""
    zoom = log2f(scale)
    z1 = int(zoom)
    z1 = min(max(z1, -1), mz)
    z2 = min(max(z1 + 1, -1), mz)
    which = 2 if zoom == F32(z2) else 1 if zoom == F32(z1) else 3
    return z1, z2, zoom, which


def centres(idx, win, overlap):
    """:47-60: float(int(idx * win * (1. - Overlap))) + win / 2 (integer division)."""
    c = (np.asarray(idx, np.int64) * win).astype(np.float64) * (1.0 - np.float64(F32(overlap)))
    return c.astype(np.int64).astype(F32) + F32(win // 2)


def indices(coord, win, n, overlap):
    """:21-45 along one axis: pos = coord / win / (1.f - Overlap) in float32; idx1 = int(pos - 2), idx2 = int(pos - 1), clamped to [0, n - 1]."""
    omo = F32(F32(1.0) - F32(overlap))
    pos = (coord / F32(win)).astype(F32) / omo
    i1 = (pos - F32(2)).astype(F32).astype(np.int64)
    i2 = (pos - F32(1)).astype(F32).astype(np.int64)
    clamp = lambda i: np.where(np.where(i < 0, 0, i) >= n, n - 1, np.where(i < 0, 0, i))
    return clamp(i1), clamp(i2)


class Restated:
    """PyramidEmbedding::GetPixelValue over the pyramid `emb` {(hor, vert, zoom, img): [1, D]}, views [(W, H), ...]."""

    def __init__(self, emb, wh, clip, overlap, mz=None):
        self.emb, self.wh, self.clip, self.overlap = emb, list(wh), clip, overlap
        self.mz = max_zoom_out(self.wh, clip) if mz is None else mz
        self._tables = {}

    def table(self, zoom, img):
        """[nh * nw, D] fp32 torch rows of one level, row v * nw + h; KeyError on a missing entry (the reference's undefined tensor)."""
        key = (zoom, img)
        if key not in self._tables:
            W, H = self.wh[img]
            win, nw, nh = geometry(W, H, self.clip, self.overlap, zoom)
            if nw <= 0 or nh <= 0:
                raise KeyError(f"level {zoom} of image {img} has no grid")
            rows = [np.asarray(self.emb[(h, v, zoom, img)], F32).reshape(-1) for v in range(nh) for h in range(nw)]
            self._tables[key] = torch.from_numpy(np.stack(rows))
        return self._tables[key]

    def level(self, x, y, zoom, img):
        """Interpolate (:174-195) at one level for float32 pixel arrays x, y -> [n, D] torch fp32: each form's pixels at once, a per-pixel scalar as a column."""
        W, H = self.wh[img]
        win, nw, nh = geometry(W, H, self.clip, self.overlap, zoom)
        T = self.table(zoom, img)
        h1, h2 = indices(x, win, nw, self.overlap)
        v1, v2 = indices(y, win, nh, self.overlap)
        x1, x2, y1, y2 = centres(h1, win, self.overlap), centres(h2, win, self.overlap), centres(v1, win, self.overlap), centres(v2, win, self.overlap)
        rows = lambda v, h: T[torch.from_numpy(v * nw + h)]
        E11, E21, E12, E22 = rows(v1, h1), rows(v1, h2), rows(v2, h1), rows(v2, h2)
        col = lambda a, m: torch.from_numpy(np.ascontiguousarray(a[m], F32)).reshape(-1, 1)
        out = E11.clone()
        same_x, same_y = x2 == x1, y2 == y1
        m = same_x & ~same_y
        if m.any():
            t = torch.from_numpy(m)
            out[t] = E11[t] + (E12[t] - E11[t]) / col(y2 - y1, m) * col(y - y1, m)
        m = same_y & ~same_x
        if m.any():
            t = torch.from_numpy(m)
            out[t] = E11[t] + (E21[t] - E11[t]) / col(x2 - x1, m) * col(x - x1, m)
        m = ~same_x & ~same_y
        if m.any():
            t = torch.from_numpy(m)
            d1 = col((x2 - x1) * (y2 - y1), m)
            a, b, c, e = col(x2 - x, m), col(y2 - y, m), col(x - x1, m), col(y - y1, m)
            out[t] = E11[t] / d1 * a * b + E21[t] / d1 * c * b + E12[t] / d1 * a * e + E22[t] / d1 * c * e
        return out

    def level_one(self, x, y, zoom, img):
        """The same for ONE pixel (float32 x, y) with [1, D] tensors and scalar operands, literally as Interpolate is written."""
        W, H = self.wh[img]
        win, nw, nh = geometry(W, H, self.clip, self.overlap, zoom)
        T = self.table(zoom, img)
        (h1,), (h2,) = indices(np.array([x], F32), win, nw, self.overlap)
        (v1,), (v2,) = indices(np.array([y], F32), win, nh, self.overlap)
        x1, x2, y1, y2 = (float(centres(i, win, self.overlap)) for i in (h1, h2, v1, v2))
        E = lambda h, v: T[v * nw + h].reshape(1, -1)
        f = lambda v: float(F32(v))
        x, y = F32(x), F32(y)
        if x2 == x1 and y2 == y1:
            return E(h1, v1)
        if x2 == x1:
            return E(h1, v1) + (E(h1, v2) - E(h1, v1)) / f(F32(y2) - F32(y1)) * f(y - F32(y1))
        if y2 == y1:
            return E(h1, v1) + (E(h2, v1) - E(h1, v1)) / f(F32(x2) - F32(x1)) * f(x - F32(x1))
        d1 = f(F32(F32(x2) - F32(x1)) * F32(F32(y2) - F32(y1)))
        a, b, c, e = f(F32(x2) - x), f(F32(y2) - y), f(x - F32(x1)), f(y - F32(y1))
        return E(h1, v1) / d1 * a * b + E(h2, v1) / d1 * c * b + E(h1, v2) / d1 * a * e + E(h2, v2) / d1 * c * e

    def pixel_values(self, x, y, scale, img):
        """GetPixelValue for int arrays x, y (converted to float32 as .to(kFloat) does) -> [n, D] numpy fp32."""
        x = np.asarray(x, np.int64).astype(F32)
        y = np.asarray(y, np.int64).astype(F32)
        z1, z2, zoom, which = levels_for_scale(scale, self.mz)
        e1, e2 = self.level(x, y, z1, img), self.level(x, y, z2, img)      # the reference evaluates both levels
        if which == 1:
            return e1.numpy()
        if which == 2:
            return e2.numpy()
        return (e1 + (e2 - e1) / float(F32(F32(z2) - F32(z1))) * float(F32(zoom - F32(z1)))).numpy()

    def pixel_value_loop(self, x, y, scale, img):
        """GetPixelValue one pixel per call (level_one), the shape of the reference's host loop (NeRFDataset.cpp:182-193) -> [n, D] numpy fp32."""
        z1, z2, zoom, which = levels_for_scale(scale, self.mz)
        rows = []
        for xi, yi in zip(np.asarray(x, np.int64).astype(F32), np.asarray(y, np.int64).astype(F32)):
            e1, e2 = self.level_one(xi, yi, z1, img), self.level_one(xi, yi, z2, img)
            if which == 1:
                r = e1
            elif which == 2:
                r = e2
            else:
                r = e1 + (e2 - e1) / float(F32(F32(z2) - F32(z1))) * float(F32(zoom - F32(z1)))
            rows.append(r)
        return torch.cat(rows).numpy()


def random_pyramid(wh, clip, overlap, d, seed, mz=None, drop_levels=()):
    """Unit-norm random embeddings for every level the reference's builder produces (PyramidEmbedder.cpp:382-446: levels -1 .. min(n_img, MaxZoomOut))."""
    rng = np.random.RandomState(seed)
    mz = max_zoom_out(wh, clip) if mz is None else mz
    emb = {}
    for img, (W, H) in enumerate(wh):
        top = min(int(min(log2f(W // clip) if W // clip else -np.inf, log2f(H // clip) if H // clip else -np.inf)), mz)
        for z in range(-1, top + 1):
            if (img, z) in drop_levels:
                continue
            _, nw, nh = geometry(W, H, clip, overlap, z)
            for h in range(max(nw, 0)):
                for v in range(max(nh, 0)):
                    e = rng.randn(1, d).astype(F32)
                    emb[(h, v, z, img)] = (e / np.linalg.norm(e)).astype(F32)
    return emb


def same_bits(a, b):
    """Equal bit for bit outside NaNs, NaN in the same places (the NaN a division produces carries a sign that differs between x86 and the GPU)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
GEOMETRY_CASES = [(800, 800, 336, 0.75), (1008, 756, 224, 0.5), (160, 96, 32, 0.5), (48, 40, 32, 0.5), (1001, 333, 225, 0.3), (640, 480, 97, 0.9)]


@pytest.mark.parametrize("w,h,clip,overlap", GEOMETRY_CASES)
def test_level_geometry_matches_the_restatement(w, h, clip, overlap):
    from nerfpp_amd.pyramid import LevelGeometry
    for z in range(-1, 5):
        assert LevelGeometry(w, h, clip, overlap, z) == geometry(w, h, clip, overlap, z), (w, h, clip, overlap, z)
    assert geometry(800, 800, 336, 0.75, -1) == (168, 16, 16) and geometry(800, 800, 336, 0.75, 0) == (336, 6, 6) and geometry(800, 800, 336, 0.75, 1) == (672, 1, 1)


def test_max_zoom_out_matches_the_restatement():
    from nerfpp_amd import _lib as L
    from nerfpp_amd.pyramid import MaxZoomOut
    V = lambda W, H: type("V", (), dict(W=W, H=H))
    cases = [([(800, 800)], 336), ([(1008, 756)], 224), ([(160, 96), (48, 40)], 32), ([(1343, 100), (200, 671)], 336), ([(4096, 2048)], 224),
             ([(671, 671)], 336), ([(672, 672)], 336), ([(2687, 2688)], 336)]
    for wh, clip in cases:
        assert MaxZoomOut([V(w, h) for w, h in wh], clip) == max_zoom_out(wh, clip), (wh, clip)
    assert max_zoom_out([(1343, 100), (200, 671)], 336) == 0           # wmax and hmax from different views; 671 // 336 = 1
    # a largest view below the CLIP size: the integer quotient is 0 and log2f(0) = -inf, which the reference stores into an int (undefined); float division
    # would have given int(log2(300 / 336)) = 0 -- the library refuses instead
    with pytest.raises(L.NrfError):
        MaxZoomOut([V(300, 800)], 336)


def test_save_load_round_trip_in_the_reference_format(tmp_path):
    from nerfpp_amd.pyramid import PyramidEmbedding
    emb = random_pyramid([(160, 96), (48, 40)], 32, 0.5, 8, seed=3)
    keys = list(emb)
    rng = np.random.RandomState(0)
    shuffled = {keys[i]: emb[keys[i]] for i in rng.permutation(len(keys))}
    path = str(tmp_path / "pyramid_embeddings.pt")
    PyramidEmbedding(embeddings=shuffled).Save(path)
    m = torch.jit.load(path, map_location="cpu")
    params = dict(m.named_parameters())
    assert sorted(params, key=int) == [str(i) for i in range(2 * len(emb))] and not dict(m.named_buffers())
    order = sorted(emb)                      # std::map<std::tuple<int, int, int, int>> order: hor, then vert, then zoom (-1 first), then image
    assert order[0] == (0, 0, -1, 0) and order[1] == (0, 0, -1, 1) and order[2] == (0, 0, 0, 0)
    for i, k in enumerate(order):
        idx, e = params[str(2 * i)], params[str(2 * i + 1)]
        assert idx.dtype == torch.int32 and tuple(idx.shape) == (4,) and tuple(idx.tolist()) == k
        assert e.dtype == torch.float32 and tuple(e.shape) == (1, 8) and np.array_equal(e.detach().numpy(), emb[k])
    back = PyramidEmbedding().Load(path)
    assert list(back.Embeddings) == order and all(np.array_equal(back.Embeddings[k], emb[k]) for k in order)
    # a key read again replaces the earlier entry, as the map assignment in Load does (PyramidEmbedder.cpp:221)
    from nerfpp_amd.checkpoint import save_tensor_list
    save_tensor_list(path, [np.array([1, 0, 0, 0], np.int32), np.ones((1, 8), F32), np.array([1, 0, 0, 0], np.int32), np.full((1, 8), 2, F32)])
    assert np.array_equal(PyramidEmbedding().Load(path).Embeddings[(1, 0, 0, 0)], np.full((1, 8), 2, F32))


@pytest.mark.parametrize("clip,overlap", [(32, 0.75), (32, 0.5)])
def test_restatement_reproduces_a_linear_field(clip, overlap):
    """Entries f(cx, cy) = a + b * cx + c * cy at the patch centres of every level: bilinear inside (and, the reference's quirk at overlap 0.5, just outside) the
    centre pairs and linear across levels, so every pixel between the outer centres reads f(x, y) to rounding."""
    W, H, d = 256, 192, 6
    rng = np.random.RandomState(1)
    a, b, c = rng.randn(d), rng.randn(d) / 100, rng.randn(d) / 100
    wh = [(W, H)]
    mz = max_zoom_out(wh, clip)
    emb = {}
    lo, hi = 0.0, np.inf
    for z in range(-1, mz + 1):
        win, nw, nh = geometry(W, H, clip, overlap, z)
        cx, cy = centres(np.arange(nw), win, overlap), centres(np.arange(nh), win, overlap)
        lo, hi = max(lo, cx[0], cy[0]), min(hi, cx[-1], cy[-1])
        for h in range(nw):
            for v in range(nh):
                emb[(h, v, z, 0)] = (a + b * np.float64(cx[h]) + c * np.float64(cy[v])).astype(F32).reshape(1, d)
    R = Restated(emb, wh, clip, overlap)
    g = np.arange(int(np.ceil(lo)), int(hi) + 1)
    xs, ys = np.meshgrid(g, g, indexing="ij")
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    want = a + b * xs[:, None] + c * ys[:, None]
    for scale in (0.5, 1.0, 0.7, 1.5):
        got = R.pixel_values(xs, ys, scale, 0).astype(np.float64)
        assert np.abs(got - want).max() < 1e-4 * np.abs(want).max(), scale


def test_restatement_is_constant_beyond_the_outer_patch_centres():
    """Beyond the first / last patch centre both indices clamp to the same patch: the value stops changing along that axis (bit for bit)."""
    wh = [(160, 96)]
    R = Restated(random_pyramid(wh, 32, 0.75, 16, seed=4), wh, 32, 0.75)
    for z in (-1, 0):
        win, nw, nh = geometry(160, 96, 32, 0.75, z)
        first, last = centres(0, win, 0.75), centres(nw - 1, win, 0.75)
        scale = 2.0 ** z
        ys = np.arange(96)
        left = [R.pixel_values(np.full(96, x), ys, scale, 0) for x in range(0, int(first) - 2)]
        right = [R.pixel_values(np.full(96, x), ys, scale, 0) for x in range(int(last) + 4 * win, int(last) + 4 * win + 3)]
        assert len(left) >= 2 and all(np.array_equal(left[0], v) for v in left[1:])
        assert all(np.array_equal(right[0], v) for v in right[1:])
        inner = R.pixel_values(np.full(96, int(first) + win // 4), ys, scale, 0)
        assert not np.array_equal(inner, left[0])


def test_restatement_vectorised_equals_the_per_pixel_loop():
    """The batched restatement (one ATen op per term over all pixels of a form) against one call per pixel with scalar operands, as the reference loops."""
    wh = [(160, 96), (48, 40)]
    R = Restated(random_pyramid(wh, 32, 0.5, 24, seed=5), wh, 32, 0.5)
    rng = np.random.RandomState(6)
    x, y = rng.randint(0, 96, 300), rng.randint(0, 160, 300)
    for scale in (0.5, 1.0, 0.25, 0.7, 3.0):
        assert same_bits(R.pixel_values(x, y, scale, 0), R.pixel_value_loop(x, y, scale, 0)), scale
    assert np.isnan(R.pixel_values(x, y, 3.0, 0)).all() and not np.isnan(R.pixel_values(x, y, 2.0, 0)).any()


def test_restatement_missing_level_is_an_error():
    wh = [(160, 96), (48, 40)]
    R = Restated(random_pyramid(wh, 32, 0.5, 4, seed=7), wh, 32, 0.5)
    R.pixel_values([3], [5], 0.5, 1)
    with pytest.raises(KeyError):
        R.pixel_values([3], [5], 1.0, 1)          # level 1 of the 48 x 40 view was never built
