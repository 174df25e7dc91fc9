"""The yardstick of the image metrics (image_metrics.hip, nerfpp_amd/metrics.py): a numpy float64 restatement of the operation order include/nerfpp_hip.h states
for nrf_ssim / nrf_ms_ssim / nrf_image_mse, and the seeded image pairs of the tests.  numpy rounds every elementwise float64 op once and fuses nothing, so with the
library's own window (nrf_ssim_window) the SSIM map must equal the kernel's bit for bit.  tests/test_metrics_host.py pins this file against an independent definition
built on scipy.ndimage.correlate1d."""
import numpy as np

from nerfpp_amd.synth import synth_u01

TAPS = 11
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
# (h, w, c) of the single-scale tests.  Valid regions 1x1, 1x65, 2x3, 33x32, 64x129, 129x64, 30x257: around the kernel's 32 x 32 output tile they hold an edge of exactly
# one tile (32), one past it (33), two tiles (64) and one past (65), and one past four and eight tiles (129, 257); 43x42x3 and 40x267x4 also have partial tiles in both axes.
SHAPES = ((11, 11, 1), (11, 75, 3), (12, 13, 3), (43, 42, 3), (74, 139, 1), (139, 74, 3), (40, 267, 4))


def window():
    """g[k] = exp(-(k-5)^2 / 4.5) / sum, the sum added in order k = 0..10."""
    g = np.exp(-((np.arange(TAPS, dtype=np.float64) - 5.0) ** 2) / 4.5)
    s = g[0]
    for k in range(1, TAPS):
        s = s + g[k]
    return g / s


def filt(a, g, axis):
    """The valid 11-tap sum along `axis`: acc = g[0] * a[0]; acc = acc + g[k] * a[k], k = 1..10."""
    n = a.shape[axis] - (TAPS - 1)
    sl = lambda k: tuple(slice(k, k + n) if d == axis else slice(None) for d in range(a.ndim))
    acc = g[0] * a[sl(0)]
    for k in range(1, TAPS):
        acc = acc + g[k] * a[sl(k)]
    return acc


def ssim_maps(x, y, g, data_range=1.0):
    """x, y [b, h, w, c] -> (ssim, cs), each [b, h-10, w-10, c] float64."""
    x, y = np.asarray(x).astype(np.float64), np.asarray(y).astype(np.float64)
    L = np.float64(data_range)
    c1, c2 = (0.01 * L) * (0.01 * L), (0.03 * L) * (0.03 * L)
    both = lambda a: filt(filt(a, g, 2), g, 1)          # along the row first, then along the column
    mx, my, exx, eyy, exy = both(x), both(y), both(x * x), both(y * y), both(x * y)
    mxx, myy, mxy = mx * mx, my * my, mx * my
    sxx, syy, sxy = exx - mxx, eyy - myy, exy - mxy
    cs = (2.0 * sxy + c2) / ((sxx + syy) + c2)
    lum = (2.0 * mxy + c1) / ((mxx + myy) + c1)
    return lum * cs, cs


def means_of(ssim, cs):
    """[b, c, 2]: numpy's sum of each map over the valid region, divided by its count."""
    n = ssim.shape[1] * ssim.shape[2]
    return np.stack([ssim.sum(axis=(1, 2)) / n, cs.sum(axis=(1, 2)) / n], axis=-1)


def pool2(a):
    """((a00 + a01) + (a10 + a11)) * 0.25 in double; an odd trailing row / column is dropped."""
    a = np.asarray(a).astype(np.float64)
    h2, w2 = a.shape[1] // 2, a.shape[2] // 2
    a = a[:, :2 * h2, :2 * w2]
    return ((a[:, 0::2, 0::2] + a[:, 0::2, 1::2]) + (a[:, 1::2, 0::2] + a[:, 1::2, 1::2])) * 0.25


def ms_ssim_scale_means(x, y, g, data_range=1.0, scales=5):
    """[scales, b, c, 2] and the pooled sizes [(h, w)] of every scale."""
    out, sizes = [], []
    for i in range(scales):
        if i:
            x, y = pool2(x), pool2(y)
        sizes.append((x.shape[1], x.shape[2]))
        out.append(means_of(*ssim_maps(x, y, g, data_range)))
    return np.stack(out), sizes


def ms_ssim_combine(scale_means, weights=MS_WEIGHTS):
    """[scales, b, c, 2] -> [b]: per channel prod_i max(cs_i, 0)^w_i over all scales but the last, times max(ssim_last, 0)^w_last; the mean over channels."""
    m = np.asarray(scale_means, np.float64)
    w = np.asarray(weights, np.float64)
    assert m.shape[0] == w.shape[0]
    terms = np.maximum(np.concatenate([m[:-1, ..., 1], m[-1:, ..., 0]], axis=0), 0.0)
    return np.prod(terms ** w[:, None, None], axis=0).mean(axis=1)


def ssim_independent(x, y, data_range=1.0):
    """An independent definition: scipy.ndimage.correlate1d with its own Gaussian (normalised by np.sum), the 'same'-size result cropped to the valid region, the
    textbook formula with the covariances formed apart.  -> ssim [b, h-10, w-10, c]."""
    from scipy.ndimage import correlate1d
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    k = np.arange(-5, 6, dtype=np.float64)
    g = np.exp(-k * k / (2.0 * 1.5 ** 2))
    g = g / np.sum(g)
    f = lambda a: correlate1d(correlate1d(a, g, axis=1, mode="constant"), g, axis=2, mode="constant")[:, 5:-5, 5:-5]
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mx, my = f(x), f(y)
    vx, vy, cxy = f(x * x) - mx * mx, f(y * y) - my * my, f(x * y) - mx * my
    return ((2 * mx * my + c1) * (2 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))


def mse(x, y):
    """[b]: the mean over an image of ((double)x - (double)y)^2."""
    d = np.asarray(x).astype(np.float64) - np.asarray(y).astype(np.float64)
    d = d.reshape(d.shape[0], -1)
    return (d * d).sum(axis=1) / d.shape[1]


MSE_PER_BLOCK = 4096


def mse_partials(x, y):
    """[b, blocks]: what nrf_image_mse leaves in its workspace.  Blocks of 4096 elements; lane t of 256 takes t, t + 256, ... in ascending order from 0.0; then the
    ordered block sum (ordered_sum_ref.block_sums)."""
    from ordered_sum_ref import block_sums
    d = np.asarray(x).astype(np.float64) - np.asarray(y).astype(np.float64)
    d = d.reshape(d.shape[0], -1)
    b, n = d.shape
    nb = -(-n // MSE_PER_BLOCK)
    sq = np.zeros((b, nb * MSE_PER_BLOCK))
    sq[:, :n] = d * d
    sq = sq.reshape(b, nb, MSE_PER_BLOCK // 256, 256)
    lanes = np.zeros((b, nb, 256))
    for i in range(MSE_PER_BLOCK // 256):
        lanes = lanes + sq[:, :, i]
    return block_sums(lanes.reshape(-1, 256)).reshape(b, nb)


def mse_ordered(x, y):
    """[b]: nrf_image_mse bit for bit: the ordered finish pass over mse_partials, divided by the count."""
    from ordered_sum_ref import finish
    n = np.asarray(x).reshape(np.asarray(x).shape[0], -1).shape[1]
    return np.array([finish(p) / np.float64(n) for p in mse_partials(x, y)])


ORDERED_MSE_ELEMS = (1, 4097, 256 * 4096 + 1)          # one element; one block and one element; 257 block partials: a second strided trip that ends off a multiple of 256
ORDERED_MSE_SEED = 89          # at which the 257 partials of both images and the lanes of the first block tell summation orders apart (test_ordered_sum_host.py)


def ordered_mse_pair(n):
    """two images of n elements, [2, n] fp32 each: the inputs of the bit-for-bit MSE test"""
    x, y = pair("indep", 2, 1, n, 1, seed=ORDERED_MSE_SEED)
    return x.reshape(2, n), y.reshape(2, n)


def pair(kind, b, h, w, c, seed=77):
    """Seeded fp32 image pairs [b, h, w, c] in [0, 1] (synth_u01).  SSIM over the SHAPES above with b = 3, as measured with this file:
       noise  a smooth sinusoid (0.3 .. 0.7) plus 0.2 of noise, against the same image plus 0.1 of fresh noise: channel means 0.897 .. 0.941, pixels 0.76 .. 0.98
       indep  two independent uniform images: channel means -0.29 .. 0.36 at the tiny shapes, within 0.04 of 0 from 43 x 42 on; pixels -0.63 .. 0.71
       same   y = x: exactly 1 at every pixel
       flat   0.25 against 0.75: 0.3751 / 0.6251 at every pixel."""
    n = b * h * w * c
    shape = (b, h, w, c)
    u = lambda k: synth_u01(seed + 1000 * k + 7 * h + 13 * w + c, n).reshape(shape)
    if kind == "flat":
        return np.full(shape, 0.25, np.float32), np.full(shape, 0.75, np.float32)
    if kind == "indep":
        return u(1), u(2)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    smooth = (0.5 + 0.2 * np.sin(0.21 * xx + 0.13 * yy)).astype(np.float32)[None, :, :, None]
    x = (smooth + np.float32(0.2) * (u(3) - np.float32(0.5))).astype(np.float32)
    if kind == "same":
        return x, x.copy()
    assert kind == "noise", kind
    y = (x + np.float32(0.1) * (u(4) - np.float32(0.5))).astype(np.float32)
    return x, y
