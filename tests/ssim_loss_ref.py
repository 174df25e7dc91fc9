"""The yardstick of the SSIM training loss (image_metrics.hip: nrf_ssim_loss; rays.hip: nrf_rand_patches): a numpy float64 restatement of the operation order
include/nerfpp_hip.h states for the gradient of 1 - mean SSIM, built on metrics_ref.window / filt, and a host model of nrf_rand_patches on Trainer._rng_u32's
arithmetic.  numpy rounds every elementwise float64 op once and fuses nothing, so with the library's own window d_grad64 must equal grad64() value for value.
tests/test_ssim_loss_host.py pins this file against float64 torch.autograd of the textbook formula."""
import numpy as np

import metrics_ref as MR

# (b, h, w, c): a 1 x 1 valid region; the training shapes (16 and 32: one workgroup per image channel, 32 the largest it takes); 12 x 13; partial 32-wide tiles in
# both axes; one pixel past one tile (33) and past two (65); two full tiles by a partial one; four channels
SHAPES = ((1, 11, 11, 1), (4, 16, 16, 3), (3, 32, 32, 3), (2, 12, 13, 3), (1, 43, 42, 3), (1, 33, 65, 1), (1, 64, 43, 3), (1, 21, 53, 4))
KINDS = ("noise", "indep", "flat", "same")


def filt_t(m, g, axis):
    """The transposed window along `axis`, m padded with 10 zeros on both sides: acc = g[0]*M[p]; acc = acc + g[k]*M[p-k], k = 1..10.  n -> n + 10."""
    n = m.shape[axis] + (MR.TAPS - 1)
    pad = [(MR.TAPS - 1, MR.TAPS - 1) if d == axis else (0, 0) for d in range(m.ndim)]
    mp = np.pad(m, pad)                                      # M[p] of the definition is mp[p + 10]
    sl = lambda k: tuple(slice(MR.TAPS - 1 - k, MR.TAPS - 1 - k + n) if d == axis else slice(None) for d in range(m.ndim))
    acc = g[0] * mp[sl(0)]
    for k in range(1, MR.TAPS):
        acc = acc + g[k] * mp[sl(k)]
    return acc


def grad64(x, y, g, data_range=1.0):
    """x, y [b, h, w, c] -> (loss [2] = {1 - mean, mean} with numpy's sum, d (1 - mean SSIM) / dx [b, h, w, c] float64) in the header's order."""
    x, y = np.asarray(x).astype(np.float64), np.asarray(y).astype(np.float64)
    L = np.float64(data_range)
    c1, c2 = (0.01 * L) * (0.01 * L), (0.03 * L) * (0.03 * L)
    both = lambda a: MR.filt(MR.filt(a, g, 2), g, 1)
    mx, my, exx, eyy, exy = both(x), both(y), both(x * x), both(y * y), both(x * y)
    mxx, myy, mxy = mx * mx, my * my, mx * my
    sxx, syy, sxy = exx - mxx, eyy - myy, exy - mxy
    cd = (sxx + syy) + c2
    ld = (mxx + myy) + c1
    cs = (2.0 * sxy + c2) / cd
    lum = (2.0 * mxy + c1) / ld
    ssim = lum * cs
    A = cs * (2.0 * (my - lum * mx) / ld) + lum * (2.0 * (cs * mx - my) / cd)
    B = -(ssim / cd)
    Cc = 2.0 * lum / cd
    T = lambda m: filt_t(filt_t(m, g, 1), g, 2)              # along the column (image rows) first, then along the row
    n = np.float64(ssim.size)
    grad = -(((T(A) + 2.0 * x * T(B)) + y * T(Cc))) / n
    mean = ssim.sum() / n
    return np.array([1.0 - mean, mean]), grad


def rng_u32(seed, stream, idx):
    """include/nrf_rng.h's nrf_rng_u32 (the arithmetic of nerfpp_amd.train.Trainer._rng_u32)."""
    m = (1 << 64) - 1
    x = (seed + idx * 0x9E3779B97F4A7C15) & m
    x ^= (stream * 0xD1B54A32D192ED03) & m
    x ^= x >> 30; x = (x * 0xBF58476D1CE4E5B9) & m
    x ^= x >> 27; x = (x * 0x94D049BB133111EB) & m
    x ^= x >> 31
    return x >> 32


def rand_patches(seed, it, h_start, h_end, w_start, w_end, n_patches, patch):
    """-> (rand_h, rand_w) int64 [n_patches * patch * patch]: patch k's origin from streams 19 / 20, element k*patch^2 + i*patch + j = (oy + i, ox + j)."""
    rh, rw = [], []
    i, j = np.meshgrid(np.arange(patch, dtype=np.int64), np.arange(patch, dtype=np.int64), indexing="ij")
    for k in range(n_patches):
        oy = h_start + (rng_u32(seed, 19, it * n_patches + k) * (h_end - h_start - patch + 2) >> 32)
        ox = w_start + (rng_u32(seed, 20, it * n_patches + k) * (w_end - w_start - patch + 2) >> 32)
        rh.append((oy + i).reshape(-1)); rw.append((ox + j).reshape(-1))
    return np.concatenate(rh), np.concatenate(rw)
