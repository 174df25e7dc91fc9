"""float64 model, case tables and input builders for the stage-level tests of the LeRF head's matrix-core passes (mlp_lerf_mfma.hip, mlp_lerf_split_mfma.hip,
sigma_lerf_f32.hip): tests/test_lerf_head_shapes_host.py checks the cases themselves on the CPU, tests/test_lerf_head_shapes_gpu.py runs them on the device.

The network is tests/lerf_query_ref.py's (split_blob, head).  The render side comes in two forms --
  direct:      out[ray] = sum_s w_s (W a_s) / max(||W a_s||, 1e-8)
  projection:  W . sum_s (w_s / max(sqrt(max(a_s^T (W^T W) a_s, 0)), 1e-8)) a_s          (what the kernels compute)
-- and the projection form once more over a POOL: every case draws its points from a pool of POOL feature rows per network (with repeats), so the float64 network runs
once per pool and a case of 131 k points is one [rays, POOL] x [POOL, 256] product.

Two networks: the random one of the existing stage tests (the manifest's `lerf` blob, sigma row x 20) and an INTEGER one -- sparse -1 / 0 / +1 weights, small integer
features -- on which every product and sum up to the LE0 output a and the Gram form a^T (W^T W) a is exact in fp16 operands, in (hi, lo) pairs and in fp32
(integer_conditions states what that takes; the host test asserts it)."""
import functools

import numpy as np
import torch

import lerf_query_ref as Q

IN, HID, GEO, EMB = Q.IN, Q.HID, Q.GEO, Q.EMB
POOL = 4096
DEAD_ROW = 0                       # integer pool: row 0 is all zero -> h = 0, sigma = 0, geo = 0, a = 0 (every LE0 unit dead)

# ------------------------------------------------------------------------------------------------ case tables
# density entries: point counts.  Workgroups take 256 points (fp16 kernel A), 128 (split kernel A), 512 (exact kernel) per iteration on a grid of at most 256.
DENSITY_SMALL = [1, 31, 32, 33, 127, 128, 129, 255, 257, 511, 513]
DENSITY_SPLIT_PERSISTENT = 65536 + 130        # split kernel A: third persistent iteration of the first workgroups
DENSITY_F16_PERSISTENT = 131072 + 300         # fp16 kernel A: third iteration
DENSITY_EXACT_PERSISTENT = 131072 + 70        # exact kernel: second iteration
DENSITY_XLO = [33, 257, 65536 + 130]          # random network, fp32 rows that are not fp16 numbers

# ray-sum entries: (rays, samples per ray)
RAY_SMALL = [(n, s) for s in (32, 64, 96, 192, 256) for n in (1, 3, 4, 5)]
RAY_KERNEL_C_EDGES = [(31, 32), (33, 32), (129, 32)]          # kernel C: 32-ray tile, 128-ray block
RAY_SPLIT_PERSISTENT = [(1027, 32), (1027, 64)]               # split kernel B and k_lerf_split_geo: one ray per wave, 1024 rays per sweep of the grid
RAY_F16_PERSISTENT = [(2051, 32), (4101, 32)]                 # fp16 kernel B: 65 536 points per sweep: second and third iteration
RAY_XLO = [(5, 96), (1027, 32)]
RAY_LE1_SCALE = (33, 64)
LE1_SCALE_EXPONENTS = [-8, -4, 0, 4, 8]
RAY_UPLOAD, DENSITY_UPLOAD = (5, 96), 257
PSTRIDE_PAD, GEO_STRIDE_PAD = 24, 8

# bars on random networks: the existing stage tests' (test_gpu_parity.py), on the same scales
BAR_SIGMA = {"f16": 3e-3, "split": 1e-5}          # x max|sigma|
BAR_SUM = {"f16": 4e-3, "split": 6e-5}            # x max|ref|
BAR_DIRECTION_SPLIT = 2e-6                        # per component of the normalised ray sum
BAR_GEO_PLANES = 2e-6                             # hi + lo of a geo plane row, x max|row|
BAR_ATOMICS_ORDER = 1e-5                          # fp16 kernel B: float atomics in another order, x max|ref|


# ------------------------------------------------------------------------------------------------ the float64 model
def head_full(blob, x):
    """(sigma [p], geo [p, 32], a [p, 256], W_le1 [768, 256]) of LeRFImpl::forward in float64 numpy; sigma, a and W are lerf_query_ref.head's."""
    w0, w1, l0, l1 = Q.split_blob(blob)
    xt = torch.as_tensor(np.asarray(x, np.float32)).to(torch.float64)
    h = torch.relu(xt @ w0.T)
    s = h @ w1.T
    a = torch.relu(torch.cat([s[:, 1:], xt], dim=1) @ l0.T)
    return s[:, 0].numpy(), s[:, 1:].numpy(), a.numpy(), l1.numpy()


def sample_norm(a, W):
    """max(sqrt(max(a^T (W^T W) a, 0)), 1e-8) per row of a."""
    g = W.T @ W
    return np.maximum(np.sqrt(np.maximum(((a @ g) * a).sum(-1), 0.0)), 1e-8)


def render_direct(a, W, w):
    """a [n, s, 256], w [n, s] -> out [n, 768]: the 768-wide embedding per sample, normalised, weighted, summed."""
    e = a @ W.T
    nrm = np.maximum(np.linalg.norm(e, axis=-1), 1e-8)
    return (np.asarray(w, np.float64)[..., None] * e / nrm[..., None]).sum(1)


def render_projection(a, W, w):
    """The kernels' form -> (out [n, 768], bound [n, 768] = |W| @ sum_s |f_s a_s|, the scale of the element-wise error bars)."""
    f = np.asarray(w, np.float64) / sample_norm(a, W)
    asum = (f[..., None] * a).sum(1)
    return asum @ W.T, (np.abs(f)[..., None] * np.abs(a)).sum(1) @ np.abs(W).T


class Net:
    """A parameter blob, its pool of feature rows [POOL, 128] fp32 and the float64 network on the pool (evaluated once)."""

    def __init__(self, kind, blob, pool):
        self.kind, self.blob, self.pool = kind, np.ascontiguousarray(blob, np.float32), np.ascontiguousarray(pool, np.float32)
        assert self.pool.shape == (POOL, IN)

    @functools.cached_property
    def model(self):
        sigma, geo, a, W = head_full(self.blob, self.pool)
        return dict(sigma=sigma, geo=geo, a=a, W=W, nrm=sample_norm(a, W))

    def with_le1_scaled(self, k):
        """The same network with LE1 multiplied by 2^k (exact in fp32): every output of the model is unchanged, the render included."""
        b = self.blob.copy()
        b[-EMB * HID:] = np.ldexp(b[-EMB * HID:], k)
        n = Net(self.kind, b, self.pool)
        n.__dict__["model"] = self.model
        return n

    def render(self, idx, w):
        """Projection form for samples pool[idx] ([n * s] row indices) with weights w [n, s], through the pool -> (out [n, 768], bound [n, 768])."""
        m = self.model
        n, s = w.shape
        f = np.asarray(w, np.float64).reshape(-1) / m["nrm"][idx]
        mat = np.zeros((n, POOL))
        np.add.at(mat, (np.repeat(np.arange(n), s), idx), f)
        return (mat @ m["a"]) @ m["W"].T, (np.abs(mat) @ np.abs(m["a"])) @ np.abs(m["W"]).T


# ------------------------------------------------------------------------------------------------ networks and pools
def random_blob(manifest):
    """The blob of the existing stage tests (test_gpu_parity.py): the manifest's `lerf` entries, the sigma row of the sigma net's last layer x 20."""
    from nerfpp_amd import synth
    blob = synth.blob_from_manifest(manifest["lerf"]).copy()
    blob[IN * HID:IN * HID + HID] *= 20.0
    return blob


def _sparse(rng, rows, cols, nnz, lo=0):
    w = np.zeros((rows, cols), np.float32)
    for r in range(rows):
        c = lo + rng.choice(cols - lo, nnz, replace=False)
        w[r, c] = rng.choice(np.float32([-1, 1]), nnz)
    return w


INTEGER_SEED = 20


def integer_blob(seed=INTEGER_SEED):
    """Sparse -1 / 0 / +1 weights in all four matrices: 4 per sigma0 row, 8 per sigma1 row, 3 feature columns (and, for every second row, one geo column) per LE0 row;
    LE1 four fifths full, which puts the largest entry of W^T W (a column's count of non-zeros) between 512 and 1024."""
    rng = np.random.default_rng(seed)
    w0 = _sparse(rng, HID, IN, 4)
    w1 = _sparse(rng, 1 + GEO, HID, 8)
    l0 = _sparse(rng, HID, GEO + IN, 3, lo=GEO)
    rows = np.arange(0, HID, 2)
    l0[rows, rng.integers(0, GEO, rows.size)] = rng.choice(np.float32([-1, 1]), rows.size)
    l1 = (rng.choice(np.float32([-1, 1]), (EMB, HID)) * (rng.random((EMB, HID)) < 0.8)).astype(np.float32)
    return np.concatenate([m.reshape(-1) for m in (w0, w1, l0, l1)]).astype(np.float32)


def integer_pool(seed=INTEGER_SEED):
    """Features in {-2, -1, 0, 1, 2} (half of them zero); row DEAD_ROW all zero."""
    rng = np.random.default_rng(seed + 1)
    x = rng.choice(np.float32([-2, -1, 1, 2]), (POOL, IN)) * (rng.random((POOL, IN)) < 0.5)
    x[DEAD_ROW] = 0
    return x.astype(np.float32)


def random_pool_f16(seed=311):
    """Features that are fp16 numbers, as the CuHashEmbedder's are, of the existing tests' amplitude."""
    return np.random.default_rng(seed).uniform(-0.5, 0.5, (POOL, IN)).astype(np.float16).astype(np.float32)


def random_pool_f32(seed=312):
    """Features that are NOT fp16 numbers: the XLO instantiations of k_lerf_split carry their lo parts."""
    return np.random.default_rng(seed).uniform(-0.5, 0.5, (POOL, IN)).astype(np.float32)


def integer_net():
    return Net("int", integer_blob(), integer_pool())


def gram_exponent(gmax):
    """The packers' power-of-two exponent e (mlp_lerf_pack_f16): the image holds W^T W * 2^-e with max|.| in (512, 1024]."""
    if not gmax > 0:
        return 0
    m, e = np.frexp(np.float32(gmax) / np.float32(1024))          # gmax / 1024 = m 2^e, m in [0.5, 1)
    e = int(e) - 1 if m == 0.5 else int(e)
    return max(e, -100)


def packed_gram(W):
    """The Gram operand as the weight image holds it, before its rounding to fp16: W^T W * 2^-e, diagonal 32-blocks as they are, blocks above doubled, blocks below zero."""
    g = np.asarray(W, np.float64).T @ np.asarray(W, np.float64)
    e = gram_exponent(np.abs(g).max())
    t = np.arange(HID) // 32
    return np.ldexp(g, -e) * np.where(t[:, None] == t[None, :], 1.0, np.where(t[None, :] > t[:, None], 2.0, 0.0)), e


def integer_conditions(net):
    """What exactness on the integer network rests on, as a dict of booleans / figures over the pool (the host test asserts them)."""
    w0, w1, l0, l1 = [t.numpy() for t in Q.split_blob(net.blob)]
    x = net.pool.astype(np.float64)
    h = np.maximum(x @ w0.T, 0)
    m = net.model
    vals = [x, h, m["sigma"], m["geo"], m["a"]]
    integral = all(np.array_equal(v, np.round(v)) for v in vals)
    biggest = max(np.abs(v).max() for v in vals)
    g = l1.T @ l1
    pg, e = packed_gram(l1)
    a = np.abs(m["a"])
    # every partial sum of a^T G a, in ANY order, is bounded by the sum of the terms' magnitudes
    gram_abs_sum = ((a @ np.abs(pg)) * a).sum(1).max()
    return dict(integral=integral, biggest=biggest, weights_ternary=bool(np.isin(net.blob, [-1, 0, 1]).all()), gram_integral=bool(np.array_equal(g, np.round(g))),
                gram_fp16_exact=bool(np.array_equal(pg.astype(np.float16).astype(np.float64), pg)), gram_exponent=e, gram_abs_sum=gram_abs_sum,
                dead_rows=np.nonzero((m["a"] == 0).all(1))[0], negative_sigma=int((m["sigma"] < 0).sum()))


# ------------------------------------------------------------------------------------------------ cases
def _seed(*k):
    return np.random.default_rng([int(v) for v in k])


def density_case(net, p):
    """p points of the pool (rows idx, with repeats; the integer network's include dead rows) and a keep mask with a fifth of the points masked."""
    rng = _seed(1, p)
    idx = rng.integers(0, POOL, p)
    keep = (rng.random(p) >= 0.2).astype(np.uint8)
    if net.kind == "int" and p >= 31:
        idx[rng.integers(0, p, max(1, p // 16))] = DEAD_ROW
        neg = np.nonzero(net.model["sigma"] < 0)[0]
        idx[5], idx[p - 1] = neg[0], neg[1 % neg.size]              # a negative sigma at the tail, where a dropped tile would hide it
        keep[3], keep[p - 2] = 0, 0
        keep[5], keep[p - 1] = 1, 1
    return dict(p=p, idx=idx, keep=keep)


def ray_case(net, n, s):
    """n rays of s samples over a table of cols = n s / 2 + 7 feature columns: column c holds pool row col_idx[c], sample i reads column src[i] (repeats, the last column
    included), so idx = col_idx[src] are the samples' pool rows -- the entries without a merge map get those rows laid out in sample order.  Weights in [0, 1), a tenth
    of them zero.  From three rays on, ray 1 is made of dead samples only (integer network) and ray `zero_ray` (2; 0 of three rays, whose last one stays live) has zero
    weights; the integer network also has dead samples sprinkled over the other rays."""
    rng = _seed(2, n, s)
    cols = n * s // 2 + 7
    col_idx = rng.integers(1, POOL, cols)
    src = rng.integers(0, cols, n * s).astype(np.int32)
    src[n * s - 1] = cols - 2                                        # the very last sample reads a column of its own
    w = rng.random((n, s)).astype(np.float32)
    w[rng.random((n, s)) < 0.1] = 0
    zero_ray = None if n < 3 else 0 if n == 3 else 2
    if net.kind == "int":
        col_idx[3] = DEAD_ROW
        dead = rng.random(n * s) < 0.1
        dead[n * s - 1] = False
        src[dead] = 3
        if n >= 3:
            src[s:2 * s] = 3
    src[(n - 1) * s] = cols - 1                                       # the last column of the table, read by a live ray
    if n >= 3:
        w[zero_ray] = 0
    w[n - 1, s - 1] = 0.75
    return dict(n=n, s=s, cols=cols, zero_ray=zero_ray, col_idx=col_idx, src=src, idx=col_idx[src], w=w)


# ------------------------------------------------------------------------------------------------ the kernels' data layouts
def to_level_major(rows, pstride=None, fill=np.nan):
    """rows [p, 128] -> fp16 [16][pstride][8]: feature 8 level + j of point q at [level][q][j]; columns p.. hold `fill` (NaN: a read past the call's columns shows)."""
    rows = np.asarray(rows, np.float32)
    p = rows.shape[0]
    pstride = p if pstride is None else pstride
    out = np.full((16, pstride, 8), fill, np.float16)
    out[:, :p, :] = rows.reshape(p, 16, 8).transpose(1, 0, 2).astype(np.float16)
    return out


def perm_row(f, h, j):
    """Row of the chained operand that element j of lane half h of fragment f carries (mfma_frag.h)."""
    return 16 * f + 8 * (j >> 2) + 4 * h + (j & 3)


def decode_geo(buf, geo_stride):
    """The geo planes [fragment 3][hi | lo][geo_stride][lane half 2][8] fp16 (raw bytes) -> (hi, lo) as float64 [geo_stride, 48]: row 0 = sigma, rows 1..32 = geo,
    rows 33..47 = the zero padding of the third fragment."""
    g = np.ascontiguousarray(buf).view(np.float16).reshape(3, 2, geo_stride, 2, 8).astype(np.float64)
    hi, lo = np.empty((geo_stride, 48)), np.empty((geo_stride, 48))
    for f in range(3):
        for h in range(2):
            for j in range(8):
                hi[:, perm_row(f, h, j)], lo[:, perm_row(f, h, j)] = g[f, 0, :, h, j], g[f, 1, :, h, j]
    return hi, lo
