"""numpy restatement of the library's ordered fp64 sum (include/nerfpp_hip.h, step 4 of the surface-sampling contract; nerfpp_amd/csrc/reduce.h is the one place the
device code states it): block partials, then one ordered pass over them.  tests/test_ordered_sum_host.py holds it to a scalar model; the GPU tests of every loss and
metric compare with it bit for bit.  Imports nothing of the package."""
import numpy as np

# Uniform doubles in [0, 1) do not tell two summation orders apart at every seed (a few hundred roundings agree by chance about one time in five): for each count the
# first seed from 1 at which the ordered sum differs in bits from a sequential sum and, above 256 partials, from the tree over contiguous runs
# (tests/test_ordered_sum_host.py asserts it)
SEEDS = {0: 1, 1: 1, 255: 1, 256: 1, 257: 3, 513: 3, 1025: 2}
BLOCK_SEED = 1          # the same for the lanes of a block (256 and 3 * 256 values) against their sequential sum


def seeded(count, seed=None):
    """`count` uniform doubles in [0, 1): the partials of the host tests"""
    return np.random.default_rng(SEEDS[count] if seed is None else seed).random(count)


def block_sums(lanes):
    """[nb, 256] one double per lane -> [nb]: per wave the butterfly v += v[lane ^ o], o = 32 .. 1, then ((w0 + w1) + w2) + w3"""
    v = np.asarray(lanes, np.float64).reshape(-1, 4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    w = v[..., 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def finish(partials, is_max=False):
    """thread t of 256 takes k = t, t + 256, ... in ascending order from 0.0; then s[t] (+|max)= s[t + o], o = 128 .. 1"""
    p = np.asarray(partials, np.float64)
    rows = -(-len(p) // 256)
    p = np.concatenate([p, np.zeros(rows * 256 - len(p))]).reshape(rows, 256)
    s = np.zeros(256)
    for r in p:
        s = np.maximum(s, r) if is_max else s + r
    o = 128
    while o:
        s[:o] = np.maximum(s[:o], s[o:2 * o]) if is_max else s[:o] + s[o:2 * o]
        o >>= 1
    return s[0]
