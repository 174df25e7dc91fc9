"""The ordered fp64 sum without a GPU: tests/ordered_sum_ref.py (the numpy restatement every GPU test of a loss or metric compares with bit for bit) is held to a
scalar model written apart from it -- plain Python loops over 256 "threads", no numpy vector add -- and the inputs are shown to tell summation orders apart: a
restatement that summed in another order would not have the same bits on them.  Python floats are IEEE doubles and + rounds once, as numpy's and the device's do."""
import numpy as np
import pytest

import metrics_ref as MR
import ordered_sum_ref as OS

COUNTS = (0, 1, 255, 256, 257, 513, 1025)
bits = lambda a: np.float64(a).view(np.uint64)


def model_finish(p, is_max=False):
    """include/nerfpp_hip.h: thread t of 256 adds k = t, t + 256, ... in ascending order from 0.0, then s[t] += s[t + o] for t < o, o = 128 .. 1"""
    p = [float(v) for v in p]
    s = []
    for t in range(256):
        a = 0.0
        for k in range(t, len(p), 256):
            a = max(a, p[k]) if is_max else a + p[k]
        s.append(a)
    o = 128
    while o:
        for t in range(o):
            s[t] = max(s[t], s[t + o]) if is_max else s[t] + s[t + o]
        o //= 2
    return s[0]


def model_block_sum(lanes):
    """one block of 256 lanes: per wave the butterfly v += v[lane ^ o], o = 32 .. 1, then ((w0 + w1) + w2) + w3"""
    w = []
    for wave in range(4):
        v = [float(x) for x in lanes[wave * 64:wave * 64 + 64]]
        for o in (32, 16, 8, 4, 2, 1):
            v = [v[lane] + v[lane ^ o] for lane in range(64)]
        assert all(x == v[0] for x in v)          # the butterfly leaves the same bits in every lane
        w.append(v[0])
    return ((w[0] + w[1]) + w[2]) + w[3]


def sequential(p):
    a = 0.0
    for v in p:
        a = a + float(v)
    return a


def contiguous_tree(p):
    """the other natural split of the same pass: thread t takes a contiguous run of ceil(n / 256) partials, then the same halving tree"""
    p = [float(v) for v in p]
    run = -(-len(p) // 256)
    s = [sequential(p[t * run:(t + 1) * run]) for t in range(256)]
    o = 128
    while o:
        for t in range(o):
            s[t] = s[t] + s[t + o]
        o //= 2
    return s[0]


@pytest.mark.parametrize("count", COUNTS)
def test_finish_has_the_bits_of_the_scalar_model_and_of_no_other_order(count):
    p = OS.seeded(count)
    got, want = OS.finish(p), model_finish(p)
    seq, run = sequential(p), contiguous_tree(p)
    print(f"count {count}: finish {float(got)!r}, sequential {seq!r}, contiguous runs {run!r}")
    assert bits(got) == bits(want)
    assert bits(OS.finish(p, is_max=True)) == bits(model_finish(p, True)) == bits(max(p, default=0.0))
    if count >= 2:          # (a sum of fewer than two terms has one order)
        assert bits(want) != bits(seq)
    if count > 256:         # (up to 256 partials every run is one partial: the two orders are the same)
        assert bits(want) != bits(run)
    else:
        assert bits(want) == bits(run)


@pytest.mark.parametrize("nb", [1, 3])
def test_block_sums_have_the_bits_of_the_scalar_model_and_not_of_a_sequential_sum(nb):
    lanes = OS.seeded(nb * 256, seed=OS.BLOCK_SEED).reshape(nb, 256)
    got = OS.block_sums(lanes)
    assert got.shape == (nb,)
    for i in range(nb):
        assert bits(got[i]) == bits(model_block_sum(lanes[i])), i
        assert bits(got[i]) != bits(sequential(lanes[i])), i


def test_the_mse_inputs_of_the_gpu_test_tell_the_orders_apart():
    """tests/test_metrics_gpu.py pins nrf_image_mse end to end on these pairs: their lane sums and their 257 block partials must discriminate too."""
    n = MR.ORDERED_MSE_ELEMS[-1]
    assert MR.ORDERED_MSE_ELEMS == (1, 4097, 256 * 4096 + 1)
    x, y = MR.ordered_mse_pair(n)
    parts = MR.mse_partials(x, y)
    assert parts.shape == (2, 257)
    for img in range(2):
        assert bits(OS.finish(parts[img])) == bits(model_finish(parts[img]))
        assert bits(model_finish(parts[img])) != bits(sequential(parts[img])) and bits(model_finish(parts[img])) != bits(contiguous_tree(parts[img])), img
    # the first block's lanes, restated here with scalar adds: lane t takes t, t + 256, ... in ascending order
    d = x[0, :4096].astype(np.float64) - y[0, :4096].astype(np.float64)
    sq = [float(v) for v in d * d]
    lanes = [sequential(sq[t::256]) for t in range(256)]
    assert bits(parts[0, 0]) == bits(model_block_sum(lanes)) and bits(parts[0, 0]) != bits(sequential(lanes)) and bits(parts[0, 0]) != bits(sequential(sq))
    # and the small shapes are what they say: one element, one block and one element
    for n in MR.ORDERED_MSE_ELEMS[:2]:
        x, y = MR.ordered_mse_pair(n)
        parts = MR.mse_partials(x, y)
        assert parts.shape == (2, -(-n // 4096))
        d = float(x[0, 0]) - float(y[0, 0])
        assert n > 1 or bits(MR.mse_ordered(x, y)[0]) == bits(d * d)


def test_geometry_ref_uses_this_file():
    import geometry_ref as G
    assert G._block_sums is OS.block_sums and G._finish is OS.finish
