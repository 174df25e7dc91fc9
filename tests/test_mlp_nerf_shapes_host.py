"""CPU tests that pin the C oracle's classic NeRF (orc_mlp_nerf, orc_mlp_nerf_backward: fp32 FMA chains, which the goldens hold to LibTorch autograd through the
compiled NeRF.cpp) against the float64 restatement of tests/mlp_nerf_ref.py on its three shapes, and the integer-network builder against its own conditions.  The
GPU module (tests/test_mlp_nerf_shapes_gpu.py) holds the kernels to forward64 / backward64 on the same cases, so the blob layout pinned here carries over.

  integer networks, 64 rows: the oracle EQUALS forward64 and backward64 as numbers, every entry of every parameter tensor and of g_x;
  random networks (scene.synth_linear_stack, make_classic_scene's fill: gain 1.4, biases 0.1, alpha row x 40), 333 points: within 2e-5 of each tensor's largest
  entry -- test_classic_mlp_backward_vs_reference_autograd's bar against the oracle."""
import numpy as np
import pytest

from oracle import capi as O
from nerfpp_amd import scene as S
import mlp_nerf_ref as MN

SEEDS = (11, 12, 13)                 # the GPU module uses 11 (network A) and 12 (network B)
ROUNDING_BAR = 2e-5


def random_network(shape, seed):
    """make_classic_scene's fill on the shape's own layer list -> blob float32"""
    scales = {"alpha_linear.weight": 40.0} if shape[6] else None
    params = S.synth_linear_stack([("model_" + name, o, i, True) for name, o, i in MN.layers(shape)], seed, 1.4, 0.1, scales)
    return np.concatenate([a.reshape(-1) for _, a in params])


def random_batch(shape, seed, p):
    """features in [-1, 1], as the positional encodings give them; g_out of the size a mean-squared loss hands back -> (x, g_out) float32"""
    rng = np.random.RandomState(seed)
    return rng.uniform(-1, 1, (p, shape[2] + shape[3])).astype(np.float32), (rng.standard_normal((p, MN.out_dims(shape))) * 1e-3).astype(np.float32)


KINK_MARGIN = 3e-4


def kink_free_batch(blob, shape, seed, p, candidates=4096):
    """The first p rows of random_batch(shape, seed, candidates) on which no pre-activation under a ReLU lies within KINK_MARGIN of zero (float64) -> (x, g_out).
    A ReLU that decides the other way moves a gradient by a whole term of its sum, whatever the arithmetic: on the plain 700-row batch, flipping the FOUR
    pre-activations below 1e-6 in float64 moves pts_linears_3.weight by 0.14 of its largest entry (profiles/mlp_nerf_shapes/measured_errors.txt).  A batch that is
    to measure the products' arithmetic keeps clear of the kink.  The margin: the least precise products (bf16x3) carry 16 significant bits per operand, 2^-16 =
    1.5e-5 of each term; the |terms| of a pre-activation of the 8 x 256 network sum to 3 - 6 in the median and to at most 9.3 (pts_linears) and 18.3
    (views_linears_0) on this batch, so 1.4e-4 / 2.8e-4 if every rounding error of a sum had the same sign, and some 1e-5 with random signs: 3e-4 is above both."""
    x, g = random_batch(shape, seed, candidates)
    pres = MN.forward64(blob, x, shape)[2]
    near = np.min([np.abs(a).min(1) for n, a in pres.items() if n.startswith("pts_linears") or n.startswith("views_linears")], 0)
    keep = np.nonzero(near > KINK_MARGIN)[0][:p]
    assert keep.size == p, f"{keep.size} of {candidates} candidates keep clear of the kink, {p} wanted"
    return np.ascontiguousarray(x[keep]), np.ascontiguousarray(g[keep])


def test_the_layer_list_is_the_blob_layout_of_the_library_and_the_oracle():
    d, w, in_ch, in_views, out_ch, skip, vd = MN.BUILT
    assert [(n, o, i) for n, o, i, _ in S.nerf_shapes(d, w, in_ch, in_views, skip)] == [("model_" + n, o, i) for n, o, i in MN.layers(MN.BUILT)]
    for shape in MN.SHAPES:
        assert MN.n_params(shape) == O.lib().orc_mlp_nerf_param_count(*[int(q) for q in shape])
        ts = MN.tensors(shape)
        assert ts[0][1] == 0 and all(a[1] + int(np.prod(a[2])) == b[1] for a, b in zip(ts, ts[1:])) and ts[-1][1] + int(np.prod(ts[-1][2])) == MN.n_params(shape)
    assert [t[0] for t in MN.tensors(MN.BUILT)][-8:] == [n + k for n in ("views_linears_0", "feature_linear", "alpha_linear", "rgb_linear") for k in (".weight", ".bias")]


@pytest.mark.parametrize("shape", MN.SHAPES, ids=MN.shape_id)
def test_oracle_equals_float64_on_the_integer_networks(shape):
    blob, x, g, out, (gp, gx) = MN.integer_network(shape, 11, 64)
    assert out.shape == (64, MN.out_dims(shape)) and gx.shape == (64, shape[2]) and gp.shape == blob.shape
    y = O.mlp_nerf(blob, x, **MN.oracle_kw(shape))
    assert np.array_equal(y.astype(np.float64), out), MN.shape_id(shape)
    ogp, ogx = O.mlp_nerf_backward(blob, x, g, **MN.oracle_kw(shape))
    assert np.array_equal(ogx.astype(np.float64), gx), MN.shape_id(shape)
    for name, off, dims in MN.tensors(shape):
        n = int(np.prod(dims))
        a, b = ogp[off:off + n].astype(np.float64), gp[off:off + n]
        assert b.any(), f"{name}: the gradient says nothing"
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, f"{MN.shape_id(shape)} {name}: {bad.size} of {n} differ, first at {bad[:5]}: {a[bad[:3]]} vs {b[bad[:3]]}"


@pytest.mark.parametrize("shape", MN.SHAPES, ids=MN.shape_id)
def test_oracle_vs_float64_on_a_random_network(shape):
    blob = random_network(shape, 7000 + 17 * MN.SHAPES.index(shape))
    x, g = random_batch(shape, 5, 333)
    out, _, pres = MN.forward64(blob, x, shape)
    y = O.mlp_nerf(blob, x, **MN.oracle_kw(shape))
    err = np.abs(y - out).max() / np.abs(out).max()
    print(f"{MN.shape_id(shape)} forward: {err:.2e} of the largest output")
    assert err <= ROUNDING_BAR
    # (a pre-activation within fp32 rounding of the kink may decide the other way in the fp32 chain and move a gradient by a whole term: the nearest one is printed)
    print(f"{MN.shape_id(shape)} smallest |pre-activation| under a ReLU: {min(np.abs(a).min() for n, a in pres.items() if n.startswith('pts') or n.startswith('views')):.2e}")
    gp, gx = MN.backward64(blob, x, g, shape)
    ogp, ogx = O.mlp_nerf_backward(blob, x, g, **MN.oracle_kw(shape))
    err = np.abs(ogx - gx).max() / np.abs(gx).max()
    print(f"{MN.shape_id(shape)} g_x: {err:.2e}")
    assert err <= ROUNDING_BAR
    for name, off, dims in MN.tensors(shape):
        n = int(np.prod(dims))
        a, b = ogp[off:off + n], gp[off:off + n]
        err = np.abs(a - b).max() / np.abs(b).max()
        print(f"{MN.shape_id(shape)} {name}: {err:.2e}")
        assert np.abs(b).max() > 0 and err <= ROUNDING_BAR, (name, err)


def test_the_kink_free_batch_keeps_its_margin_and_is_deterministic():
    shape = MN.BUILT
    blob = random_network(shape, 7000)
    x, g = kink_free_batch(blob, shape, 5, 700)
    x2, g2 = kink_free_batch(blob, shape, 5, 700)
    assert x.shape == (700, 90) and g.shape == (700, 4) and np.array_equal(x, x2) and np.array_equal(g, g2)
    pres = MN.forward64(blob, x, shape)[2]
    for name, a in pres.items():
        if name.startswith("pts_linears") or name.startswith("views_linears"):
            assert np.abs(a).min() > KINK_MARGIN and (a > 0).any() and (a < 0).any(), name
    with pytest.raises(AssertionError):
        kink_free_batch(blob, shape, 5, 700, candidates=800)


def test_backward64_against_central_differences():
    """backward64 is itself checked: central differences of forward64 in float64, on both head forms"""
    for shape in ((3, 16, 5, 3, 5, 0, True), (3, 16, 5, 0, 4, 1, False)):
        blob = random_network(shape, 99).astype(np.float64)
        x, g = (a.astype(np.float64) for a in random_batch(shape, 3, 5))
        assert min(np.abs(a).min() for a in MN.forward64(blob, x, shape)[2].values()) > 1e-5, "a kink within the difference step"
        gp, gx = MN.backward64(blob, x, g, shape)
        loss = lambda b, xx: float((MN.forward64(b, xx, shape)[0] * g).sum())
        rng = np.random.RandomState(1)
        for k in np.concatenate([rng.choice(blob.size, 60, replace=False), [t[1] for t in MN.tensors(shape)]]):          # (the first entry of every tensor among them)
            d = np.zeros_like(blob); d[k] = 1e-6
            assert abs((loss(blob + d, x) - loss(blob - d, x)) / 2e-6 - gp[k]) <= 1e-6 * max(1e-3, abs(gp[k])), (shape, k)
        for r in range(5):
            for c in range(shape[2]):
                d = np.zeros_like(x); d[r, c] = 1e-6
                assert abs((loss(blob, x + d) - loss(blob, x - d)) / 2e-6 - gx[r, c]) <= 1e-6 * max(1e-3, abs(gx[r, c])), (shape, r, c)


@pytest.mark.parametrize("shape", MN.SHAPES, ids=MN.shape_id)
def test_integer_network_is_deterministic_and_meets_its_conditions(shape):
    for seed in SEEDS:
        assert MN.attempts_used(shape, seed) <= MN.ATTEMPTS
    a, b = MN.integer_network(shape, 11, 1), MN.integer_network(shape, 11, 700)
    assert np.array_equal(a[0], b[0]) and not np.array_equal(a[0], MN.integer_network(shape, 12, 1)[0]), "the network depends on (shape, seed) alone"
    MN._integer_network.cache_clear(); MN._network.cache_clear()
    again = MN.integer_network(shape, 11, 700)
    assert all(np.array_equal(p, q) for p, q in zip(b[:4] + b[4], again[:4] + again[4])), "the same arguments give the same case"
    for p in (1, 257, 700):
        blob, x, g, out, (gp, gx) = MN.integer_network(shape, 11, p)
        assert x.shape == (p, shape[2] + shape[3]) and g.shape == out.shape == (p, MN.out_dims(shape)) and gx.shape == (p, shape[2])
        o2, (gp2, gx2) = MN.check_integer_network(blob, x, g, shape, batch=p >= 64)
        assert np.array_equal(o2, out) and np.array_equal(gp2, gp) and np.array_equal(gx2, gx)
        assert out[0, 3] != 0 and out[0, :3].any(), "row 0 differs from a cleared buffer"
        if p >= 3:
            assert not x[1].any() and not g[2].any()
    x257 = MN.integer_network(shape, 11, MN.TILE_ROWS)[1]
    t = MN.tiled(x257, 2 * MN.TILE_ROWS + 5)
    assert t.shape[0] == 2 * MN.TILE_ROWS + 5 and np.array_equal(t[MN.TILE_ROWS:2 * MN.TILE_ROWS], x257) and np.array_equal(t[-5:], x257[:5])


def test_a_condition_that_fails_is_reported_not_relaxed():
    """check_integer_network refuses a network outside its conditions: a weight of 2, a zero bias vector, a dead alpha row"""
    shape = MN.SHAPES[1]
    blob, x, g, _, _ = MN.integer_network(shape, 11, 64)
    where = {name: (off, dims) for name, off, dims in MN.tensors(shape)}
    for name, value in (("pts_linears_2.weight", 2.0), ("alpha_linear.bias", 0.0), ("alpha_linear.weight", 0.0)):
        bad = blob.copy()
        off, dims = where[name]
        n = int(np.prod(dims)) if value == 0.0 else 1
        bad[off:off + n] = value
        with pytest.raises(AssertionError):
            MN.check_integer_network(bad, x, g, shape)
