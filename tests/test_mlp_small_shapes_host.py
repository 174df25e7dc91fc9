"""CPU tests that pin the C oracle's NeRFSmall (orc_mlp_small, orc_mlp_small_backward: fp32 FMA chains) against the float64 restatement of
tests/mlp_small_ref.py on all 60 shapes of the matrix-core family -- geo_feat_dim 0, 1, 7, 14, 15; 2 to 4 colour layers; 16 and 64 view features.  The GPU module
(tests/test_mlp_small_shapes_gpu.py) holds the kernels to the oracle and to forward64 on the same cases, so what is measured here carries over.

Measured here (random networks of random_network(), gain 1.6, with and without the x 30 sigma row; 333 points of random_inputs()):
  forward   worst max |oracle - float64| over all 60 shapes = 6.7e-7 of the output's maximum -- jointly and per column group (rgb, sigma), whichever is larger;
            bar 2e-6 (fp32 FMA chain against float64 over at most seven layers).
  backward  the three shapes nrf_mlp_backward_f16 refuses: worst max |oracle - float64| = 3.9e-7 of a layer's largest weight gradient and 3.0e-7 of the largest
            feature gradient; bar 1.6e-6 = 4 x the larger.
  integer networks: the oracle equals forward64 exactly."""
import numpy as np
import pytest

from oracle import capi as O
import mlp_small_ref as MS

FORWARD_BAR, BACKWARD_BAR = 2e-6, 1.6e-6


def test_the_case_list_is_the_whole_family():
    assert len(MS.SHAPES) == 60 and len(set(MS.SHAPES)) == 60 and len(MS.INSTANTIATIONS) == 12
    assert {s[:3] for s in MS.SHAPES} == set(MS.INSTANTIATIONS) and {s[3] for s in MS.SHAPES} == {0, 1, 7, 14, 15}
    assert all(s in MS.SHAPES for s in MS.BWD_REFUSED)
    for shape in MS.SHAPES:
        v, nl, nlc, g = shape
        named = MS.S.small_shapes(MS.IN_CH, v, nl, MS.HIDDEN, g, nlc, MS.HIDDEN)
        assert [(i, o) for _, o, i, _ in named] == MS.layer_dims(shape)          # the blob layout is scene.small_shapes'


@pytest.mark.parametrize("shape", MS.SHAPES, ids=MS.shape_id)
def test_oracle_forward_vs_float64(shape):
    for sigma_scale in (None, 30.0):
        blob = MS.random_network(shape, 7000 + 13 * MS.SHAPES.index(shape), sigma_scale)
        x = MS.random_inputs(shape, 5, 333)
        y = O.mlp_small(blob, x, **MS.oracle_kw(shape))
        ref = MS.forward64(blob, x, shape)
        joint = np.abs(y - ref).max() / np.abs(ref).max()
        groups = MS.group_errors(y, ref)
        print(f"{MS.shape_id(shape)} sigma x {sigma_scale}: joint {joint:.2e}, rgb {groups['rgb'][0]:.2e}, sigma {groups['sigma'][0]:.2e}")
        assert max(joint, groups["rgb"][0], groups["sigma"][0]) <= FORWARD_BAR


@pytest.mark.parametrize("shape", MS.SHAPES, ids=MS.shape_id)
def test_oracle_equals_float64_on_the_integer_networks(shape):
    for p in (1, 63, 257):
        blob, x, out = MS.integer_network(shape, 11, p)
        assert out.shape == (p, 4)
        y = O.mlp_small(blob, x, **MS.oracle_kw(shape))
        assert np.array_equal(y.astype(np.float64), out), MS.shape_id(shape)


def test_integer_network_is_a_function_of_shape_and_seed():
    shape = (16, 3, 2, 7)
    a, b = MS.integer_network(shape, 11, 1), MS.integer_network(shape, 11, 513)
    assert np.array_equal(a[0], b[0]) and not np.array_equal(a[0], MS.integer_network(shape, 12, 1)[0])
    assert a[2][0, 3] != 0 and a[2][0, :3].any()


def test_a_shifted_geo_column_is_visible_in_forward64():
    """What the exact tests are for: moving the geo columns of colour layer 0 by one (the off-by-one of a packer's column map) changes rgb on the integer networks."""
    for shape in [s for s in MS.SHAPES if s[3] in (1, 7, 14)]:
        v, nl, nlc, g = shape
        blob, x, out = MS.integer_network(shape, 11, 257)
        mats = MS.matrices(blob, shape)
        w = mats[nl].copy()
        w[:, v:v + g] = np.roll(w[:, v:v + g], 1, axis=1) if g > 1 else 0.0
        mats[nl] = w
        moved = MS.forward64(np.concatenate([m.reshape(-1) for m in mats]).astype(np.float32), x, shape)
        assert np.array_equal(moved[:, 3], out[:, 3]) and not np.array_equal(moved[:, :3], out[:, :3]), MS.shape_id(shape)


@pytest.mark.parametrize("shape", MS.BWD_REFUSED, ids=MS.shape_id)
def test_oracle_backward_vs_float64(shape):
    blob = MS.random_network(shape, 4321, 30.0)
    x = MS.random_inputs(shape, 6, 333)
    g = (np.random.RandomState(9).standard_normal((333, 4)) * 1e-3).astype(np.float32)
    gp, gx = O.mlp_small_backward(blob, x, g, **MS.oracle_kw(shape))
    rp, rx = MS.backward64(blob, x, g, shape)
    assert gx.shape == rx.shape == (333, MS.IN_CH)
    off = 0
    for li, (i, o) in enumerate(MS.layer_dims(shape)):
        a, b = gp[off:off + i * o], rp[off:off + i * o]
        off += i * o
        err = np.abs(a - b).max() / np.abs(b).max()
        print(f"{MS.shape_id(shape)} dW of layer {li}: {err:.2e}")
        assert np.abs(b).max() > 0 and err <= BACKWARD_BAR, (li, err)
    err = np.abs(gx - rx).max() / np.abs(rx).max()
    print(f"{MS.shape_id(shape)} d / dx: {err:.2e}")
    assert err <= BACKWARD_BAR, err


def test_backward64_against_central_differences():
    """backward64 is itself checked: central differences of forward64 in float64 on a network with no pre-activation near the kink"""
    shape = (16, 2, 2, 7)
    blob = MS.random_network(shape, 99).astype(np.float64)
    x = MS.random_inputs(shape, 3, 5).astype(np.float64)
    g = np.random.RandomState(4).standard_normal((5, 4))
    gp, gx = MS.backward64(blob, x, g, shape)
    loss = lambda b, xx: float((MS.forward64(b, xx, shape) * g).sum())
    rng = np.random.RandomState(1)
    for k in rng.choice(blob.size, 40, replace=False):
        d = np.zeros_like(blob); d[k] = 1e-6
        assert abs((loss(blob + d, x) - loss(blob - d, x)) / 2e-6 - gp[k]) <= 1e-6 * max(1.0, abs(gp[k]))
    for r, c in zip(rng.randint(0, 5, 20), rng.randint(0, MS.IN_CH, 20)):
        d = np.zeros_like(x); d[r, c] = 1e-6
        assert abs((loss(blob, x + d) - loss(blob, x - d)) / 2e-6 - gx[r, c]) <= 1e-6 * max(1.0, abs(gx[r, c]))
