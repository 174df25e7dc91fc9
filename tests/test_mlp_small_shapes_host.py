"""CPU tests that pin the C oracle's NeRFSmall (orc_mlp_small, orc_mlp_small_backward: fp32 FMA chains) against the float64 restatement of
tests/mlp_small_ref.py on all 60 shapes of the matrix-core family -- geo_feat_dim 0, 1, 7, 14, 15; 2 to 4 colour layers; 16 and 64 view features.  The GPU module
(tests/test_mlp_small_shapes_gpu.py) holds the kernels to the oracle and to forward64 on the same cases, so what is measured here carries over.

Measured here (random networks of random_network(), gain 1.6, with and without the x 30 sigma row; 333 points of random_inputs()):
  forward   worst max |oracle - float64| over all 60 shapes = 6.7e-7 of the output's maximum -- jointly and per column group (rgb, sigma), whichever is larger;
            bar 2e-6 (fp32 FMA chain against float64 over at most seven layers).
  backward  the three shapes nrf_mlp_backward_f16 refuses: worst max |oracle - float64| = 3.9e-7 of a layer's largest weight gradient and 3.0e-7 of the largest
            feature gradient; bar 1.6e-6 = 4 x the larger.
  integer networks: the oracle equals forward64 exactly, and its backward equals backward64 exactly on integer_backward_case (all 60 shapes).
The second half pins the yardsticks of tests/test_mlp_small_bwd_shapes_gpu.py: model16 (the fused backward's arithmetic) against backward64, the integer conditions of
every case that module lists, the level-major packers, and that model16's ReLU masks do not depend on its accumulator."""
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


# ------------------------------------------------------------------ the training backward: the yardsticks of tests/test_mlp_small_bwd_shapes_gpu.py
@pytest.mark.parametrize("shape", MS.SHAPES, ids=MS.shape_id)
def test_oracle_backward_equals_float64_on_the_integer_networks(shape):
    """orc_mlp_small_backward (an fp32 FMA chain) EQUALS backward64 as numbers on integer_backward_case, whose assertions are what makes every fp32 sum exact: all 60
    shapes at 1, 63 and 257 points, per tensor."""
    for p in (1, 63, 257):
        blob, x, g, (want_p, want_x) = MS.integer_backward_case(shape, MS.BWD_SEED, p)
        gp, gx = O.mlp_small_backward(blob, x, g, **MS.oracle_kw(shape))
        for name, off, (o, i) in MS.tensors(shape):
            assert np.array_equal(gp[off:off + o * i].astype(np.float64), want_p[off:off + o * i]), (MS.shape_id(shape), p, name)
        assert gx.shape == want_x.shape and np.array_equal(gx.astype(np.float64), want_x), (MS.shape_id(shape), p)


def test_tensors_cover_the_blob():
    for shape in MS.SHAPES:
        t = MS.tensors(shape)
        assert [dims for _, _, dims in t] == [(o, i) for i, o in MS.layer_dims(shape)]
        assert [off for _, off, _ in t] == list(np.cumsum([0] + [i * o for i, o in MS.layer_dims(shape)])[:-1])
        named = MS.S.small_shapes(MS.IN_CH, shape[0], shape[1], MS.HIDDEN, shape[3], shape[2], MS.HIDDEN)
        assert all(full[0].endswith(n) for (n, _, _), full in zip(t, named)) and len(t) == len(named)


@pytest.mark.parametrize("shape", MS.FUSED_SHAPES, ids=MS.shape_id)
def test_model16_equals_float64_on_the_integer_cases(shape):
    """model16 -- the fused kernel's arithmetic, the yardstick of the random-network test -- EQUALS backward64 on the integer cases with float64 and with float32
    accumulation, per tensor: its blob order, its masks and its sigma / geo hand-over are right before it is used to judge the kernel.  The loss scale is
    divided out exactly at every unit the GPU module uses."""
    for p, unit, s in [(1, MS.BWD_UNIT, None), (129, MS.BWD_UNIT, None), (257, MS.BWD_UNIT, None), (129, MS.BWD_UNIT, 24)] + [(MS.FUSED_UNITS_AT, u, None) for u in MS.FUSED_UNITS]:
        blob, x, g, (want_p, want_x) = MS.integer_backward_case(shape, MS.BWD_SEED, p, unit, s)
        for acc in (np.float64, np.float32):
            gp, gx, pres = MS.model16(blob, x, g, shape, acc)
            assert len(pres) == shape[1] - 1 + shape[2] - 1
            for name, off, (o, i) in MS.tensors(shape):
                assert np.array_equal(gp[off:off + o * i], want_p[off:off + o * i]), (MS.shape_id(shape), p, unit, s, acc.__name__, name)
            assert np.array_equal(gx, want_x), (MS.shape_id(shape), p, unit, s, acc.__name__)


def test_every_integer_case_of_the_gpu_module_meets_the_conditions():
    """integer_backward_case asserts what the GPU module's equalities rest on (chained gradients x 8 integers below 2048, sums of |terms| x 8 below 2^24, no all-zero
    tensor); here it runs for every (shape, points, unit, points per ray) that module lists, the 32 769-point cases included, so that no case can fail a condition
    on the GPU.  The prefilled blobs keep the sums exact too: the pattern adds at most 3 units to a sum whose |terms| stay below 2^24 / 8."""
    cases = MS.backward_cases()
    # (listed twice and counted once: 1 and 257 points of the four fused shapes, 257 points of the ten shapes of the modes)
    assert len(cases) == len(set(cases)) == 4 * 9 + 4 * 3 + 4 * 2 + 60 * 4 + 10 * 3 - 8 - 10
    for shape, p, unit, s in cases:
        blob, x, g, (want_p, want_x) = MS.integer_backward_case(shape, MS.BWD_SEED, p, unit, s)
        assert x.shape == (p, MS.IN_CH + shape[0]) and g.shape == (p, 4) and want_x.shape == (p, MS.IN_CH) and want_p.size == MS.n_params(shape)
        pre = MS.prefill(want_p.size, unit).astype(np.float64) / unit
        assert np.array_equal(pre, np.rint(pre)) and np.abs(pre).max() == 3 and np.abs(want_p / unit).max() + 3 < 2 ** 24 / MS.LOSS_SCALE


def test_level_major_packers_round_trip():
    """pack_level_major, pack_ray_views and pack_column_table encode the batch they were given: unpacked again they are x; the column map is not monotonic, has
    columns read by several points and by none, and a stride larger than the column count."""
    shape = MS.FUSED_SHAPES[0]
    for p, s in MS.LM_CASES:
        x = MS.integer_backward_case(shape, MS.BWD_SEED, p, s=s)[1]
        lm = MS.pack_level_major(x)
        assert lm.shape == (16, p, 2) and lm.dtype == np.float16
        assert np.array_equal(lm.transpose(1, 0, 2).reshape(p, 32).astype(np.float32), x[:, :32])
        views = MS.pack_ray_views(x, s)
        assert views.shape == (-(-p // s), 16) and views.dtype == np.float16 and p % s != 0
        assert np.array_equal(views.astype(np.float32)[np.arange(p) // s], x[:, 32:])
        table, src, pstride = MS.pack_column_table(x, MS.BWD_SEED)
        counts = np.bincount(src, minlength=pstride)
        assert table.shape == (16, pstride, 2) and src.dtype == np.int32 and src.max() < pstride - 5
        assert (np.diff(src) < 0).any() and counts.max() > 1 and (counts[:pstride - 5] == 0).any()
        assert np.array_equal(table[:, src].transpose(1, 0, 2).reshape(p, 32).astype(np.float32), x[:, :32])


@pytest.mark.parametrize("shape", MS.RANDOM_SHAPES, ids=MS.shape_id)
def test_model16_masks_do_not_depend_on_the_accumulator(shape):
    """On the kink_free16 batches of the GPU module (margin 1e-4) model16 with float32 accumulation has the same ReLU masks as with float64: what separates the two --
    and the kernel from either -- is then summation order and rare one-ulp fp16 double roundings, which is what the GPU module's bar 4 x e32 is made of.  The margin
    did not have to be raised.  Printed: e32 per tensor (1.5e-5 to 1.1e-4 per layer, 6e-5 to 2.7e-4 for g_x here) and model16's distance to backward64 (up to 12 %
    of a tensor's largest entry: ReLU flips of the fp16 forward, why float64 is no yardstick for the fused kernel on random weights)."""
    blob, x, g = MS.random_backward_case(shape)
    assert x.shape == (MS.RANDOM_POINTS, MS.IN_CH + shape[0])
    p64, x64, pres64 = MS.model16(blob, x, g, shape, np.float64)
    p32, x32, pres32 = MS.model16(blob, x, g, shape, np.float32)
    assert all(np.abs(a).min() >= MS.RANDOM_MARGIN for a in pres64)
    for a, b in zip(MS.relu_masks16(pres64), MS.relu_masks16(pres32)):
        assert np.array_equal(a, b)
    for a in pres64:          # ... and a mask is the sign of the pre-activation: nothing positive rounds to an fp16 zero
        assert np.array_equal(np.maximum(a, 0).astype(np.float16) > 0, a > 0)
    e32 = MS.tensor_errors(p32, x32, p64, x64, shape)
    far = MS.tensor_errors(p64, x64, *MS.backward64(blob, x, g, shape), shape)
    for name in e32:
        print(f"{MS.shape_id(shape)} {name}: e32 {e32[name]:.2e}, model16 to backward64 {far[name]:.2e}")
        assert 0 < e32[name] < 1e-3, (name, e32[name])
