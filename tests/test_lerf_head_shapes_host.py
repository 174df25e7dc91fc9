"""CPU checks of the cases tests/test_lerf_head_shapes_gpu.py runs (tests/lerf_head_ref.py): the two float64 forms of the render agree, the integer network meets the
conditions its bit-for-bit assertions rest on, no random case sits on the 1e-8 floor of the normalisation, and the layout helpers invert each other."""
import numpy as np
import pytest

import lerf_head_ref as H
import lerf_query_ref as Q

ALL_RAYS = H.RAY_SMALL + H.RAY_KERNEL_C_EDGES + H.RAY_SPLIT_PERSISTENT + H.RAY_F16_PERSISTENT
ALL_DENSITY = H.DENSITY_SMALL + [H.DENSITY_SPLIT_PERSISTENT, H.DENSITY_F16_PERSISTENT, H.DENSITY_EXACT_PERSISTENT]


@pytest.fixture(scope="module")
def inet():
    return H.integer_net()


@pytest.fixture(scope="module")
def rnets(manifest):
    blob = H.random_blob(manifest)
    return H.Net("rand", blob, H.random_pool_f16()), H.Net("rand", blob, H.random_pool_f32())


def test_model_is_the_query_reference_network(inet, rnets):
    for net in (inet, rnets[0]):
        sigma, a, W = Q.head(net.blob, net.pool)
        m = net.model
        assert np.array_equal(sigma.numpy(), m["sigma"]) and np.array_equal(a.numpy(), m["a"]) and np.array_equal(W.numpy(), m["W"])
        assert m["geo"].shape == (H.POOL, H.GEO)


@pytest.mark.parametrize("n,s", [(1, 32), (3, 64), (5, 96), (4, 256), (33, 32)])
def test_direct_projection_and_pooled_forms_agree(inet, rnets, n, s):
    for net in (inet, rnets[0], rnets[1]):
        c = H.ray_case(net, n, s)
        a = net.model["a"][c["idx"]].reshape(n, s, H.HID)
        direct = H.render_direct(a, net.model["W"], c["w"])
        proj, bound = H.render_projection(a, net.model["W"], c["w"])
        pooled, pbound = net.render(c["idx"], c["w"])
        scale = np.abs(direct).max()
        assert scale > 0
        assert np.abs(proj - direct).max() <= 1e-12 * scale, np.abs(proj - direct).max() / scale
        assert np.abs(pooled - proj).max() <= 1e-12 * scale and np.abs(pbound - bound).max() <= 1e-12 * bound.max()
        assert (np.abs(proj) <= bound * (1 + 1e-12)).all(), "the bound's scale dominates the value it bounds"


def test_render_is_invariant_to_the_le1_scale(rnets):
    net = rnets[0]
    n, s = H.RAY_LE1_SCALE
    c = H.ray_case(net, n, s)
    a = net.model["a"][c["idx"]].reshape(n, s, H.HID)
    ref = H.render_direct(a, net.model["W"], c["w"])
    for k in H.LE1_SCALE_EXPONENTS:
        scaled = net.with_le1_scaled(k)
        assert np.array_equal(Q.split_blob(scaled.blob)[3].numpy(), np.ldexp(net.model["W"], k)), "2^k is exact on fp32 weights of this size"
        out = H.render_direct(a, np.ldexp(net.model["W"], k), c["w"])
        assert np.abs(out - ref).max() <= 1e-13 * np.abs(ref).max()


def test_integer_network_is_exact_in_every_format(inet):
    """Integers below 2048 are fp16 numbers with a zero lo part; sums of their products below 2^24 are exact in fp32 in any order."""
    c = H.integer_conditions(inet)
    print(f"integer network: largest value {c['biggest']:.0f}, Gram exponent {c['gram_exponent']}, largest sum of |terms| of a^T G a {c['gram_abs_sum']:.0f} "
          f"(2^24 = {2 ** 24}), {c['dead_rows'].size} dead rows, {c['negative_sigma']} rows with sigma < 0")
    assert c["weights_ternary"] and c["integral"] and c["biggest"] < 2048
    assert c["gram_integral"] and c["gram_fp16_exact"]
    W = inet.model["W"]
    gmax = np.abs(W.T @ W).max()
    assert 512 < np.ldexp(gmax, -c["gram_exponent"]) <= 1024
    assert c["gram_abs_sum"] < 2 ** 24
    assert H.DEAD_ROW in c["dead_rows"] and c["negative_sigma"] > H.POOL // 8
    assert (inet.model["nrm"][c["dead_rows"]] == 1e-8).all(), "a dead sample sits on the floor of the normalisation and contributes w / 1e-8 * 0 = 0"
    live = np.setdiff1d(np.arange(H.POOL), c["dead_rows"])
    assert inet.model["nrm"][live].min() >= 1, "a live integer sample's norm is at least one"


@pytest.mark.parametrize("n,s", ALL_RAYS)
def test_integer_ray_cases_carry_their_edges(inet, n, s):
    c = H.ray_case(inet, n, s)
    m = inet.model
    dead = (m["a"][c["idx"]] == 0).all(1).reshape(n, s)
    assert c["cols"] == n * s // 2 + 7 and c["src"].min() >= 0 and c["src"].max() == c["cols"] - 1, "the merge map reaches the last column"
    assert np.unique(c["src"]).size < n * s, "the merge map repeats columns"
    assert dead.any() and not dead[n - 1, s - 1], "dead samples, and a live last one"
    assert (m["sigma"][c["idx"]] < 0).any()
    ref, bound = inet.render(c["idx"], c["w"])
    if n >= 3:                       # with fewer rays the dead ray would be the whole case
        assert dead[1].all() and (c["w"][1] > 0).any() and (ref[1] == 0).all() and (bound[1] == 0).all()
        z = c["zero_ray"]
        assert (c["w"][z] == 0).all() and not dead[z].all() and (ref[z] == 0).all() and (bound[z] == 0).all()
    assert (bound[n - 1] > 0).all() and np.abs(ref[n - 1]).max() > 0, "the last ray is live"


@pytest.mark.parametrize("p", ALL_DENSITY)
def test_integer_density_cases_carry_their_edges(inet, p):
    c = H.density_case(inet, p)
    assert c["idx"].shape == (p,) and c["keep"].shape == (p,)
    if p >= 31:                      # a single point cannot be all of these at once
        sig = inet.model["sigma"][c["idx"]]
        assert (c["idx"] == H.DEAD_ROW).any() and (c["keep"] == 0).any() and ((sig < 0) & (c["keep"] == 1)).any() and ((sig != 0) & (c["keep"] == 0)).any()
        assert sig[p - 1] < 0 and c["keep"][p - 1] == 1, "the last point is live, kept and negative"


def test_random_cases_stay_off_the_normalisation_floor(rnets):
    for net in rnets:
        nrm = net.model["nrm"]
        print(f"random network: smallest ||W a|| over the pool {nrm.min():.3e}, median {np.median(nrm):.3e}")
        assert nrm.min() > 1e-3, "five orders of magnitude above the 1e-8 floor"
        for n, s in ALL_RAYS + H.RAY_XLO + [H.RAY_LE1_SCALE]:
            c = H.ray_case(net, n, s)
            assert net.model["nrm"][c["idx"]].min() > 1e-3
            assert c["src"].max() == c["cols"] - 1
    f32 = rnets[1].pool
    assert (f32.astype(np.float16).astype(np.float32) != f32).mean() > 0.99, "the XLO pool's features are not fp16 numbers"
    f16 = rnets[0].pool
    assert np.array_equal(f16.astype(np.float16).astype(np.float32), f16)
    # the sweep of the LE1 scale moves the norm by 2^k: still far from the floor at 2^-8
    assert np.ldexp(rnets[0].model["nrm"].min(), min(H.LE1_SCALE_EXPONENTS)) > 1e-6


def test_case_tables_reach_the_paths_they_name():
    """Sizes against the launchers' grids: 256 workgroups of 256 (fp16 kernels A, B), 128 (split kernel A), 512 (exact kernel) points; split kernel B and
    k_lerf_split_geo: 4 rays per workgroup."""
    sweeps = lambda blocks: -(-blocks // 256)
    assert sweeps(-(-H.DENSITY_SPLIT_PERSISTENT // 128)) == 3 and sweeps(-(-H.DENSITY_F16_PERSISTENT // 256)) == 3 and sweeps(-(-H.DENSITY_EXACT_PERSISTENT // 512)) == 2
    assert all(sweeps(-(-n // 4)) == 2 for n, _ in H.RAY_SPLIT_PERSISTENT)
    assert [sweeps(-(-n * s // 256)) for n, s in H.RAY_F16_PERSISTENT] == [2, 3]
    assert all(s % 32 == 0 for _, s in ALL_RAYS) and {s // 32 for _, s in H.RAY_SMALL} == {1, 2, 3, 6, 8}
    assert {n % 4 for n, _ in H.RAY_SMALL} == {0, 1, 3} and all(n % 32 for n, _ in H.RAY_KERNEL_C_EDGES)


def test_layout_helpers():
    rows = np.arange(5 * 128, dtype=np.float32).reshape(5, 128) % 97
    lm = H.to_level_major(rows, 9)
    assert lm.shape == (16, 9, 8) and lm.dtype == np.float16
    for q in range(5):
        for k in (0, 7, 8, 63, 127):
            assert lm[k // 8, q, k % 8] == rows[q, k]
    assert np.isnan(lm[:, 5:, :].astype(np.float32)).all()
    assert sorted(H.perm_row(f, h, j) for f in range(3) for h in range(2) for j in range(8)) == list(range(48))
    # a plane buffer written the way kernel A writes it decodes to the rows it was written from
    stride = 7
    vals = np.random.default_rng(0).integers(-100, 100, (stride, 48)).astype(np.float64)
    buf = np.zeros((3, 2, stride, 2, 8), np.float16)
    for f in range(3):
        for h in range(2):
            for j in range(8):
                buf[f, 0, :, h, j] = vals[:, H.perm_row(f, h, j)]
                buf[f, 1, :, h, j] = 0.5
    hi, lo = H.decode_geo(buf.view(np.uint8).reshape(-1), stride)
    assert np.array_equal(hi, vals) and (lo == 0.5).all()
