"""CPU checks of what tests/test_lerf_train_shapes_gpu.py rests on (tests/lerf_train_ref.py): the float64 model reproduces the reference-autograd goldens train_lerf*,
the CPU fp32 oracle agrees with the model on the cases, the inputs meet their conditions (pool acceptance, kink share, the margins), the case tables hold every value
they name, and the dispatch of lerf_train.hip -- restated from the shapes in lerf_train_ref.dispatch -- takes every branch in at least one case."""
import numpy as np
import pytest

import lerf_train_ref as T
from conftest import load_golden
from oracle import capi as O
from test_oracle_golden import lerf_golden_case


def assert_close(got, ref, rtol, atol, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bad = np.abs(got - ref) > atol + rtol * np.abs(ref)
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} off, worst {np.abs(got - ref).max():.3e} (largest reference entry {np.abs(ref).max():.3e})"


# ------------------------------------------------------------------------------------------------ the model against reference autograd
@pytest.mark.parametrize("tag", ["train_lerf", "train_lerf_l3", "train_lerf_main"])
def test_model_reproduces_the_reference_autograd_goldens(tag, manifest):
    """The bars test_oracle_golden.py holds the oracle to: forward values to 1e-5 (weights 2e-5 / 2e-7, rendered 1e-4 / 2e-6), every gradient to 2e-4 of its tensor's
    largest entry, the loss to 2e-6 relative and its gradient to rtol 1e-5."""
    c, blob, g, where = lerf_golden_case(tag, manifest)
    dims = (c["in_ch"], c["n_layers"], c["hidden"], c["geo"], c["embed"])
    assert T.param_count(dims) == blob.size and [v[0] for v in T.param_slices(dims).values()] == [v[0] for v in where.values()]
    loss, g_r = T.huber_rows_nanmean(g["rendered"], g["target"])
    assert abs(loss - float(g["loss"][0])) <= 2e-6 * abs(float(g["loss"][0]))
    assert_close(g_r, g["grad_rendered"], 1e-5, 1e-9, "d loss / d rendered")
    r = T.model(blob, dims, g["emb"], g["keep"], g["z"], g["d"], g["grad_rendered"])
    assert_close(r["weights"], g["weights"], 2e-5, 2e-7, "WeightsLE")
    assert_close(r["rendered"], g["rendered"], 1e-4, 2e-6, "RenderedLangEmbedding")
    assert_close(r["g_emb"], g["grad_emb"], 0, 2e-4 * float(np.abs(g["grad_emb"]).max()), "d loss / d features")
    for name, (off, shape) in where.items():
        ref, mine = g["grad_" + name], r["g_params"][off:off + int(np.prod(shape))]
        if ref.size != mine.size:
            mine = mine[::c["stride"]]
        assert_close(mine, ref.reshape(-1), 0, 2e-4 * float(np.abs(ref).max()), f"d loss / d {name}")


def test_model_reproduces_the_nan_row_golden():
    g = load_golden("train_lerf_nan")
    loss, grad = T.huber_rows_nanmean(g["pred"], g["target"])
    assert abs(loss - float(g["loss"][0])) <= 1e-6 * abs(float(g["loss"][0]))
    ref = g["grad_pred"]
    assert (np.isnan(grad) == np.isnan(ref)).all()
    ok = ~np.isnan(ref)
    assert_close(grad[ok], ref[ok], 1e-6, 0, "d loss / d pred")


# ------------------------------------------------------------------------------------------------ the oracle against the model
def oracle_error(c, ref):
    """The CPU fp32 oracle's own error against the model, per output: max|orc - ref| / max|ref| (kink rays left out of the values) -> dict, + the oracle's outputs."""
    d = c["dims"]
    o = O.lerf_head_backward(c["blob"], c["emb"], c["keep"], c["z"], np.ascontiguousarray(c["d"][:, :3]), c["g_rendered"], in_ch=d[0], n_layers=d[1], hidden=d[2], geo=d[3],
                             embed=d[4], noise=c["noise"], noise_std=c["noise_std"])
    return T.compare(c, ref, o["weights"], o["rendered"], o["g_emb"], o["g_params"])


HOST_SPECS = T.sample_count_specs() + [sp for sp in T.threshold_specs() if sp[0] == T.SMALL] + [sp for sp in T.head_shape_specs() if sp[1] < 100 and max(sp[0]) <= 256]


@pytest.mark.parametrize("spec", HOST_SPECS, ids=lambda sp: "-".join(str(v) for v in sp[0]) + f"-n{sp[1]}-s{sp[2]}-{sp[3]}")
def test_oracle_agrees_with_the_model(spec):
    """orc_lerf_head_backward is the fp32 statement of the same chain: a few fp32 roundings per sum away from the model (its parameter gradients accumulate in double).
    The bar: 1e-4 of each output's scale -- the goldens' own bar for the oracle's gradients is 2e-4."""
    c = T.make_case(*spec)
    ref = T.case_model(c)
    e = oracle_error(c, ref)
    assert max(e.values()) < 1e-4, (c["tag"], e)


@pytest.mark.parametrize("n,e", [(n, e) for n in T.LOSS_N for e in T.LOSS_E])
@pytest.mark.parametrize("nan", ["none", "one", "edges", "all"])
def test_loss_oracle_agrees_with_the_model(n, e, nan):
    pred, target, rows = T.loss_case(n, e, nan)
    check_loss(pred, target, *O.huber_rows_nanmean(pred, target, T.DELTA))


def check_loss(pred, target, loss, grad):
    """The language loss's bars: 2e-6 relative, the gradient rtol 1e-5 where finite; the NaN pattern as the float64 model leaves it."""
    ref_loss, ref_grad = T.huber_rows_nanmean(pred, target)
    if np.isnan(ref_loss):
        assert np.isnan(loss)
    else:
        assert abs(loss - ref_loss) <= 2e-6 * abs(ref_loss), (loss, ref_loss)
    assert (np.isnan(grad) == np.isnan(ref_grad)).all(), f"NaN pattern: {np.isnan(grad).sum()} against {np.isnan(ref_grad).sum()} in the model"
    ok = ~np.isnan(ref_grad)
    assert_close(np.asarray(grad)[ok], ref_grad[ok], 1e-5, 1e-12, "d loss / d pred")


def test_loss_cases_hold_their_edges():
    pred, target, _ = T.loss_case(5, 64, "none")
    d = (pred - target)[0, :6]
    at = np.float32(T.DELTA)
    assert (np.abs(d[[0, 3]]) == at).all() and (np.abs(d[[1, 4]]) < at).all() and (np.abs(d[[2, 5]]) > at).all() and (np.diff(np.abs(d[:3]).view(np.int32)) != 0).all()
    assert abs(int(np.abs(d[1]).view(np.int32)) - int(at.view(np.int32))) == 1 and abs(int(np.abs(d[2]).view(np.int32)) - int(at.view(np.int32))) == 1
    big = np.abs(pred - target)
    assert (big > at).mean() > 0.2 and (big < at).mean() > 0.2
    assert T.loss_case(1025, 63, "edges")[2] == [3, 4, 255, 256] and len(T.loss_case(4, 1, "all")[2]) == 4
    assert set(T.LOSS_N) == {1, 3, 4, 5, 257, 1025} and set(T.LOSS_E) == {1, 63, 64, 65, 768}


# ------------------------------------------------------------------------------------------------ the conditions on the inputs
ALL_DIMS = sorted({sp[0] for sp in T.sample_count_specs() + T.threshold_specs() + T.head_shape_specs()} | {T.TINY, T.GEO0, T.LDS_LAYERWISE[0], T.LDS_GRAM[0]})


@pytest.mark.parametrize("dims", ALL_DIMS, ids=lambda d: "-".join(str(v) for v in d))
def test_pools_accept_at_least_half_of_their_draws(dims):
    N = T.net(dims)
    print(f"dims {dims}: {N.accepted:.3f} of {T.POOL_DRAWS} rows accepted at the margin 8 * 2^-16; sum|w||h| of the sigma row {N.sigma_bound:.3f}")
    assert N.accepted >= 0.5
    assert not N.pool[T.DEAD_ROW].any() and N.sigma[T.DEAD_ROW] == 0 and np.abs(N.pool[1:]).max() <= 0.5
    assert 8 * T.U_MARGIN * N.sigma_bound + 1e-6 < T.NUDGE, "a sample with noise keeps its density's sign in every arithmetic"
    assert T.U_MODE == {0: 2.0 ** -24, 1: 2.0 ** -16, 2: 2.0 ** -22} and T.U_MARGIN == 2.0 ** -16


def every_case():
    for sp in T.sample_count_specs() + T.threshold_specs() + T.head_shape_specs():
        yield T.make_case(*sp)
    for dims, n, s in (T.LDS_LAYERWISE, T.LDS_GRAM, (T.GEO0, 15, 17), (T.GEO0, 257, 17), T.ONE_HOT, T.UPLOAD):
        yield T.make_case(dims, n, s, "ordinary", T.SEED0 + 900 + n + s)
    for dims, n, s, _ in T.PASS_CASES:
        yield T.make_case(dims, n, s, "ordinary", T.SEED0 + 950 + n + s)


def test_kink_share_and_edges_of_every_case():
    worst = 0.0
    for c in every_case():
        if max(c["dims"]) > 256 and c["n"] * c["s"] > 4096 or c["n"] * c["s"] > 300000:
            continue                                             # (the model of these runs in the GPU test, which asserts the share there)
        ref = T.case_model(c)
        kink = T.kink_census(c, ref)
        worst = max(worst, kink.mean())
        assert kink.mean() <= T.MAX_KINK_SHARE, (c["tag"], kink.sum())
        if c["noise"] is not None:
            assert np.abs(ref["sigma"]).min() >= T.NUDGE - 1e-6, c["tag"]          # (the fp32 rounding of the noise)
        n, s = c["n"], c["s"]
        if c["masked_ray"] is not None:
            assert (ref["weights"][1] == 0).all() and (ref["rendered"][1] == 0).all() and (ref["g_emb"].reshape(n, -1)[1] == 0).all(), c["tag"]
        if n >= 3 and s > 1:
            assert c["idx"][s - 1] == T.DEAD_ROW and c["idx"][(n - 1) * s + (s - 1) // 2] == T.DEAD_ROW and c["idx"][n * s - 1] != T.DEAD_ROW
        if c["kind"] == "zero_sigma":
            assert not ref["weights"].any() and not ref["g_params"].any()
        elif c["kind"] == "negative_sigma":
            assert not ref["weights"].any(), c["tag"]
        elif c["kind"] in ("opaque_first", "opaque_at"):
            assert np.abs(ref["weights"][n - 1]).max() > 0 and (s < 3 or np.abs(ref["g_params"]).max() > 0), c["tag"]
    print(f"largest kink share of a case: {worst:.4f}")


# ------------------------------------------------------------------------------------------------ coverage of the tables and of the dispatch
def test_case_tables_hold_every_value_they_name():
    sc = T.sample_count_specs()
    assert {sp[2] for sp in sc} == set(T.SAMPLE_COUNTS) == {1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257}
    assert {(sp[2], sp[3]) for sp in sc} == {(s, k) for s in T.SAMPLE_COUNTS for k in T.KINDS} and len(T.KINDS) == 7
    assert {sp[1] for sp in sc} == {3, 5} and {sp[5] for sp in sc} == {"mask", "null"} and {sp[6] for sp in sc} == {3, 8}
    assert all(sp[0] == T.SMALL for sp in sc)
    for s in T.SAMPLE_COUNTS:                                    # pairs that select a code path: odd / even s (the alignment pad) x with / without a mask
        assert {sp[5] for sp in sc if sp[2] == s} == {"mask", "null"} or s in (1,), s
    assert {(sp[2] & 1, sp[5]) for sp in sc} == {(0, "mask"), (0, "null"), (1, "mask"), (1, "null")}
    th = T.threshold_specs()
    assert {(sp[0], sp[1], sp[2]) for sp in th} == {(d, n, s) for d in (T.SMALL, T.MAIN) for n, s in T.THRESHOLDS}
    assert sorted(n * s for n, s in T.THRESHOLDS) == [72, 255, 256, 4080, 4096, 4096, 4369] and T.MODES == (0, 1, 2, -1)
    hs = {d for d, _ in T.HEAD_SHAPES}
    assert {d[2] for d in hs} >= {24, 30, 32, 63, 64, 65, 100, 255, 256, 257} and {d[1] for d in hs} == {1, 2, 3}
    assert {d[4] for d in hs} >= {1, 40, 257, 768} and {d[0] for d in hs} >= {3, 13, 16, 128} and {d[3] for d in hs} >= {5, 8}
    assert {n * s >= 4096 for n, s in T.HEAD_SHAPE_SIZES} == {False, True}
    assert T.GEO0[3] == 0 and T.LDS_LAYERWISE[1:] == (3, 1500) and T.LDS_LAYERWISE[0][2] == 256 and T.LDS_LAYERWISE[0][4] == 40


def test_every_branch_of_the_dispatch_is_taken():
    """lerf_train_ref.dispatch restates lerf_train.hip's predicates; every branch is taken by at least one (case, mode, form) the GPU test runs.  A change of a
    threshold in the kernels' launcher shows here once dispatch() follows it."""
    runs = []
    for sp in T.sample_count_specs():
        runs += [T.dispatch(sp[0], sp[1], sp[2], -1, g) for g in (1, 0)]
    for sp in T.threshold_specs():
        runs += [T.dispatch(sp[0], sp[1], sp[2], m, g) for m in T.MODES for g in (1, 0)]
    for sp in T.head_shape_specs():
        runs += [T.dispatch(sp[0], sp[1], sp[2], m, 1) for m in (0, 1, 2)]
    runs += [T.dispatch(d, n, s, -1, g) for d, n, s, g in T.PASS_CASES]
    runs += [T.dispatch(*T.LDS_LAYERWISE, -1, 1), T.dispatch(*T.LDS_GRAM, -1, 1), T.dispatch(*T.ONE_HOT, 1, 1), T.dispatch(*T.UPLOAD, -1, 1)]
    seen = lambda **kw: any(all(r[k] == v for k, v in kw.items()) for r in runs)
    for gram in (True, False):
        for yo in (0, 3):
            assert seen(gram=gram, yo=yo), (gram, yo)
        assert seen(gram=gram, split_fwd=True) and seen(gram=gram, split_fwd=False)
        assert seen(gram=gram, passes=2), gram
    for m in (1, 2):
        assert seen(arith=m, arith_r=m) and seen(arith=m, arith_r=0), m
    assert seen(gram=True, arith=0, split_fwd=True), "256 <= c < 4096: split forward, fp32 Gram products"
    assert seen(gram=True, arith=0, c=4096) and seen(gram=True, arith=0, c=4369), "mode 0 above the threshold"
    assert seen(cat2="aligned") and seen(cat2="offset", yo=3) and seen(cat2="offset", yo=0) and seen(cat2=None, c=4369, split_fwd=True), "both variants of the two-segment product, and its refusal"
    assert seen(passes=3, gram=False) and seen(passes=2, gram=True) and seen(gram_from_packer=True)
    # the refusals of the Gram form, one by one
    assert not T.gram_form((16, 2, 257, 8, 48), 17) and not T.gram_form((16, 1, 32, 8, 48), 17) and T.gram_form((16, 2, 256, 8, 48), 17)
    d, n, s = T.LDS_LAYERWISE
    assert not T.gram_form(d, s) and not T.unsupported(d, s) and T.gram_form(T.LDS_GRAM[0], T.GRAM_S_MAX) and not T.gram_form(T.LDS_GRAM[0], T.GRAM_S_MAX + 1)
    assert T.unsupported(T.SMALL, T.UNSUPPORTED_S) and not T.unsupported(T.SMALL, T.UNSUPPORTED_S - 1)
    # passes: the even cut, and the pass boundaries the GPU test looks at
    for (d, n, s, g), (passes, rays) in zip(T.PASS_CASES, ((2, 1025), (3, 1366), (2, 2049))):
        r = T.dispatch(d, n, s, -1, g)
        assert (r["passes"], r["rays"]) == (passes, rays) and 0 < r["tail_rays"] <= rays, r
    r = T.dispatch(*T.ONE_HOT, 1, 1)
    assert r["arith"] and r["arith_r"] and r["passes"] == 1
