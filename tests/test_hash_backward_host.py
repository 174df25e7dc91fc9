"""CPU checks of tests/hash_backward_ref.py, the yardstick of tests/test_hash_backward_gpu.py: the numpy restatement of the hash-grid table gradient against the forward
restatements of tests/hash_shapes_ref.py (adjoint identity), against the C oracle's exact accumulation (equality), the sanity of every input the GPU tests use, and the
search for an input that overflows a fixed-point field of the packed / binned backward (k_level_mass's outside-box bound)."""
import itertools

import numpy as np
import pytest

import hash_backward_ref as B
import hash_shapes_ref as HS

O = HS.O
f32, f64 = np.float32, np.float64


def some_points(case, n=1500):
    """every kind of hash_shapes_ref.points() and a gradient with zero rows, zero levels and zero features"""
    x, kinds = HS.points(case, n=n, seed=3)
    g = B.grads(case, x.shape[0], 1, np.zeros(x.shape[0], np.int64), "signed", seed=9)
    return x, kinds, g


# ------------------------------------------------------------------ adjoint identity
@pytest.mark.parametrize("case", B.GRIDS, ids=HS.case_id)
def test_scatter_is_the_adjoint_of_the_encoder(case):
    """<g, encode(table)> == <scatter(g), table> with the forward restatements HS.ref_hash_ngp / HS.ref_hash_cu, which were written against the reference's forward and share
    no code with the backward restatement: a wrong corner, a swapped axis, a wrong row or level offset breaks it.
    HashEmbedder mode: both sides in their own fp32 (the forward's nested blend rounds 9 times per term: three 1 - w, three products, three sums; the backward's product 6
    times), summed in float64 -- they agree to 16 * 2^-24 of sum |g| |w| |table|.  CuHashEmbedder mode: the forward rounds its OUTPUT to fp16 (2^-11 of each feature) and
    reads the fp16 table, so the scatter is taken with un-rounded weights (g * w in float64, the same fp32 w) over the fp16 table; the fp16 roundings of the backward's own
    addends are held against the oracle in test_exact_sum_equals_the_oracle."""
    x, kinds, g = some_points(case)
    table = HS.table_of(case)
    L, F = case.L, case.F
    if case.mode == "ngp":
        feat, _ = HS.ref_hash_ngp(x, table, case.bbox, L, F, case.T, case.base, case.finest)
        ex = B.exact(case, x, g)
        lhs = float((g.astype(f64) * feat.astype(f64)).sum())
        rhs = float((ex.R * table.astype(f64)).sum())
        tol = 16 * 2.0 ** -24 * float((ex.A * np.abs(table.astype(f64))).sum())
    else:
        feat, _ = HS.ref_hash_cu(case, x, table)
        t16 = table.astype(np.float16).astype(f64)
        S, A = np.zeros(table.size, f64), np.zeros(table.size, f64)
        for l in range(L):
            pos, w8 = B.cu_weights(case, l, x)
            elem = B.level_elems(case, l, pos)
            for k in range(8):
                v = g[:, l * F:(l + 1) * F].astype(f64) * w8[:, k].astype(f64)[:, None]
                S += np.bincount(elem[:, k].ravel(), v.ravel(), table.size)
                A += np.bincount(elem[:, k].ravel(), np.abs(v).ravel(), table.size)
        lhs = float((g.astype(f64) * feat.astype(f64)).sum())
        rhs = float((S * t16).sum())
        tol = 2.0 ** -11 * float((np.abs(g).astype(f64) * np.abs(feat).astype(f64)).sum()) + 16 * 2.0 ** -24 * float((A * np.abs(t16)).sum())
    print(f"{case.name}: <g, encode> {lhs:.9e}  <scatter, table> {rhs:.9e}  diff {abs(lhs - rhs):.3e}  tol {tol:.3e}")
    assert tol < 1e-2 * max(abs(lhs), abs(rhs)) or case.mode == "cu", "the tolerance resolves the sum"
    assert abs(lhs - rhs) <= tol, (case.name, lhs, rhs, tol)


# ------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("case", B.GRIDS, ids=HS.case_id)
def test_exact_sum_equals_the_oracle(case):
    """float32(R) == O.hash_ngp_backward / O.hash_cu_backward, which accumulate the same fp32 addends in double, on every grid: the oracle takes the box, and in CU mode the
    level scales, biases, primes and local sizes, so it expresses every case here (none is left out).  exact(point_major=True) adds in the oracle's order, so the doubles
    are the same doubles; the level-by-level form the GPU tests use may differ from it by double rounding only."""
    x, kinds, g = some_points(case)
    ex = B.exact(case, x, g, point_major=True)
    if case.mode == "ngp":
        ref = O.hash_ngp_backward(x, case.bbox, case.L, case.F, case.T, case.base, case.finest, g).reshape(-1)
    else:
        ls = HS.local_size_of(case)
        bias = np.zeros((case.L, 3), f32) if case.biases is None else case.biases
        ref = O.hash_cu_backward(x, HS.primes_of(case), np.arange(case.L, dtype=np.int32) * ls, np.full(case.L, ls, np.int32), bias, case.bbox, HS.level_scales(case),
                                 case.L, case.F, B.table_elems(case), g)
    assert (ref != 0).mean() > 0.01
    bad = np.nonzero(ex.R.astype(f32) != ref)[0]
    assert bad.size == 0, f"{case.name}: {bad.size} elements differ, first {bad[0]}: {ex.R[bad[0]]!r} vs {ref[bad[0]]!r}"
    by_level = B.exact(case, x, g)
    assert np.array_equal(by_level.k, ex.k)
    assert (np.abs(by_level.R - ex.R) <= 2.0 ** -52 * ex.k * ex.A).all() and (np.abs(by_level.A - ex.A) <= 2.0 ** -52 * ex.k * ex.A).all()
    val, elem, live = B.addends(case, x[:50], g[:50])
    assert val.shape == (50, case.L, 8, case.F) and elem.shape == val.shape and live.shape == (50, case.L)
    assert (val[~live] == 0).all() and elem.min() >= 0 and elem.max() < B.table_elems(case)


# ------------------------------------------------------------------ the inputs of the GPU tests
@pytest.mark.parametrize("run", B.FLOAT_RUNS, ids=B.run_id)
def test_float_run_inputs(run):
    """at least 5 % of the table elements a run touches end non-zero (a gradient that is all zero, or cancels, would let anything pass); fp16(g * 128) stays finite"""
    name, n, s, pattern = run
    case = B.BY_NAME[name]
    i = B.inputs(name, n, s, pattern)
    ex = B.exact(case, i.pts, i.g) if (n * s * case.L * case.F > 1 << 22) else B.expected_exact(name, n, s, pattern)
    assert np.isfinite(i.pts).all() and np.abs(i.g).max() * 128 < 65504
    touched = ex.k > 0
    assert touched.any() and (ex.R[touched] != 0).mean() >= 0.05, (touched.sum(), (ex.R[touched] != 0).mean())
    if n >= len(B.RAY_KINDS):
        assert set(i.kind.tolist()) == set(range(len(B.RAY_KINDS)))
    if pattern == "subnormal":
        l = case.L - 1
        t = B.level_terms(case, l, i.pts, i.g)
        g16 = (i.g[:, -case.F:] * f32(128)).astype(np.float16).astype(f32)
        assert (g16 == 0).any() and (g16 != 0).any() and np.abs(g16).max() <= 2.0 ** -14, "fp16 subnormals, some flushed to zero by the rounding"
        product = np.abs(g16.astype(f64))[:, None, :] * B.cu_weights(case, l, i.pts)[1].astype(f64)[:, :, None]          # before its rounding to fp16
        got = np.abs(t.val.astype(f64)) * 128
        assert ((got == 0) & (product > 0)).any(), "addends that round to zero"
        assert ((got > product) & (product < 2.0 ** -24)).any(), "addends below the smallest subnormal that round up to it"


@pytest.mark.parametrize("run", B.FIXED_RUNS, ids=B.run_id)
def test_fixed_point_run_inputs(run):
    """The model's own conditions on every input of the fixed-point GPU runs: no group's mass bound within 1e-9 (relative) of a power of two -- the device sums the masses with
    double-precision atomics in no fixed order, which moves the bound by ~1e-16 and must not move its exponent; no field total near 2^31; the side-list runs send between 1
    and 128 pairs per level through the list in some pass; and the model meets the exact sum within its own rounding budget, so the budget is not vacuous."""
    name, n, s, pattern = run
    case = B.BY_NAME[name]
    i = B.inputs(name, n, s, pattern)
    m = B.expected_model(name, n, s, pattern) if n * s < 1 << 16 else B.fixed_point_model(case, i.pts, n, s, i.g, i.base)
    assert len(m.units) == -(-n // max(1, B.GROUP_PTS // s))
    for b in m.bounds:
        assert b > 0
        mant = np.frexp(b * 1.01)[0]                    # in [0.5, 1)
        assert mant - 0.5 > 1e-9 and 1.0 - mant > 1e-9, (name, b)
    assert m.max_total < 2 ** 30, "fields stay in int32 with room"
    if run in B.SIDE_RUNS:
        assert any(1 <= c <= B.SIDE_PER_LEVEL for g in m.side for c in g) and all(c <= B.SIDE_PER_LEVEL for g in m.side for c in g), m.side
        assert sum(m.side[-1]) > 0, "the last pass has a side list to read back"
    ex = B.exact(case, i.pts, i.g)
    err = np.abs(m.table.astype(f64) - (i.base.astype(f64) + ex.R))
    tol = B.fixed_point_tolerance(m, i.base, ex)
    assert (err <= tol).all(), (name, float((err - tol).max()))
    assert (m.table != i.base).any()


# ------------------------------------------------------------------ the bound of k_level_mass
def test_outside_box_bound_of_the_level_mass():
    """k_level_mass multiplies the mass of a HashEmbedder-mode point e_a finest cells outside the box by prod (1 + 1.001 e_a) and calls the result a bound on what a table entry
    can collect.  Below the box's minimum the weights are 1 + e and -e, and the POSITIVE corner products of a point alone sum to (1 + e)^3 + 3 (1 + e) e^2 on three axes: more
    than the factor.  Whether a 32-bit field can overflow depends on which corners share a table entry.  Searched here with the exact model: T = 2 .. 6, a pile outside on two
    and on three axes in every combination of below / above, e = 1.5 .. 4 finest cells, one sign, the scale at its finest.

    Outcome.  The largest field total is (factor the entry collects / factor of the bound) * 2^30 / 1.01:
      T = 2       three axes below the minimum: all four positive corners (000, 011, 101, 110) hash to entry 0 and the four negative ones to entry 1 (the low two bits of
                  1, 2654435761 and 805459861 are all 01).  |total| / 2^31 = 1.03 at e = 1.5 .. 1.44 at e = 4: the field WRAPS.  With one of the three axes above the
                  maximum instead it wraps from e = 3.5 on (1.12 at e = 4); nothing else in the range does.
      T = 3, 4    entry 0 collects 000 and 110 only: (1 + e)^3 + (1 + e) e^2, 0.81 * 2^31 at e = 4 and below 0.99 * 2^31 for any e (the ratio tends to 2, the scale leaves 2.02).
      T = 5, 6    the positive corners fall apart: 0.494 * 2^31, the bound itself.
      two axes    at most (1 + e)^2 + e^2 (T <= 4): 0.55 * 2^31 at e = 4, below 2^31 for any e.
    nrf_hash_create refuses log2_hashmap_size < 4, so the overflowing input cannot be given to the library: no kernel change is made, and the worst input that CAN be built
    (T = 4, three axes below, e = 4: 0.810) is the GPU case ngp-outside-pile.  If tables below 2^4 rows are ever admitted, prod (1 + 2 e_a) -- the sum of |weights| of a point --
    is the factor that bounds every subset of corners."""
    worst, wrapped = {}, {}
    for T in range(2, 7):
        for side in itertools.product((-1, 0, 1), repeat=3):
            if sum(1 for v in side if v) < 2:
                continue
            for e in (1.5, 2.0, 2.5, 3.0, 3.5, 4.0):
                case, pts, g = B.pile_outside(T, side, e)
                m = B.fixed_point_model(case, pts, 8, 16, g, np.zeros(B.table_elems(case), f32))
                r = m.max_total / 2.0 ** 31
                if r > worst.get(T, (0,))[0]:
                    worst[T] = (r, side, e)
                if r >= 1.0:
                    wrapped.setdefault(T, []).append((side, e))
                    ex = B.exact(case, pts, g)
                    assert np.abs(m.table.astype(f64) - ex.R).max() > 0.5 * np.abs(ex.R).max(), "the wrapped field is far from the sum"
    print({T: (round(v[0], 4), v[1], v[2]) for T, v in worst.items()})
    assert set(wrapped) == {2} and all(0 not in side and side.count(-1) >= 2 for side, e in wrapped[2]), wrapped
    assert [e for side, e in wrapped[2] if side == (-1, -1, -1)] == [1.5, 2.0, 2.5, 3.0, 3.5, 4.0]
    assert worst[2][0] == pytest.approx(1.442, abs=2e-3)
    assert (worst[4][0], worst[4][1], worst[4][2]) == (pytest.approx(0.810, abs=2e-3),) + B.PILE_WORST_BUILDABLE[1:]
    assert worst[3][0] == pytest.approx(0.810, abs=2e-3) and worst[5][0] == pytest.approx(0.494, abs=2e-3) and worst[6][0] == pytest.approx(0.494, abs=2e-3)
    assert max(worst[T][0] for T in (4, 5, 6)) < 1.0, "no input the library accepts reaches 2^31 units in this range"
