"""CPU tests that pin the yardsticks of tests/test_per_ray_gpu.py against each other: the C oracle's per-ray stages (orc_z_vals, orc_raw2outputs*, orc_raw2weights,
orc_raw2outputs_backward*, orc_sample_pdf*, orc_merge_sorted) against ATen's own fp32 ops where the bar is bit-exactness (SamplePDF) and against the float64 restatements
of tests/per_ray_ref.py everywhere else, on the very cases the GPU test runs.  The GPU kernels equal the oracle bit for bit, so the float64 bars measured here carry over."""
import numpy as np
import pytest

from oracle import capi as O
import per_ray_ref as PR

bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
MARGIN = 4.0          # bar = 4 x the largest error measured on this host over the committed cases: room for another host's libm / SLEEF


def test_cases_cover():
    """The drawn layout choices of the compositing cases reach every value and every pair that selects a code path."""
    specs = PR.composite_specs()
    for s in PR.SINGLE_S + PR.MERGED_S:
        assert {k for _, _, ss, _, k, *_ in specs if ss == s} == set(PR.COMPOSITE_KINDS)
    col = lambda i: {sp[i] for sp in specs}
    assert col(1) == set(PR.RAY_COUNTS) | {PR.BIG_N} and col(3) == {4, 5, 7} and col(5) == {False, True} and col(6) == {3, 11}
    assert {(sp[3] == 4, sp[7]) for sp in specs} == {(a, b) for a in (False, True) for b in (False, True)}, "c == 4 with raw aligned and not: the 16-byte row load and its fallback"
    for c in PR.cases("composite"):
        assert len(PR.noise_modes(c)) == (1 if c["kind"] == "zero_sigma" else 2), "every case but zero_sigma is composited without the sigma noise and with it"
    nws = {nb - 1 for nb in PR.PDF_NB}
    for vec in (4, 8, 16):
        assert {vec - 1, vec, vec + 1} <= nws
    assert {n for _, n, _, _ in PR.pdf_specs()} == set(PR.RAY_COUNTS) | {PR.BIG_N} and {n for _, n, _, _ in PR.fine_specs()} == set(PR.RAY_COUNTS) | {PR.BIG_N}
    for nb in PR.PDF_NB:
        assert [1 for _, n, b, ns in PR.pdf_specs() if b == nb and n >= 66 and ns >= 64], "every bin count has a batch with the all-zero and the spike rows"
    assert [1 for _, n, _, ns in PR.pdf_specs() if n >= 66 and ns == 1], "so has the single draw"


# ------------------------------------------------------------------ SamplePDF
@pytest.mark.parametrize("nb", PR.PDF_NB)
def test_sample_pdf_oracle_equals_aten(nb):
    """orc_sample_pdf / orc_sample_pdf_rand at sum_vec = 8 equal the Sampler.h chain in torch CPU fp32 ops bit for bit, indices and samples, on every case."""
    for spec in PR.pdf_specs():
        if spec[2] != nb:
            continue
        c = PR.pdf_case(*spec)
        for u, fn in ((c["u"], O.sample_pdf), (c["u_rand"], O.sample_pdf_rand)):
            got = fn(c["bins"], c["weights"], u, 8)
            want_s, want_i = PR.sample_pdf_aten(c["bins"], c["weights"], u)
            assert np.array_equal(got[1], want_i), (c["tag"], fn.__name__, "indices", int((got[1] != want_i).sum()))
            assert np.array_equal(bits(got[0]), bits(want_s)), (c["tag"], fn.__name__, "samples")


NEAR_ULP, NEAR_CAP = 4, 0.005


def pdf_indices_vs_float64(inds, c, u):
    """-> (number of draws whose index differs from the float64 definition's although no CDF entry lies within 4 fp32 ulp of the draw, number of draws left out, draws).
    Left out: draws whose index differs AND that lie within 4 ulp of a CDF entry (a subset of what may be left out)."""
    _, want, cdf = PR.sample_pdf_f64(c["bins"], c["weights"], u)
    u = np.broadcast_to(np.asarray(u, np.float64), want.shape)
    near = np.zeros(want.shape, bool)
    for k in (-1, 0):          # cdf[want - 1] <= u < cdf[want]: the two entries nearest to the draw
        e = np.take_along_axis(cdf, np.clip(want + k, 0, cdf.shape[1] - 1), 1)
        near |= np.abs(u - e) <= NEAR_ULP * np.spacing(np.maximum(np.abs(e), np.abs(u)).astype(np.float32)).astype(np.float64)
    diff = inds != want
    return int((diff & ~near).sum()), int((diff & near).sum()), want.size


@pytest.mark.parametrize("nb", PR.PDF_NB)
def test_sample_pdf_oracle_vs_float64(nb):
    """sum_vec = 0 (double-accumulated normaliser) gives the float64 definition's indices, except for draws within 4 fp32 ulp of a CDF entry: those may differ, are counted,
    and at most 0.5 % of a case's draws may be left out that way (per_ray_ref.PDF_SEEDS: the seeds at which the oracle itself stays under that cap)."""
    worst = 0.0
    for spec in PR.pdf_specs():
        if spec[2] != nb:
            continue
        c = PR.pdf_case(*spec)
        for u, fn in ((c["u"], O.sample_pdf), (c["u_rand"], O.sample_pdf_rand)):
            got = fn(c["bins"], c["weights"], u, 0)
            bad, left_out, total = pdf_indices_vs_float64(got[1], c, u)
            worst = max(worst, left_out / total)
            assert bad == 0, (c["tag"], fn.__name__, bad)
            assert left_out <= NEAR_CAP * total, (c["tag"], fn.__name__, left_out, total)
    print(f"nb {nb}: largest share of draws left out near a CDF entry {worst:.5f} (cap {NEAR_CAP})")


# ------------------------------------------------------------------ sort(cat(z, samples))
def test_merge_sorted_equals_stable_sort():
    """orc_merge_sorted == the stable numpy sort of cat(z, samples), values bit for bit, on every fine-depth case (det and random draws; rows with a swapped pair and rows
    where z and samples tie included)."""
    for c in PR.cases("fine"):
        for u, fn in ((c["u"], O.sample_pdf), (c["u_rand"], O.sample_pdf_rand)):
            smp = fn(O.z_mid(c["z"]), c["weights"][:, 1:-1], u)[0]
            want, _ = PR.merge_sorted(c["z"], smp)
            assert np.array_equal(bits(O.merge_sorted(c["z"], smp)), bits(want)), c["tag"]
            assert (np.diff(want, axis=1) >= 0).all()
        if c["s"] <= 3 and c["n"] >= 3:
            assert (smp[0] == c["z"][0, :1]).all(), "the tie rows: every sample equals the depths"


# ------------------------------------------------------------------ z_vals
def test_z_vals_oracle_vs_float64():
    """orc_z_vals against the float64 restatement.  Bar by reasoning, not measured: at most 6 fp32 roundings (two products and a sum; lindisp: three reciprocals more), each
    within 2^-24 of the largest intermediate -> 8 * 2^-24 relative to that scale (lin: max(|near|, |far|); lindisp: the result, its condition being 1)."""
    for c in PR.cases("z_vals"):
        near, far = c["rays"][:, 6], c["rays"][:, 7]
        got = O.z_vals(near, far, c["t"], c["lindisp"])
        want = PR.z_vals(near, far, c["t"], c["lindisp"])
        scale = np.abs(want) if c["lindisp"] else np.maximum(np.abs(near), np.abs(far)).astype(np.float64)[:, None]
        assert (np.abs(got - want) <= 8 * 2.0 ** -24 * scale).all(), c["tag"]


# ------------------------------------------------------------------ RawToOutputs forward
FWD_MEASURED = dict(weights=8.778e-7, rgb=3.188e-7, acc=4.569e-7, depth=2.583e-6, disp=1.655e-7)
FWD_BARS = {k: MARGIN * v for k, v in FWD_MEASURED.items()}
ACC_MIN = 0.1


def forward_errors(c, got, ref):
    """max |oracle - float64| per output of one case; depth and disp over the rays with acc >= 0.1 only (below, swz / sw divides rounding-level weights).
    -> (errors, share of rays left out of depth / disp)"""
    keep = ref["acc"].numpy() >= ACC_MIN
    err = {}
    for k in got:
        d = np.abs(got[k].astype(np.float64) - ref[k].detach().numpy())
        assert np.isfinite(got[k]).all(), (c["tag"], k)
        if k in ("depth", "disp"):
            d = d[keep]
        err[k] = float(d.max()) if d.size else 0.0
    return err, 1.0 - keep.mean()


def test_raw2outputs_forward_oracle_vs_float64():
    """orc_raw2outputs, orc_raw2outputs_noise (every case but zero_sigma, which has no draws) and orc_raw2weights (sigma_ch in {0, c - 1}) against the float64 restatement on every compositing
    case: absolute error per output, depth and disp on rays with acc >= 0.1 only.

    Measured on the committed cases / bar (= 4 x measured):
        weights  8.778e-07 / 3.511e-06      rgb  3.188e-07 / 1.275e-06      acc  4.569e-07 / 1.828e-06      depth  2.583e-06 / 1.033e-05      disp  1.655e-07 / 6.620e-07
    (depths lie in [2, 6]; the weight error is the fp32 rounding of the log-transmittance prefix, half an ulp of a value near -8, passed through exp.)
    Rays left out of depth / disp (acc < 0.1), mean / largest share over the cases of a kind: ordinary 0.061 / 1.0 (thin single rays), zero_sigma 1.0 / 1.0 and
    negative_sigma 0.77 / 1.0 (no weight at all: depth and disp are then compared bit for bit on the GPU), coincident 0.19 / 0.67, zero_dir 0.72 / 1.0 (every second ray has
    no length); opaque_first and opaque_at, the kinds with an opaque sample: 0 in every case (asserted: under half)."""
    worst, left = dict.fromkeys(FWD_BARS, 0.0), {}
    for c in PR.cases("composite"):
        err = dict.fromkeys(FWD_BARS, 0.0)
        for noise, std in PR.noise_modes(c):
            ref = PR.raw2outputs(c["raw"], c["z"], c["d"], c["white"], noise, std)
            if noise is None:
                got = O.raw2outputs(c["raw"], c["z"], c["d"], c["white"])
            else:
                got = O.raw2outputs_noise(c["raw"], c["z"], c["d"], noise, std, c["white"])
            e, out = forward_errors(c, got, ref)
            err = {k: max(v, e[k]) for k, v in err.items()}
            left.setdefault(c["kind"], []).append(out)
            if c["kind"] in ("opaque_first", "opaque_at"):
                assert out < 0.5, (c["tag"], out)
        for sigma_ch in (0, c["c"] - 1):
            refw = PR.raw2outputs(c["raw"], c["z"], c["d"], sigma_ch=sigma_ch)
            errw, _ = forward_errors(c, O.raw2weights(c["raw"], sigma_ch, c["z"], c["d"]), {k: refw[k] for k in ("weights", "depth", "disp", "acc")})
            err = {k: max(v, errw.get(k, 0.0)) for k, v in err.items()}
        for k, v in err.items():
            assert v <= FWD_BARS[k], (c["tag"], k, v, FWD_BARS[k])
            worst[k] = max(worst[k], v)
    print("RawToOutputs forward, oracle vs float64, max |error|: " + ", ".join(f"{k} {v:.3e} (bar {FWD_BARS[k]:.3e})" for k, v in worst.items()))
    print("share of rays left out of depth / disp, by kind (mean, max): " + ", ".join(f"{k} {np.mean(v):.3f} {np.max(v):.3f}" for k, v in left.items()))


# ------------------------------------------------------------------ RawToOutputs backward
BWD_MEASURED = 9.551e-7
BWD_BAR = MARGIN * BWD_MEASURED
KINK_CAP = 0.02


def test_raw2outputs_backward_oracle_vs_float64():
    """orc_raw2outputs_backward and orc_raw2outputs_backward_noise (every case but zero_sigma, which has no draws) against autograd through the float64 restatement, on every compositing case.
    Error of a case: max |oracle - float64| / max |float64| (the largest entry of the case's gradient; a case whose float64 gradient is all zero must be all zero).
    Rays with a sample on a kink (per_ray_ref.kink_rays) are left out, at most 2 % of a case's rays; the cases built on the clamp (opaque_first, opaque_at) compare the
    rgb columns only, which have no kink; zero_sigma has every sample on the relu's kink but no noise, so both precisions take the same branch: nothing is left out there.

    Measured on the committed cases: 9.551e-07; bar (= 4 x measured): 3.820e-06.  Rays left out as kinks on the committed seeds: at most 1 of 66 (0.0152) in a case."""
    worst, worst_kink = 0.0, 0.0
    for c in PR.cases("composite"):
        for noise, std in PR.noise_modes(c):
            want = PR.raw2outputs_grad(c["raw"], c["z"], c["d"], c["g_rgb"], c["white"], noise, std)
            if noise is None:
                got = O.raw2outputs_backward(c["raw"], c["z"], c["d"], c["g_rgb"], c["white"])
            else:
                got = O.raw2outputs_backward_noise(c["raw"], c["z"], c["d"], c["g_rgb"], noise, std, c["white"])
            assert np.isfinite(got).all() and not got[..., 4:].any(), c["tag"]
            cols = slice(0, 3) if c["kind"] in ("opaque_first", "opaque_at") else slice(0, 4)
            keep = np.ones(c["n"], bool)
            if c["kind"] not in ("opaque_first", "opaque_at", "zero_sigma"):
                keep = ~PR.kink_rays(c["raw"], c["z"], c["d"], noise, std)
                assert (~keep).mean() <= KINK_CAP, (c["tag"], std, (~keep).mean())
                worst_kink = max(worst_kink, (~keep).mean())
            g, w = got[keep][..., cols].astype(np.float64), want[keep][..., cols]
            top = np.abs(w).max() if w.size else 0.0
            if top == 0.0:
                assert not g.any(), c["tag"]
                continue
            err = float(np.abs(g - w).max() / top)
            assert err <= BWD_BAR, (c["tag"], std, err, BWD_BAR)
            worst = max(worst, err)
    print(f"RawToOutputs backward, oracle vs float64 autograd: max |error| / max |gradient| = {worst:.3e} (bar {BWD_BAR:.3e}); largest share of rays left out as kinks {worst_kink:.4f}")
