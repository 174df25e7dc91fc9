"""GPU tests of the classic NeRF network's kernels on exact integer networks (mlp_nerf_mfma.hip, mlp_nerf_split_mfma.hip; mlp.hip: mlp_nerf_backward, the device
repack; gemm_f32.hip, gemm_bf16x3.hip).  Cases and the float64 yardstick are tests/mlp_nerf_ref.py's, which tests/test_mlp_nerf_shapes_host.py pins against the C
oracle on the CPU.  On those networks every arithmetic the library has gives the float64 result exactly, so every comparison below except (d) is EQUALITY.

Which test runs which kernel or branch (shapes: 'built' = 8 x 256 skip 4 with view directions, 'w64' = 4 x 64 skip 1 with view directions, 'w160' = 3 x 160 skip 0
without; modes are nrf_set_train_gemm's: 0 fp32 products, 1 bf16x3, 2 f16x3):
  k_mlp_nerf_mfma<false> (rows form, fp16) and k_mlp_nerf_split (rows form), tails on both sides of the 256- / 128-point block,
    a second persistent iteration of workgroup 0 (256 blocks + 1 point) ............ test_forward_rows_exact[built]
  forward_f32 (mlp.hip's FMA layer kernels) on all three shapes; the refusal of the
    matrix-core precisions outside the built family ................................ test_forward_rows_exact[built | w64 | w160]
  k_merge_views, the three gather maps of nrf_mlp_set_params from device memory,
    the host repack of the same handle .............................................. test_set_params_on_the_device_is_exact
  mlp_nerf_backward, per parameter tensor and g_x:
    fewer than 256 points: mlp.hip's fp32 kernels in every mode (k_linear, k_grad_w, k_grad_b, k_relu_mask, k_sum_rank1, k_sum_cols) ... test_backward_exact, p = 1, 255
    mode 0, 256 points and more: rocBLAS sgemm products where nrf_fp32_gemm_available() (else the same fp32 kernels) + k_bias_relu .... test_backward_exact[*-mode0]
    modes 1, 2, 256 points and more: gemm_nt_split forward products with bias + ReLU in the epilogue; ReLU masks fused into the back-propagation
      products' write-out (run_backprop_fuses_mask); the masks as bits on built and w160 (gemm_nt_bits_ok: 128 < N <= 256), as floats on w64; the rank-1 alpha
      addend inside feature_linear's back-propagation (built, w64); the skip layer's partial product on rows [in_ch, in_ch + w) of W^T with d_g_x = NULL, the
      whole product + k_sum_cols with d_g_x given; k_backprop_thin through rgb_linear (built, w64; output_linear's 223 inputs are no multiple of 4 and take
      the tile kernel) ............................................................................................................... test_backward_exact[*-mode1 | *-mode2]
    the weight gradients' split-precision products (gemm_tn_bf16x3, gemm_tn_bf16x3_2 with the bias sums, gemm_tn_thin) start at 4 096 points ... test_backward_exact_weight_gradient_products
  the same on a random network, per tensor against float64 ............................ test_backward_random_network_per_tensor
Every GPU step runs once."""
import numpy as np
import pytest
import torch

import mlp_nerf_ref as MN
from test_mlp_nerf_shapes_host import random_network, kink_free_batch

pytestmark = pytest.mark.gpu

NRF_OK, NRF_ERR_UNSUPPORTED = 0, 3
SEED_A, SEED_B = 11, 12
host = lambda t: t.detach().cpu().numpy()
P = lambda t: None if t is None else t.data_ptr()


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from types import SimpleNamespace
    from nerfpp_amd import _lib as L, modules as M
    return SimpleNamespace(L=L, M=M, lib=L.lib(), PRECS=(("f32", L.NRF_PREC_F32), ("f16", L.NRF_PREC_F16_MFMA), ("split", L.NRF_PREC_F16_SPLIT)))


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype, order="C")).cuda()          # (a copy: the cases are shared read-only arrays)


def equals64(got, want64, what):
    """float32 results against float64 integers: equal as numbers; the first differing index is reported"""
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    assert got.shape == want64.shape, (what, got.shape, want64.shape)
    bad = np.nonzero(~(got == want64).reshape(-1))[0]          # (a NaN differs)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[:5]}: {got.reshape(-1)[bad[:3]]} vs {want64.reshape(-1)[bad[:3]]}"


def nerf(api, shape, blob):
    d, w, in_ch, in_views, out_ch, skip, vd = shape
    return api.M.NeRF(d, w, in_ch, in_views, out_ch, (skip,), vd, "model", params=blob)


def forward_into_nan(api, m, xd, p, prec, od):
    """nrf_mlp_forward into a NaN-filled buffer of p + 3 rows -> (status, the buffer on the host)"""
    out = torch.full((p + 3, od), float("nan"), device="cuda")
    rc = api.lib.nrf_mlp_forward(m._m, P(xd), p, prec, P(out), None)
    torch.cuda.synchronize()
    return rc, host(out)


# ------------------------------------------------------------------ (a) forward, rows form
COUNTS = (1, 255, 257, 700)
SPLIT_COUNTS = (127, 129)                                   # both sides of the split kernel's 128-point block
SECOND_ITERATION = {"f16": 256 * 256 + 1, "split": 256 * 128 + 1}          # one point past the persistent grid's reach (256 workgroups x NBLK / SNBLK points)


@pytest.mark.parametrize("shape", MN.SHAPES, ids=MN.shape_id)
def test_forward_rows_exact(api, shape):
    """nrf_mlp_forward on the integer networks.  The built shape in NRF_PREC_F32, NRF_PREC_F16_MFMA and NRF_PREC_F16_SPLIT: rows < p EQUAL forward64, rows >= p of the
    NaN-filled buffer stay NaN -- at 1, 255, 257 and 700 points, at 127 and 129 in split precision, and one point past the persistent grid (tiled inputs), where
    workgroup 0 walks the weight stream a second time.  A wrong k-step, perm_row, skip operand, merged-layer entry or alpha row shows at full size.  The other shapes:
    NRF_PREC_F32 equals forward64; the matrix-core precisions answer NRF_ERR_UNSUPPORTED with a message and write nothing."""
    od = MN.out_dims(shape)
    blob = MN.integer_network(shape, SEED_A, 1)[0]
    m = nerf(api, shape, blob)
    built = shape == MN.BUILT
    counts = {name: list(COUNTS if built else (1, 257, 700)) for name, _ in api.PRECS}
    if built:
        counts["split"] += list(SPLIT_COUNTS) + [SECOND_ITERATION["split"]]
        counts["f16"] += [SECOND_ITERATION["f16"]]
    for p in sorted({c for cs in counts.values() for c in cs}):
        if p > 700:
            _, x, _, want, _ = MN.integer_network(shape, SEED_A, MN.TILE_ROWS)
            x, want = MN.tiled(x, p), MN.tiled(want, p)
        else:
            _, x, _, want, _ = MN.integer_network(shape, SEED_A, p)
        xd = dev(x)
        for name, prec in api.PRECS:
            if p not in counts[name]:
                continue
            rc, got = forward_into_nan(api, m, xd, p, prec, od)
            what = f"{MN.shape_id(shape)} {name} p {p}"
            if built or name == "f32":
                assert rc == NRF_OK, (what, rc, api.lib.nrf_last_error())
                assert np.isnan(got[p:]).all(), what + ": rows past the batch were written"
                equals64(got[:p], want, what)
            else:
                assert rc == NRF_ERR_UNSUPPORTED, (what, rc)
                assert len(api.lib.nrf_last_error()) > 0, what + ": a refusal says why"
                assert np.isnan(got).all(), what + ": a refused call wrote to the output"


# ------------------------------------------------------------------ (b) nrf_mlp_set_params on the device
def test_set_params_on_the_device_is_exact(api):
    """A handle created from integer network A and moved to network B by nrf_mlp_set_params from DEVICE memory computes B's forward64 exactly in all three
    precisions: the device-side merged layer (views_linears_0 o feature_linear) and the three gather maps (fp16 image, split image, the exact sigma kernel's) are
    right entry for entry, not merely the same as a fresh handle's.  Moved back to A from HOST memory, it computes A's.  nrf_mlp_device_repack_images counts the
    maps: 7 for the built family; 0 would be the host repack."""
    shape, p = MN.BUILT, 257
    blob_a, x, _, want_a, _ = MN.integer_network(shape, SEED_A, p)
    blob_b = MN.integer_network(shape, SEED_B, p)[0]
    assert not np.array_equal(blob_a, blob_b)
    m = nerf(api, shape, blob_a)
    assert api.lib.nrf_mlp_device_repack_images(m._m) == 7
    # B on A's batch: one batch throughout, so only the parameters move; the integer conditions are asserted for this pairing like for any other
    want_b_on_x = MN.check_integer_network(blob_b, x, np.zeros((p, 4), np.float32), shape, batch=False)[0]
    assert not np.array_equal(want_b_on_x, want_a)
    xd, bd = dev(x), dev(blob_b)
    api.L.check(api.lib.nrf_mlp_set_params(m._m, P(bd), 1, None))
    for name, prec in api.PRECS:
        rc, got = forward_into_nan(api, m, xd, p, prec, 4)
        assert rc == NRF_OK, (name, rc, api.lib.nrf_last_error())
        equals64(got[:p], want_b_on_x, f"{name}: after nrf_mlp_set_params from device memory")
    a_host = np.ascontiguousarray(blob_a, np.float32)
    api.L.check(api.lib.nrf_mlp_set_params(m._m, a_host.ctypes.data, 0, None))
    for name, prec in api.PRECS:
        rc, got = forward_into_nan(api, m, xd, p, prec, 4)
        assert rc == NRF_OK, (name, rc, api.lib.nrf_last_error())
        equals64(got[:p], want_a, f"{name}: after nrf_mlp_set_params from host memory")


# ------------------------------------------------------------------ (c) backward, exact, per tensor
BWD_COUNTS = (1, 255, 256, 257, 700)                        # both sides of the npts >= 256 switch between mlp.hip's fp32 kernels and the library / split products
GUARD, GUARD_BYTE, SCRATCH_BYTE = 64, 0xA5, 0xFF            # (a workspace of 0xFF bytes is all NaN: scratch that is read before it is written shows)
PREFILLED = (1, 257)                                        # counts at which d_g_params starts from a pattern, not from zero


def pattern(n):
    return ((np.arange(n) % 7) - 3).astype(np.float32)


def run_backward(api, m, shape, x, g, p, with_gx, prefill, ws_short=0):
    """one nrf_mlp_backward call on a workspace of exactly the asked size (less ws_short) with a guard behind it -> (status, g_params, g_x or None, guard intact)"""
    n = MN.n_params(shape)
    nb = int(api.lib.nrf_mlp_backward_workspace_bytes(m._m, p))
    assert nb > 0
    ws = torch.full((nb + GUARD,), SCRATCH_BYTE, dtype=torch.uint8, device="cuda")
    ws[nb:] = GUARD_BYTE
    gp = dev(pattern(n)) if prefill else torch.zeros(n, device="cuda")
    gx = torch.full((p + 3, shape[2]), float("nan"), device="cuda") if with_gx else None
    rc = api.lib.nrf_mlp_backward(m._m, P(x), P(g), p, P(gp), P(gx), P(ws), nb - ws_short, None)
    torch.cuda.synchronize()
    return rc, host(gp), None if gx is None else host(gx), bool((ws[nb:] == GUARD_BYTE).all())


def compare_backward(shape, got_p, got_x, want_p, want_x, p, prefill, what):
    base = pattern(got_p.size).astype(np.float64) if prefill else 0.0
    want_p = want_p + base
    for name, off, dims in MN.tensors(shape):
        n = int(np.prod(dims))
        equals64(got_p[off:off + n], want_p[off:off + n], f"{what} d / d {name}")
    if got_x is not None:
        assert np.isnan(got_x[p:]).all(), what + ": g_x rows past the batch were written"
        equals64(got_x[:p], want_x, what + " g_x")


@pytest.mark.parametrize("mode", (0, 1, 2), ids=lambda mode: "mode%d" % mode)
@pytest.mark.parametrize("shape", MN.SHAPES, ids=MN.shape_id)
def test_backward_exact(api, shape, mode):
    """nrf_mlp_backward on the integer networks at 1, 255, 256, 257 and 700 points, with d_g_x and with d_g_x = NULL (the trainer's call), in one nrf_set_train_gemm
    mode: every entry of every parameter tensor -- the 1-element alpha_linear.bias, the 3-element rgb_linear.bias and the input_pts columns of the skip layer among
    them -- EQUALS backward64, and so do rows < p of g_x; its rows >= p stay NaN.  d_g_params is accumulated into: at 1 and 257 points it starts from a pattern and
    ends at pattern + gradient.  The workspace is exactly nrf_mlp_backward_workspace_bytes(m, p) bytes of 0xFF (NaN) with 64 guard bytes behind it that stay as
    they were; one byte less is refused with a message before anything is launched: d_g_params keeps its pattern."""
    prev = api.lib.nrf_get_train_gemm()
    blob = MN.integer_network(shape, SEED_A, 1)[0]
    m = nerf(api, shape, blob)
    fp32 = "rocBLAS sgemm" if api.lib.nrf_fp32_gemm_available() else "mlp.hip's fp32 kernels"
    try:
        api.L.check(api.lib.nrf_set_train_gemm(mode))
        for p in BWD_COUNTS:
            _, x, g, _, (want_p, want_x) = MN.integer_network(shape, SEED_A, p)
            xd, gd = dev(x), dev(g)
            for with_gx in (True, False):
                what = f"{MN.shape_id(shape)} mode {mode} p {p} {'with g_x' if with_gx else 'g_x NULL'}"
                rc, got_p, got_x, guard = run_backward(api, m, shape, xd, gd, p, with_gx, p in PREFILLED)
                assert rc == NRF_OK, (what, rc, api.lib.nrf_last_error())
                assert guard, what + ": bytes behind the workspace were written"
                compare_backward(shape, got_p, got_x, want_p, want_x, p, p in PREFILLED, what)
            if p == 257:
                what = f"{MN.shape_id(shape)} mode {mode} p {p}, a workspace one byte short"
                rc, got_p, got_x, guard = run_backward(api, m, shape, xd, gd, p, True, True, ws_short=1)
                assert rc != NRF_OK and len(api.lib.nrf_last_error()) > 0, (what, rc)
                assert guard and np.array_equal(got_p, pattern(got_p.size)) and np.isnan(got_x).all(), what + ": the refused call wrote something"
        print(f"{MN.shape_id(shape)} mode {mode}: exact at {BWD_COUNTS} points; the fp32 products at 256 points and more are {fp32 if mode == 0 else 'not used'}")
    finally:
        api.L.check(api.lib.nrf_set_train_gemm(prev))


WEIGHT_GRADIENT_COUNT = 4097                                # run_grad_w_fast / run_grad_wb_fast: the split-precision weight-gradient products start at 4 096 points


@pytest.mark.parametrize("mode", (1, 2), ids=lambda mode: "mode%d" % mode)
def test_backward_exact_weight_gradient_products(api, mode):
    """The built shape at 4 097 points (one past the threshold, ragged against every tile): the weight gradients come from gemm_tn_bf16x3, from gemm_tn_bf16x3_2
    with the bias sums riding along (out >= 32) and from gemm_tn_thin (rgb_linear's 3 rows, alpha_linear's 1), which the counts of test_backward_exact never reach.
    The integer conditions are asserted for this batch like for any other (sums of |terms| stay below 2^24), so every tensor EQUALS backward64 again."""
    shape, p = MN.BUILT, WEIGHT_GRADIENT_COUNT
    prev = api.lib.nrf_get_train_gemm()
    blob, x, g, _, (want_p, want_x) = MN.integer_network(shape, SEED_A, p)
    m = nerf(api, shape, blob)
    try:
        api.L.check(api.lib.nrf_set_train_gemm(mode))
        for with_gx in (True, False):
            what = f"{MN.shape_id(shape)} mode {mode} p {p} {'with g_x' if with_gx else 'g_x NULL'}"
            rc, got_p, got_x, guard = run_backward(api, m, shape, dev(x), dev(g), p, with_gx, not with_gx)
            assert rc == NRF_OK, (what, rc, api.lib.nrf_last_error())
            assert guard, what + ": bytes behind the workspace were written"
            compare_backward(shape, got_p, got_x, want_p, want_x, p, not with_gx, what)
    finally:
        api.L.check(api.lib.nrf_set_train_gemm(prev))


# ------------------------------------------------------------------ (d) backward, random network, per tensor
RANDOM_POINTS = 700
CAPS = {1: 3e-3, 2: 3e-4}                                   # the blob-wide bars of test_classic_and_lerf_train_steps_in_the_split_gemm_modes_follow_the_fp32_chain: no bar exceeds them
# e(mode, tensor) = max |g - g64| / max |g64| as measured on the MI355X (profiles/mlp_nerf_shapes/measured_errors.txt holds the table and the bars): (mode 0, 1, 2)
MEASURED = {
    "pts_linears_0.weight": (6.123e-07, 1.063e-05, 7.803e-07), "pts_linears_0.bias": (5.220e-07, 1.080e-05, 8.535e-07),
    "pts_linears_1.weight": (6.581e-07, 1.050e-05, 8.484e-07), "pts_linears_1.bias": (3.403e-07, 1.070e-05, 9.746e-07),
    "pts_linears_2.weight": (1.072e-06, 1.170e-05, 1.689e-06), "pts_linears_2.bias": (4.008e-07, 1.067e-05, 1.405e-06),
    "pts_linears_3.weight": (6.560e-07, 9.417e-06, 8.690e-07), "pts_linears_3.bias": (6.057e-07, 8.683e-06, 9.824e-07),
    "pts_linears_4.weight": (8.146e-07, 9.365e-06, 9.377e-07), "pts_linears_4.bias": (4.360e-07, 7.581e-06, 7.829e-07),
    "pts_linears_5.weight": (7.647e-07, 9.449e-06, 9.229e-07), "pts_linears_5.bias": (5.340e-07, 7.491e-06, 6.892e-07),
    "pts_linears_6.weight": (1.024e-06, 1.002e-05, 1.005e-06), "pts_linears_6.bias": (5.696e-07, 7.372e-06, 3.695e-07),
    "pts_linears_7.weight": (7.277e-07, 1.024e-05, 9.680e-07), "pts_linears_7.bias": (3.118e-07, 7.031e-07, 5.068e-07),
    "views_linears_0.weight": (1.228e-06, 1.146e-05, 8.274e-07), "views_linears_0.bias": (3.461e-07, 2.738e-07, 4.197e-07),
    "feature_linear.weight": (7.720e-07, 6.916e-06, 7.818e-07), "feature_linear.bias": (4.508e-07, 4.711e-06, 4.138e-07),
    "alpha_linear.weight": (1.335e-06, 1.354e-05, 8.999e-07), "alpha_linear.bias": (3.760e-07, 1.418e-07, 9.244e-08),
    "rgb_linear.weight": (4.517e-07, 9.043e-06, 4.942e-07), "rgb_linear.bias": (1.088e-07, 2.738e-07, 3.564e-07),
    "g_x": (4.123e-07, 1.632e-05, 5.898e-07),
}


def one_digit_up(v):
    """v rounded up to one significant digit"""
    from decimal import Decimal, ROUND_CEILING
    d = Decimal(repr(float(v)))
    return float(d.quantize(Decimal(1).scaleb(d.adjusted()), rounding=ROUND_CEILING)) if d > 0 else 0.0


def bar(mode, name):
    """the larger of 4 x the measured error rounded up to one significant digit and 4 x mode 0's own measured error for that tensor; never above the blob-wide bar"""
    e = MEASURED[name]
    return min(max(one_digit_up(4 * e[mode]), 4 * e[0]), CAPS[mode])


def test_backward_random_network_per_tensor(api):
    """The built shape with make_classic_scene's fill at 700 points, in modes 0, 1 and 2, against backward64: e(mode, t) = max |g - g64| / max |g64| for every parameter
    tensor t and for g_x, each printed.  Modes 1 and 2 are held per tensor to the larger of 4 x their measured error (rounded up to one digit) and 4 x mode 0's own --
    mode 0 is a legitimate fp32 chain -- and never to more than the blob-wide bars the project holds (3e-3 bf16x3, 3e-4 f16x3).  Mode 0 is held to the 2e-5 that
    test_classic_mlp_backward_vs_reference_autograd allows between the library and the oracle.
    The 700 points are kink_free_batch's: no pre-activation under a ReLU within 3e-4 of zero.  On the plain batch four pre-activations lie within 1e-6 of zero;
    mode 1 decides them the other way and the tensors below them move by whole terms -- up to 0.14 of pts_linears_3.weight's largest entry, far above the
    blob-wide bars, and reproduced to two digits in float64 by flipping those four masks (measured_errors.txt; mode 0 shows the same step, 1.6e-3, from layer 4
    down).  That says nothing about the products: on the batch that keeps clear of the kink mode 0 and mode 2 sit at 1e-6 and mode 1 at 1e-5 in every tensor."""
    shape, p = MN.BUILT, RANDOM_POINTS
    blob = random_network(shape, 7000)
    x, g = kink_free_batch(blob, shape, 5, p)
    want_p, want_x = MN.backward64(blob, x, g, shape)
    m = nerf(api, shape, blob)
    xd, gd = dev(x), dev(g)
    prev = api.lib.nrf_get_train_gemm()
    errs = {}
    try:
        for mode in (0, 1, 2):
            api.L.check(api.lib.nrf_set_train_gemm(mode))
            rc, got_p, got_x, guard = run_backward(api, m, shape, xd, gd, p, True, False)
            assert rc == NRF_OK and guard, (mode, rc, api.lib.nrf_last_error())
            assert np.isfinite(got_p).all() and np.isfinite(got_x[:p]).all() and np.isnan(got_x[p:]).all()
            for name, off, dims in MN.tensors(shape):
                n = int(np.prod(dims))
                errs[mode, name] = np.abs(got_p[off:off + n] - want_p[off:off + n]).max() / np.abs(want_p[off:off + n]).max()
            errs[mode, "g_x"] = np.abs(got_x[:p] - want_x).max() / np.abs(want_x).max()
    finally:
        api.L.check(api.lib.nrf_set_train_gemm(prev))
    names = [t[0] for t in MN.tensors(shape)] + ["g_x"]
    print("fp32 products: " + ("rocBLAS sgemm" if api.lib.nrf_fp32_gemm_available() else "mlp.hip's fp32 kernels"))
    for name in names:
        print("%-24s mode 0 %.3e   mode 1 %.3e   mode 2 %.3e" % (name, errs[0, name], errs[1, name], errs[2, name]))
    assert set(MEASURED) == set(names), "no measured table to take the bars from"
    for name in names:
        assert errs[0, name] <= 2e-5, (0, name, errs[0, name])
        for mode in (1, 2):
            assert errs[mode, name] <= bar(mode, name), (mode, name, errs[mode, name], bar(mode, name))
