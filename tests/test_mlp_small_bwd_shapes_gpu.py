"""GPU tests of the NeRFSmall training backward on exact integer networks: the fused fp16 kernel k_small_bwd<NL, NLC> (mlp_small_bwd_mfma.hip) in its three input
forms, and the fp32 chain mlp_small_backward (mlp.hip, through gemm_f32.hip / gemm_bf16x3.hip) that is the parity trainer's and serves every shape the fused kernel
refuses.  Cases and yardsticks are tests/mlp_small_ref.py's (integer_backward_case, backward64, model16), which tests/test_mlp_small_shapes_host.py pins on the CPU.
On those networks every arithmetic the library has gives the float64 gradient exactly, so every comparison below except (d) is EQUALITY, per parameter tensor.

Which test runs which kernel or branch (a shape is (views, NL, NLC, geo); modes are nrf_set_train_gemm's: 0 fp32 products, 1 bf16x3, 2 f16x3):
  k_small_bwd<2 | 3, 3 | 4>, rows form (nrf_mlp_backward_f16), with d_g_x and with d_g_x = NULL, nrf_mlp_backward_f16_flags == (0, 0) behind every call:
    one point; both sides of the 32-point wave tile (31, 32, 33) and of the 128-point workgroup block (127, 128, 129); 257;
    256 workgroups x 128 points + 1 = 32 769: workgroup 0 takes a second iteration of the persistent loop ......................... test_fused_rows_exact
    d_g_params prefilled (1 and 129 points), d_g_x rows behind the batch, a workspace of exactly the asked size + guard ......... test_fused_rows_exact
    the loss scale 2^(4 - e) at units 2^-40, 1 and 2^20; a workspace one byte short is refused and nothing is written .......... test_fused_rows_units_and_short_workspace
  k_small_bwd, level-major input (nrf_mlp_backward_f16_lm) and the column-map form the trainer calls (nrf_mlp_backward_f16_lm_src:
    a map that is not monotonic, shared and unread columns, pstride above the column count), a partial last ray; g_x bit-equal to
    the rows form's; s = 0, pstride = 0 and a misaligned direction buffer refused before any launch ............................. test_fused_level_major_forms_exact
  mlp_small_backward (nrf_mlp_backward), default mode, all 60 shapes -- ragged cat[views, geo] inputs of 16 | 64 + 0 / 1 / 7 / 14 / 15 columns; geo 0: an empty
    second segment, no k_copy_col launch for geo, a one-row last sigma layer:
    fewer than 256 points: mlp.hip's k_linear / k_grad_w / k_relu_mask (1, 255); 256 and 257: rocBLAS sgemm products + k_bias_relu
    where nrf_fp32_gemm_available() (else the same fp32 kernels) ................................................................. test_chain_exact_default_mode
  the same in modes 0, 1, 2 on ten shapes (the four fused, the three refused, (16, 2, 2, 0), (64, 2, 3, 1), (64, 3, 4, 14)):
    257 points, modes 1 and 2: gemm_nt_split forward products with the ReLU in the epilogue; k_backprop_thin through the last sigma layer (1 + geo outputs) and
      the rgb layer (3); the other back-propagations through gemm_nt_split; weight gradients still from rocBLAS / k_grad_w;
    4 097 points, modes 1 and 2: gemm_tn_thin for the 1 + geo and 3-row heads, gemm_tn_bf16x3 for the rest, colour layer 0 in two column segments;
    16 400 points, mode 0 with rocBLAS: the sliced strided-batched weight-gradient product, 32 slices of 512 and a remainder of 16 ... test_chain_exact_in_every_mode
  (d) random networks, two shapes, 700 kink-free rows: k_small_bwd against model16 at 4 x the distance between model16's float32 and float64
    accumulation, per tensor ................................................................................................. test_fused_random_network_against_model16
    the fp32 chain against backward64 per tensor: mode 0 at 2e-5, modes 1 and 2 at the project's 3e-3 and 3e-4 ................. test_chain_random_network_per_tensor
  The MI355X values of (d) are in profiles/mlp_small_bwd_shapes/measured_errors.txt.
Every GPU step runs once."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mlp_small_ref as MS
from test_mlp_nerf_shapes_gpu import equals64, GUARD, GUARD_BYTE, SCRATCH_BYTE

pytestmark = pytest.mark.gpu

NRF_OK = 0
host = lambda t: t.detach().cpu().numpy()
P = lambda t: None if t is None else t.data_ptr()
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from types import SimpleNamespace
    from nerfpp_amd import _lib as L, modules as M
    return SimpleNamespace(L=L, M=M, lib=L.lib())


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype, order="C")).cuda()          # (a copy: the cases are shared read-only arrays)


@functools.lru_cache(maxsize=32)
def case(shape, p, unit=MS.BWD_UNIT, s=None):
    return MS.integer_backward_case(shape, MS.BWD_SEED, p, unit, s)


def small(api, shape, blob):
    v, nl, nlc, g = shape
    return api.M.NeRFSmall(nl, MS.HIDDEN, g, nlc, MS.HIDDEN, False, 3, 64, MS.IN_CH, v, "model", params=blob)


def run_backward(api, m, shape, p, nbytes, call, with_gx, prefill_unit=None, ws_short=0):
    """One backward call -- call(d_g_params, d_g_x, d_workspace, workspace_bytes) -- on a workspace of exactly the asked size (less ws_short) of 0xFF bytes (all NaN:
    scratch read before it is written shows) with a guard behind it; d_g_params starts from prefill(n, prefill_unit) or from zero, d_g_x is NaN and three rows longer
    than the batch -> (status, g_params, g_x or None, guard intact, the workspace)"""
    n = MS.n_params(shape)
    nb = int(nbytes(m._m, p))
    assert nb > 0
    ws = torch.full((nb + GUARD,), SCRATCH_BYTE, dtype=torch.uint8, device="cuda")
    ws[nb:] = GUARD_BYTE
    gp = dev(MS.prefill(n, prefill_unit)) if prefill_unit is not None else torch.zeros(n, device="cuda")
    gx = torch.full((p + 3, MS.IN_CH), float("nan"), device="cuda") if with_gx else None
    rc = call(P(gp), P(gx), P(ws), nb - ws_short)
    torch.cuda.synchronize()
    return rc, host(gp), None if gx is None else host(gx), bool((ws[nb:] == GUARD_BYTE).all()), ws


def compare(shape, got_p, got_x, want_p, want_x, p, unit, prefilled, what):
    """per tensor and for rows < p of g_x: EQUAL; rows >= p of g_x stay NaN.  A prefilled blob ends at prefill + gradient; the prefill is asserted to be small integer
    multiples of the unit, which keeps every sum exact"""
    if prefilled:
        base = MS.prefill(got_p.size, unit).astype(np.float64)
        assert np.array_equal(base / unit, np.rint(base / unit)) and np.abs(base / unit).max() == 3
        assert np.abs(want_p / unit).max() + 3 < 2 ** 24 / MS.LOSS_SCALE, what
        want_p = want_p + base
    for name, off, (o, i) in MS.tensors(shape):
        equals64(got_p[off:off + o * i], want_p[off:off + o * i], f"{what} d / d {name}")
    if got_x is not None:
        assert np.isnan(got_x[p:]).all(), what + ": g_x rows past the batch were written"
        equals64(got_x[:p], want_x, what + " g_x")


def untouched(shape, got_p, got_x, guard, ws, unit, what):
    """a refused call wrote nothing: the prefill pattern, the NaN rows, the guard and the workspace are as they were"""
    assert guard, what + ": bytes behind the workspace were written"
    assert bool((ws[:ws.numel() - GUARD] == SCRATCH_BYTE).all()), what + ": the workspace was written"
    assert np.array_equal(bits(got_p), bits(MS.prefill(got_p.size, unit))), what + ": d_g_params was written"
    assert got_x is None or np.isnan(got_x).all(), what + ": d_g_x was written"


def flags_clean(api, ws, what):
    fl = (C.c_uint32 * 2)(7, 7)
    api.L.check(api.lib.nrf_mlp_backward_f16_flags(P(ws), fl, None))
    assert (fl[0], fl[1]) == (0, 0), (what, fl[0], fl[1])


def fused_rows(api, m, xd, gd, p):
    return lambda gp, gx, ws, nb: api.lib.nrf_mlp_backward_f16(m._m, P(xd), P(gd), p, gp, gx, ws, nb, None)


# ------------------------------------------------------------------ (a) fused kernel, rows form
@pytest.mark.parametrize("p", MS.FUSED_COUNTS)
@pytest.mark.parametrize("shape", MS.FUSED_SHAPES, ids=MS.shape_id)
def test_fused_rows_exact(api, shape, p):
    """nrf_mlp_backward_f16 on the integer networks, with d_g_x and with d_g_x = NULL: every parameter tensor and rows < p of g_x EQUAL backward64; rows >= p of g_x
    stay NaN; the flags read (0, 0).  At 1 and 129 points d_g_params starts from a pattern and ends at pattern + gradient.  A wrong fragment index, selector, mask,
    tail guard or blob offset, a dropped k-step or a weight gradient lost between the wave tiles, the LDS copy and the global blob shows at full size."""
    blob, x, g, (want_p, want_x) = case(shape, p)
    m = small(api, shape, blob)
    xd, gd = dev(x), dev(g)
    pre = MS.BWD_UNIT if p in MS.FUSED_PREFILLED else None
    for with_gx in (True, False):
        what = f"{MS.shape_id(shape)} fused rows p {p} {'with g_x' if with_gx else 'g_x NULL'}"
        rc, got_p, got_x, guard, ws = run_backward(api, m, shape, p, api.lib.nrf_mlp_backward_f16_workspace_bytes, fused_rows(api, m, xd, gd, p), with_gx, pre)
        assert rc == NRF_OK, (what, rc, api.lib.nrf_last_error())
        assert guard, what + ": bytes behind the workspace were written"
        flags_clean(api, ws, what)
        compare(shape, got_p, got_x, want_p, want_x, p, MS.BWD_UNIT, pre is not None, what)


@pytest.mark.parametrize("shape", MS.FUSED_SHAPES, ids=MS.shape_id)
def test_fused_rows_units_and_short_workspace(api, shape):
    """129 points with output gradients in units of 2^-40, 1 and 2^20: the loss scale 2^(4 - e) follows max |g_out| and, a power of two, leaves every result exact.
    A workspace one byte short is refused with a message before anything is launched: the prefilled d_g_params, the NaN d_g_x, the workspace and the guard behind
    it stay as they were."""
    p = MS.FUSED_UNITS_AT
    for unit in MS.FUSED_UNITS:
        blob, x, g, (want_p, want_x) = case(shape, p, unit)
        m = small(api, shape, blob)
        xd, gd = dev(x), dev(g)
        what = f"{MS.shape_id(shape)} fused rows p {p} unit {unit:g}"
        rc, got_p, got_x, guard, ws = run_backward(api, m, shape, p, api.lib.nrf_mlp_backward_f16_workspace_bytes, fused_rows(api, m, xd, gd, p), True, unit)
        assert rc == NRF_OK and guard, (what, rc, api.lib.nrf_last_error())
        flags_clean(api, ws, what)
        compare(shape, got_p, got_x, want_p, want_x, p, unit, True, what)
    blob, x, g, _ = case(shape, p)
    m = small(api, shape, blob)
    xd, gd = dev(x), dev(g)
    what = f"{MS.shape_id(shape)} fused rows p {p}, a workspace one byte short"
    rc, got_p, got_x, guard, ws = run_backward(api, m, shape, p, api.lib.nrf_mlp_backward_f16_workspace_bytes, fused_rows(api, m, xd, gd, p), True, MS.BWD_UNIT, ws_short=1)
    assert rc != NRF_OK and len(api.lib.nrf_last_error()) > 0, (what, rc)
    untouched(shape, got_p, got_x, guard, ws, MS.BWD_UNIT, what)


# ------------------------------------------------------------------ (b) fused kernel, the trainer's input forms
@pytest.mark.parametrize("p,s", MS.LM_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("shape", MS.FUSED_SHAPES, ids=MS.shape_id)
def test_fused_level_major_forms_exact(api, shape, p, s):
    """nrf_mlp_backward_f16_lm (features [16][p] half2, one fp16 view row per ray) and nrf_mlp_backward_f16_lm_src (a column table read through an int32 map that is
    not monotonic, with columns read by several points and by none and a stride above the column count; what no point reads holds 77) on a batch whose last ray is
    partial: every tensor and g_x EQUAL backward64 of the batch they encode, with d_g_x and with NULL, and g_x is the rows form's bit for bit.
    s = 0, pstride = 0 with a map and a direction buffer that is not 16-byte aligned are refused with a message before any launch: nothing is written."""
    blob, x, g, (want_p, want_x) = case(shape, p, MS.BWD_UNIT, s)
    assert p % s != 0
    m = small(api, shape, blob)
    nbytes = api.lib.nrf_mlp_backward_f16_workspace_bytes
    xd, gd = dev(x), dev(g)
    feats, dirs = dev(MS.pack_level_major(x), np.float16), dev(MS.pack_ray_views(x, s), np.float16)
    table_h, src_h, pstride = MS.pack_column_table(x, MS.BWD_SEED)
    table, src = dev(table_h, np.float16), dev(src_h, np.int32)
    assert feats.shape == (16, p, 2) and table.shape == (16, pstride, 2) and dirs.data_ptr() % 16 == 0
    forms = {
        "rows": fused_rows(api, m, xd, gd, p),
        "lm": lambda gp, gx, ws, nb: api.lib.nrf_mlp_backward_f16_lm(m._m, P(feats), P(dirs), s, P(gd), p, gp, gx, ws, nb, None),
        "lm_src": lambda gp, gx, ws, nb: api.lib.nrf_mlp_backward_f16_lm_src(m._m, P(table), pstride, P(src), P(dirs), s, P(gd), p, gp, gx, ws, nb, None),
    }
    gx_of = {}
    for name, call in forms.items():
        for with_gx in ((True,) if name == "rows" else (True, False)):
            what = f"{MS.shape_id(shape)} fused {name} p {p} s {s} {'with g_x' if with_gx else 'g_x NULL'}"
            rc, got_p, got_x, guard, ws = run_backward(api, m, shape, p, nbytes, call, with_gx, None if with_gx else MS.BWD_UNIT)
            assert rc == NRF_OK, (what, rc, api.lib.nrf_last_error())
            assert guard, what + ": bytes behind the workspace were written"
            flags_clean(api, ws, what)
            compare(shape, got_p, got_x, want_p, want_x, p, MS.BWD_UNIT, not with_gx, what)
            if with_gx:
                gx_of[name] = got_x[:p]
    for name in ("lm", "lm_src"):
        assert np.array_equal(bits(gx_of[name]), bits(gx_of["rows"])), f"{MS.shape_id(shape)} p {p} s {s}: g_x of {name} is not the rows form's bit for bit"
    # bad arguments
    rays = dirs.shape[0]
    odd = torch.zeros(rays * 16 + 8, dtype=torch.float16, device="cuda")
    shifted = odd[1:1 + rays * 16]
    shifted.copy_(dirs.reshape(-1))
    assert shifted.data_ptr() % 16 == 2
    refused = {
        "lm, s = 0": lambda gp, gx, ws, nb: api.lib.nrf_mlp_backward_f16_lm(m._m, P(feats), P(dirs), 0, P(gd), p, gp, gx, ws, nb, None),
        "lm_src, s = 0": lambda gp, gx, ws, nb: api.lib.nrf_mlp_backward_f16_lm_src(m._m, P(table), pstride, P(src), P(dirs), 0, P(gd), p, gp, gx, ws, nb, None),
        "lm_src, pstride = 0": lambda gp, gx, ws, nb: api.lib.nrf_mlp_backward_f16_lm_src(m._m, P(table), 0, P(src), P(dirs), s, P(gd), p, gp, gx, ws, nb, None),
        "lm, directions off by 2 bytes": lambda gp, gx, ws, nb: api.lib.nrf_mlp_backward_f16_lm(m._m, P(feats), P(shifted), s, P(gd), p, gp, gx, ws, nb, None),
        "lm_src, directions off by 2 bytes": lambda gp, gx, ws, nb: api.lib.nrf_mlp_backward_f16_lm_src(m._m, P(table), pstride, P(src), P(shifted), s, P(gd), p, gp, gx, ws, nb, None),
    }
    for name, call in refused.items():
        what = f"{MS.shape_id(shape)} p {p} s {s}: {name}"
        rc, got_p, got_x, guard, ws = run_backward(api, m, shape, p, nbytes, call, True, MS.BWD_UNIT)
        assert rc != NRF_OK and len(api.lib.nrf_last_error()) > 0, (what, rc)
        untouched(shape, got_p, got_x, guard, ws, MS.BWD_UNIT, what)


# ------------------------------------------------------------------ (c) fp32 chain
def chain(api, m, xd, gd, p):
    return lambda gp, gx, ws, nb: api.lib.nrf_mlp_backward(m._m, P(xd), P(gd), p, gp, gx, ws, nb, None)


def chain_exact(api, m, shape, p, prefilled, tag):
    blob, x, g, (want_p, want_x) = case(shape, p)
    xd, gd = dev(x), dev(g)
    for with_gx in (True, False):
        what = f"{MS.shape_id(shape)} fp32 chain {tag} p {p} {'with g_x' if with_gx else 'g_x NULL'}"
        rc, got_p, got_x, guard, _ = run_backward(api, m, shape, p, api.lib.nrf_mlp_backward_workspace_bytes, chain(api, m, xd, gd, p), with_gx, MS.BWD_UNIT if prefilled else None)
        assert rc == NRF_OK, (what, rc, api.lib.nrf_last_error())
        assert guard, what + ": bytes behind the workspace were written"
        compare(shape, got_p, got_x, want_p, want_x, p, MS.BWD_UNIT, prefilled, what)


def fp32_products(api):
    return "rocBLAS sgemm" if api.lib.nrf_fp32_gemm_available() else "mlp.hip's fp32 kernels"


@pytest.mark.parametrize("shape", MS.SHAPES, ids=MS.shape_id)
def test_chain_exact_default_mode(api, shape):
    """nrf_mlp_backward in the mode the library starts in (NeRFSmall: fp32 products) on all 60 shapes at 1, 255, 256 and 257 points, with d_g_x and with NULL: every
    parameter tensor and g_x EQUAL backward64; d_g_params starts from a pattern at 1 and 257 points; the workspace is exactly nrf_mlp_backward_workspace_bytes
    with an untouched guard behind it.  geo 0 has an empty second input segment in colour layer 0 and a one-row last sigma layer."""
    m = small(api, shape, case(shape, 1)[0])
    for p in MS.CHAIN_COUNTS:
        chain_exact(api, m, shape, p, p in (1, 257), "default mode")
    print(f"{MS.shape_id(shape)}: exact at {MS.CHAIN_COUNTS} points in mode {api.lib.nrf_get_train_gemm()}; the fp32 products at 256 points and more are {fp32_products(api)}")


@pytest.mark.parametrize("mode", (0, 1, 2), ids=lambda mode: "mode%d" % mode)
@pytest.mark.parametrize("shape", MS.CHAIN_MODE_SHAPES, ids=MS.shape_id)
def test_chain_exact_in_every_mode(api, shape, mode):
    """nrf_set_train_gemm(0 | 1 | 2) applies to NeRFSmall too: at 257 points (the split forward and back-propagation products, k_backprop_thin through the 1 + geo and
    3-row heads) and at 4 097 (gemm_tn_thin for those heads, gemm_tn_bf16x3 for the other weight gradients, colour layer 0 in two column segments) every tensor and
    g_x EQUAL backward64; in mode 0 also at 16 400 points where the fp32 products are rocBLAS's: 32 slices of 512 points and a remainder of 16.  The previous mode is
    restored."""
    prev = api.lib.nrf_get_train_gemm()
    m = small(api, shape, case(shape, 1)[0])
    counts = list(MS.CHAIN_MODE_COUNTS)
    if mode == 0 and api.lib.nrf_fp32_gemm_available():
        counts.append(MS.CHAIN_SLICED_COUNT)
    try:
        api.L.check(api.lib.nrf_set_train_gemm(mode))
        assert api.lib.nrf_get_train_gemm() == mode
        for p in counts:
            chain_exact(api, m, shape, p, p == 4097, f"mode {mode}")
    finally:
        api.L.check(api.lib.nrf_set_train_gemm(prev))
    print(f"{MS.shape_id(shape)} mode {mode}: exact at {tuple(counts)} points; the fp32 products are {fp32_products(api) if mode == 0 else 'not used'}")


# ------------------------------------------------------------------ (d) random networks
FP32_BAR, SPLIT_BARS = 2e-5, {1: 3e-3, 2: 3e-4}          # test_training_backward_stages_vs_reference_autograd's / test_classic_and_lerf_train_steps_in_the_split_gemm_modes_follow_the_fp32_chain's


@functools.lru_cache(maxsize=2)
def random_case(shape):
    blob, x, g = MS.random_backward_case(shape)
    return blob, x, g, MS.backward64(blob, x, g, shape)


@pytest.mark.parametrize("shape", MS.RANDOM_SHAPES, ids=MS.shape_id)
def test_fused_random_network_against_model16(api, shape):
    """The fused kernel on random_network(shape, 7000, 30.0) at 700 kink-free rows against model16, its own arithmetic restated with float64 accumulation: per tensor
    and for g_x, e = max |got - model16| / max |model16| <= 4 x e32, where e32 is the same distance between model16 with float32 and with float64 accumulation,
    computed here from the two references alone.  The kernel's only freedom against the model is its fp32 summation order (e32 is rare one-ulp fp16 double roundings
    of sums that differ in the last fp32 bit); the factor 4 covers an order neither model has.  A wrong rounding or a dropped k-step in one fragment is orders
    above that.  Printed for information: the distance to backward64, percents -- ReLU flips of the fp16 forward, why float64 is no yardstick here."""
    blob, x, g, (ref_p, ref_x) = random_case(shape)
    p = x.shape[0]
    p64, x64, _ = MS.model16(blob, x, g, shape, np.float64)
    p32, x32, _ = MS.model16(blob, x, g, shape, np.float32)
    e32 = MS.tensor_errors(p32, x32, p64, x64, shape)
    m = small(api, shape, blob)
    rc, got_p, got_x, guard, ws = run_backward(api, m, shape, p, api.lib.nrf_mlp_backward_f16_workspace_bytes, fused_rows(api, m, dev(x), dev(g), p), True)
    assert rc == NRF_OK and guard, (rc, api.lib.nrf_last_error())
    flags_clean(api, ws, MS.shape_id(shape))
    assert np.isfinite(got_p).all() and np.isfinite(got_x[:p]).all() and np.isnan(got_x[p:]).all()
    e = MS.tensor_errors(got_p, got_x[:p], p64, x64, shape)
    far = MS.tensor_errors(got_p, got_x[:p], ref_p, ref_x, shape)
    for name in e:
        print("%s fused %-12s e %.3e   e32 %.3e   bar %.3e   to backward64 %.3e" % (MS.shape_id(shape), name, e[name], e32[name], 4 * e32[name], far[name]))
    for name in e:
        assert e32[name] > 0 and e[name] <= 4 * e32[name], (name, e[name], e32[name])


@pytest.mark.parametrize("shape", MS.RANDOM_SHAPES, ids=MS.shape_id)
def test_chain_random_network_per_tensor(api, shape):
    """The fp32 chain on the same networks and rows against backward64, per tensor and for g_x: mode 0 within the 2e-5 the project allows its fp32 chains, modes 1
    and 2 within its 3e-3 (bf16x3) and 3e-4 (f16x3).  The rows keep clear of the ReLU kink in float64 as well (random_backward_case), so no mask is decided by the
    arithmetic."""
    blob, x, g, (ref_p, ref_x) = random_case(shape)
    p = x.shape[0]
    m = small(api, shape, blob)
    xd, gd = dev(x), dev(g)
    prev = api.lib.nrf_get_train_gemm()
    errs = {}
    try:
        for mode in (0, 1, 2):
            api.L.check(api.lib.nrf_set_train_gemm(mode))
            rc, got_p, got_x, guard, _ = run_backward(api, m, shape, p, api.lib.nrf_mlp_backward_workspace_bytes, chain(api, m, xd, gd, p), True)
            assert rc == NRF_OK and guard, (mode, rc, api.lib.nrf_last_error())
            assert np.isfinite(got_p).all() and np.isfinite(got_x[:p]).all() and np.isnan(got_x[p:]).all()
            errs[mode] = MS.tensor_errors(got_p, got_x[:p], ref_p, ref_x, shape)
    finally:
        api.L.check(api.lib.nrf_set_train_gemm(prev))
    print("fp32 products: " + fp32_products(api))
    for name in errs[0]:
        print("%s chain %-12s mode 0 %.3e   mode 1 %.3e   mode 2 %.3e" % (MS.shape_id(shape), name, errs[0][name], errs[1][name], errs[2][name]))
    for name in errs[0]:
        assert errs[0][name] <= FP32_BAR, (0, name, errs[0][name])
        for mode in (1, 2):
            assert errs[mode][name] <= SPLIT_BARS[mode], (mode, name, errs[mode][name])
