"""GPU tests of the hash grid's table gradient (nerfpp_amd/csrc/train.hip): nrf_hash_backward, nrf_hash_backward_rays, nrf_hash_backward_rays_packed and
nrf_hash_backward_rays_binned against tests/hash_backward_ref.py, which tests/test_hash_backward_host.py checks on the CPU.  Every comparison is of WHOLE gradient tables
(kilobytes to 12 MB), accumulated into a non-zero base table.
  float paths        |got - (base + R)| <= gamma(k + 1) (|base| + A) per element: R, A, k the exact sum, the sum of magnitudes and the count of the element's addends; the bound
                     of an fp32 sum in any order, so it covers the atomics and the walk's pre-summation alike.  No measured constant.
  fixed-point paths  equality of BITS with fixed_point_model(), of the table and of every pass's unit read from the workspace; and the exact sum within the model's rounding
                     budget, as a statement of what the bits are worth.

Which run executes which instantiation (B.FLOAT_RUNS, B.FIXED_RUNS; every grid at n = 701 rays of s = 37 samples unless noted):
  k_hash_ngp_bwd<2>, k_hash_bwd_ray<2, false> ............ ngp-4-64 (all ray shapes), ngp-2-30, ngp-box, ngp-16-2048 at (7, 17)
  k_hash_cu_bwd<1>, k_hash_bwd_ray<1, true> .............. lmf-L2-F1 (all ray shapes), lmf-L5-F1-bias-box
  k_hash_cu_bwd<2>, k_hash_bwd_ray<2, true> .............. cu-L16 (all ray shapes; one sample, subnormal, dominating gradients), cu-L8 .. cu-L32, -bias, -box, -T4, -T5,
                                                           -scales-integers, -scales-64bit, lmf-L7-F2
  k_hash_cu_bwd<4>, <8>, k_hash_bwd_ray_fl<4, true>, <8, true>  lmf-L3-F4, lmf-L16-F8 (all ray shapes: last wavefronts with 4 .. 60 live lanes; groups whose row is all zero)
  k_hash_bwd_ray<4, true>, <8, true> ...................... test_thread_per_segment_walk_at_4_and_8_features (a child process with NRF_HASH_BWD_FEATURE_LANES=0)
  k_hash_bwd_ray<2, CU, true, 0> + k_unpack_q ............ packed, every FIXED_RUNS entry
  k_hash_bwd_ray<2, CU, true, 1>, <.., 2>, k_bin_scan, k_bin_accumulate  binned, every FIXED_RUNS entry, with the worst-case and the batch-sized workspace
  k_level_mass with L < 16 ............................... cu-L8, lmf-L7-F2, cu-L3-T19, ngp-L2-T19;  L = 16: the L16 grids;  L > 16 (a second level per thread): cu-L32
  k_level_mass's outside-box factor ...................... every ngp run (rays from outside, hash_shapes_ref's outside points), ngp-outside-pile
  k_bin_accumulate with one bin .......................... cu-L16-T4, -T5, cu-L8 (tables below 2^14 words);  many bins: cu-L3-T19 (64), ngp-L2-T19 (64), the T = 10 grids (2)
  a level that starts off a bin edge ..................... cu-L16-T4 (8 words per level step), -T5
  two passes (k_level_mass over grid.y, two units) ....... (1400, 192) on cu-L16 and ngp-4-64; the side list of the LAST pass on ngp-4-64 dominating
  the side list .......................................... the dominating runs, and (1, 1): a lone sample's addends are ~2^29 units
NOT run: more passes than the 64-KB header holds (pass_cap = 65536 / (8 L + 8), ~480 passes of 2^18 points: minutes, not seconds); n_features = 3 and log2_hashmap_size < 4
or > 24, which nrf_hash_create refuses before any backward could.
Every GPU step runs once."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hash_backward_paths as G
import hash_backward_ref as B
import hash_shapes_ref as HS
from hash_backward_paths import P, dev, host

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
BIN_HDR = 65536                   # the binned workspace's header; the side list's counter lies right behind it
PACKED_QS = 768                   # PackedHead: double mass[64], 256 bytes of padding, float qs[64]


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from types import SimpleNamespace
    from nerfpp_amd import _lib as L, modules as M
    handles = {}

    def handle(case):
        if case.name not in handles:
            handles[case.name] = G.make_handle(M, case)
        return handles[case.name]
    return SimpleNamespace(L=L, M=M, lib=L.lib(), handle=handle)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def assert_bits(got, want, what):
    bad = np.nonzero(bits(got) != bits(want))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} elements differ, first {bad[0]}: {got[bad[0]]!r} vs {want[bad[0]]!r}"


def packed(api, e, i, n, s, ws=None):
    """-> (table, unit of the LAST pass, workspace)"""
    nb = api.lib.nrf_hash_backward_packed_workspace_bytes(e._h)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda") if ws is None else ws
    gt, dp, dg = dev(i.base), dev(i.pts), dev(i.g)
    api.L.check(api.lib.nrf_hash_backward_rays_packed(e._h, P(dp), n, s, P(dg), P(gt), P(ws), nb, None))
    torch.cuda.synchronize()
    return host(gt), host(ws[PACKED_QS:PACKED_QS + 8]).view(f32)[1], ws


def binned(api, e, i, n, s, nb, ws=None):
    """-> (table, units of all passes, entries of the last pass's side list, workspace)"""
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda") if ws is None else ws
    gt, dp, dg = dev(i.base), dev(i.pts), dev(i.g)
    api.L.check(api.lib.nrf_hash_backward_rays_binned(e._h, P(dp), n, s, P(dg), P(gt), P(ws), nb, None))
    torch.cuda.synchronize()
    L = e.NLevels
    qs = (BIN_HDR // (L * 8 + 8)) * L * 8          # the scales follow the masses of pass_cap passes
    passes = -(-n // max(1, B.GROUP_PTS // s))
    units = host(ws[qs:qs + 8 * passes]).view(f32)[1::2]
    return host(gt), units, int(host(ws[BIN_HDR:BIN_HDR + 4]).view(np.uint32)[0]), ws


# ------------------------------------------------------------------ float paths
@pytest.mark.parametrize("run", B.FLOAT_RUNS, ids=B.run_id)
def test_float_paths_vs_exact_sum(api, run):
    """nrf_hash_backward and nrf_hash_backward_rays, into a non-zero table, against base + R under gamma(k + 1) (|base| + A).  (Found with it: k_hash_cu_bwd, and the
    thread-per-segment walk at 4 and 8 features, rounded g * w to fp16 ONCE where the reference rounds the fp32 product -- 8 elements of cu-L16-box beyond the bound, each by
    one fp16 ulp of one addend; see cu_addend_f16 in train.hip.)"""
    name, n, s, pattern = run
    case = B.BY_NAME[name]
    i, ex = B.inputs(name, n, s, pattern), B.expected_exact(name, n, s, pattern)
    tol = G.float_tolerance(i, ex)
    e = api.handle(case)
    for path in ("points", "rays"):
        G.check_against_exact(G.run_float(api.L, e, path, i, n, s), i, ex, tol, f"{B.run_id(run)} {path}")


def test_thread_per_segment_walk_at_4_and_8_features(api):
    """k_hash_bwd_ray<4>, <8>: the walk LeRF's grid took before the lane-per-feature kernel, still selectable (NRF_HASH_BWD_FEATURE_LANES=0, read once per process): one fresh
    child process, lmf-L3-F4 and lmf-L16-F8 under the float paths' bound"""
    helper = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "hash_backward_walk_child.py")
    out = subprocess.run([sys.executable, helper], env=dict(os.environ, NRF_HASH_BWD_FEATURE_LANES="0"), capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.returncode, out.stdout[-2000:], out.stderr[-4000:])


# ------------------------------------------------------------------ fixed-point paths
def check_fixed(api, case, i, n, s, m, ex, what, side_list=False):
    e = api.handle(case)
    tol = B.fixed_point_tolerance(m, i.base, ex)
    got, unit, ws = packed(api, e, i, n, s)
    assert bits(unit) == bits(m.units[-1]), f"{what}: packed unit {unit!r}, model {m.units[-1]!r}"
    assert_bits(got, m.table, what + " packed")
    got2, unit2, _ = packed(api, e, i, n, s, ws)
    assert_bits(got2, m.table, what + " packed, second call on the same workspace")
    G.check_against_exact(got, i, ex, tol, what + " packed")
    nbb = api.lib.nrf_hash_backward_binned_workspace_bytes(e._h, s)
    nbf = api.lib.nrf_hash_backward_binned_workspace_bytes_for(e._h, n, s)
    assert 0 < nbf <= nbb
    got, units, side, ws = binned(api, e, i, n, s, nbb)
    assert np.array_equal(bits(units), bits(m.units)), f"{what}: binned units {units!r}, model {m.units!r}"
    assert_bits(got, m.table, what + " binned")
    print(f"{what}: units {m.units}, side list of the last pass {side} (model {sum(m.side[-1])}), largest field total {m.max_total / 2.0 ** 31:.4f} * 2^31")
    assert side == sum(m.side[-1]), f"{what}: {side} entries in the last pass's side list, model {sum(m.side[-1])}"
    if side_list:
        assert side > 0
    got2, units2, side2, _ = binned(api, e, i, n, s, nbb, ws)
    assert_bits(got2, m.table, what + " binned, second call on the same workspace")
    assert side2 == side and np.array_equal(bits(units2), bits(m.units))
    got3, units3, side3, _ = binned(api, e, i, n, s, nbf)
    assert_bits(got3, m.table, what + " binned, batch-sized workspace")
    assert side3 == side and np.array_equal(bits(units3), bits(m.units))


@pytest.mark.parametrize("run", B.FIXED_RUNS, ids=B.run_id)
def test_fixed_point_paths_equal_the_model(api, run):
    """nrf_hash_backward_rays_packed and nrf_hash_backward_rays_binned: the table and every pass's unit equal fixed_point_model()'s BIT FOR BIT; a second call on the same
    workspace gives the same bits (word table, bin counts and side list were left clean); the binned form with the worst-case and with the batch-sized workspace; the side
    list's count behind the header equals the model's for the last pass; and the table is within f unit / 2 + gamma(16) A + 2^-23 (|base| + A + f unit / 2) of the exact sum,
    with the MODEL's unit and flush count f."""
    name, n, s, pattern = run
    case = B.BY_NAME[name]
    i, ex, m = B.inputs(name, n, s, pattern), B.expected_exact(name, n, s, pattern), B.expected_model(name, n, s, pattern)
    check_fixed(api, case, i, n, s, m, ex, B.run_id(run), side_list=run in B.SIDE_RUNS)


def test_ngp_outside_pile(api):
    """The input of test_outside_box_bound_of_the_level_mass's search that comes closest to 2^31 units among those the library accepts (T = 4, the pile four finest cells
    below the box on three axes: 0.81 * 2^31 in the field of entry 0): packed and binned against the model's bits and against base + R."""
    T, side, ecells = B.PILE_WORST_BUILDABLE
    case, pts, g = B.pile_outside(T, side, ecells)
    n, s = 8, 16
    i = B.Inputs(pts, np.zeros(n, np.int64), g, B.base_table(case))
    m, ex = B.fixed_point_model(case, pts, n, s, g, i.base), B.exact(case, pts, g)
    assert 0.8 < m.max_total / 2.0 ** 31 < 1.0
    check_fixed(api, case, i, n, s, m, ex, case.name)


@pytest.mark.parametrize("name", ["cu-L16", "ngp-4-64"])
def test_all_zero_gradient_changes_nothing(api, name):
    """all four entry points on a gradient of zeros (-0.0 among them): status OK and the table's bits unchanged; the unit of an empty pass is 1 (k = 0)"""
    case = B.BY_NAME[name]
    n, s = B.MAIN
    i = B.inputs(name, n, s, "zero")
    g = np.array(i.g)
    g[1::3] = f32(-0.0)
    i = i._replace(g=g)
    e = api.handle(case)
    for path in ("points", "rays"):
        assert_bits(G.run_float(api.L, e, path, i, n, s), i.base, f"{name} {path}, zero gradient")
    got, unit, _ = packed(api, e, i, n, s)
    assert_bits(got, i.base, name + " packed, zero gradient")
    assert unit == 1.0
    got, units, side, _ = binned(api, e, i, n, s, api.lib.nrf_hash_backward_binned_workspace_bytes_for(e._h, n, s))
    assert_bits(got, i.base, name + " binned, zero gradient")
    assert units.tolist() == [1.0] and side == 0


# ------------------------------------------------------------------ refusals
def test_refusals_leave_the_table_untouched(api):
    """NRF_ERR_UNSUPPORTED: packed and binned at F != 2, binned at T = 20 (n_features = 3 is refused by nrf_hash_create, so no backward ever sees it).  NRF_ERR_INVALID_ARG: a
    workspace pointer offset by 8 bytes, a table pointer offset by 4.  NRF_ERR_WORKSPACE: a workspace one byte short.  n = 0: OK, nothing written.  In every case the table
    keeps its bits."""
    lib, L = api.lib, api.L
    UNSUPPORTED, INVALID, WORKSPACE = 3, 1, 4
    n, s = 5, 16
    with pytest.raises(L.NrfError):
        api.M.CuHashEmbedder("f3", HS.LEGO_BBOX, 4, 3, 10, 4, 64)
    with pytest.raises(L.NrfError):
        api.M.HashEmbedder("t3", HS.LEGO_BBOX, 4, 2, 3, 4, 64)

    def attempt(case, e, call, want, table_off=0):
        i = B.inputs(case.name, n, s) if case.name in B.BY_NAME else None
        pts, g, base = (i.pts, i.g, i.base) if i else (B.ray_points(case, n, s)[0], B.grads(case, n, s, np.zeros(n, np.int64)), B.base_table(case))
        gt, dp, dg = dev(np.concatenate([base, base[:2]])), dev(pts), dev(g)
        status = call(e, P(dp), P(dg), P(gt) + table_off)
        torch.cuda.synchronize()
        assert status == want, (case.name, status, want, L.lib().nrf_last_error().decode())
        assert_bits(host(gt)[:base.size], base, case.name + ": a refused or empty call wrote to the table")

    f4 = B.BY_NAME["lmf-L3-F4"]
    e4 = api.handle(f4)
    ws = torch.zeros(1 << 26, dtype=torch.uint8, device="cuda")
    attempt(f4, e4, lambda e, p, g, t: lib.nrf_hash_backward_rays_packed(e._h, p, n, s, g, t, P(ws), ws.numel(), None), UNSUPPORTED)
    attempt(f4, e4, lambda e, p, g, t: lib.nrf_hash_backward_rays_binned(e._h, p, n, s, g, t, P(ws), ws.numel(), None), UNSUPPORTED)
    t20 = HS.Case("cu-L2-T20", "cu", 2, 2, 20, 16, 64, np.asarray(HS.LEGO_BBOX, f32), None, None, HS.ALL, "one past the binned form's largest level")
    attempt(t20, G.make_handle(api.M, t20), lambda e, p, g, t: lib.nrf_hash_backward_rays_binned(e._h, p, n, s, g, t, P(ws), ws.numel(), None), UNSUPPORTED)
    for name in ("cu-L16", "ngp-4-64"):
        case = B.BY_NAME[name]
        e = api.handle(case)
        nbp = lib.nrf_hash_backward_packed_workspace_bytes(e._h)
        nbb = lib.nrf_hash_backward_binned_workspace_bytes_for(e._h, n, s)
        assert max(nbp, nbb) + 256 <= ws.numel() and P(ws) % 256 == 0
        pk = lambda e, p, g, t, w=P(ws), nb=nbp: lib.nrf_hash_backward_rays_packed(e._h, p, n, s, g, t, w, nb, None)
        bn = lambda e, p, g, t, w=P(ws), nb=nbb: lib.nrf_hash_backward_rays_binned(e._h, p, n, s, g, t, w, nb, None)
        attempt(case, e, lambda e, p, g, t: pk(e, p, g, t, w=P(ws) + 8), INVALID)
        attempt(case, e, lambda e, p, g, t: bn(e, p, g, t, w=P(ws) + 8), INVALID)
        attempt(case, e, pk, INVALID, table_off=4)
        attempt(case, e, bn, INVALID, table_off=4)
        attempt(case, e, lambda e, p, g, t: pk(e, p, g, t, nb=nbp - 1), WORKSPACE)
        attempt(case, e, lambda e, p, g, t: bn(e, p, g, t, nb=nbb - 1), WORKSPACE)
        attempt(case, e, lambda e, p, g, t: lib.nrf_hash_backward(e._h, p, 0, g, t, None), L.NRF_OK)
        attempt(case, e, lambda e, p, g, t: lib.nrf_hash_backward_rays(e._h, p, 0, s, g, t, None), L.NRF_OK)
        attempt(case, e, lambda e, p, g, t: lib.nrf_hash_backward_rays_packed(e._h, p, 0, s, g, t, P(ws), nbp, None), L.NRF_OK)
        attempt(case, e, lambda e, p, g, t: lib.nrf_hash_backward_rays_binned(e._h, p, 0, s, g, t, P(ws), lib.nrf_hash_backward_binned_workspace_bytes_for(e._h, 0, s), None), L.NRF_OK)
