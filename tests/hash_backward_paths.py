"""What tests/test_hash_backward_gpu.py and its child process (tests/helpers/hash_backward_walk_child.py) share: handles on the cases of hash_backward_ref.py, one call of each
float backward entry point, and the comparison against the exact sum."""
import numpy as np
import torch

import hash_backward_ref as B
import hash_shapes_ref as HS

f64 = np.float64
host = lambda t: t.detach().cpu().numpy()
P = lambda t: t.data_ptr()


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()          # (a copy: the shared inputs are read-only)


def make_handle(M, case):
    """a handle on the case's grid with nothing baked (the backward reads no table): level scales, biases, box and primes are the case's"""
    if case.mode == "cu":
        e = M.CuHashEmbedder("embedder", case.bbox, case.L, case.F, case.T, case.base, case.finest)
        if case.scales is not None:
            e.set_level_scales(case.scales)
        e.set_dense_budget(0)
        e.set_primes(HS.primes_of(case), case.biases)
    else:
        e = M.HashEmbedder("embedder", case.bbox, case.L, case.F, case.T, case.base, case.finest)
        e.set_dense_budget(0)
    assert np.array_equal(e.level_scales().view(np.uint32), HS.level_scales(case).view(np.uint32)), case.name + ": the handle's level scales are the case's"
    assert e.table_elems() == B.table_elems(case)
    return e


def run_float(L, e, path, i, n, s):
    """nrf_hash_backward ('points') or nrf_hash_backward_rays ('rays') into a copy of the base table -> the table"""
    gt, dp, dg = dev(i.base), dev(i.pts), dev(i.g)
    if path == "points":
        L.check(L.lib().nrf_hash_backward(e._h, P(dp), n * s, P(dg), P(gt), None))
    else:
        L.check(L.lib().nrf_hash_backward_rays(e._h, P(dp), n, s, P(dg), P(gt), None))
    torch.cuda.synchronize()
    return host(gt)


def float_tolerance(i, ex):
    """|fl(base + sum of k addends, any order and any grouping) - (base + R)| <= gamma(k + 1) * (|base| + A), fp32"""
    return B.gamma(ex.k + 1) * (np.abs(i.base.astype(f64)) + ex.A)


def check_against_exact(got, i, ex, tol, what):
    """every element within tol of base + R; untouched elements keep the base's bits.  Prints the worst ratio before it asserts."""
    want = i.base.astype(f64) + ex.R
    err = np.abs(got.astype(f64) - want)
    ratio = float((err / np.maximum(tol, 1e-300))[ex.k > 0].max()) if (ex.k > 0).any() else 0.0
    print(f"{what}: {int((ex.k > 0).sum())} of {got.size} elements touched, worst |got - exact| / tolerance {ratio:.3f}, largest error {err.max():.3e}")
    same = ex.k == 0
    assert np.array_equal(got[same].view(np.uint32), i.base[same].view(np.uint32)), what + ": an element no addend reaches changed"
    bad = np.nonzero(err > tol)[0]
    assert bad.size == 0, f"{what}: {bad.size} elements beyond the bound, first {bad[0]}: got {got[bad[0]]!r}, exact {want[bad[0]]!r}, tolerance {tol[bad[0]]:.3e} (k = {ex.k[bad[0]]})"
    assert np.isfinite(got).all()
