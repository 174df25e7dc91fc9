"""GPU tests of the four small kernels that close every training step (nerfpp_amd/csrc/train.hip), each against the plain numpy model of tests/train_tail_ref.py, which
tests/test_train_tail_host.py holds to the C oracle and to the reference's goldens on the CPU.  The comparisons are exact (bit patterns) wherever the kernel is
elementwise, and bounded by a derived rounding budget where it accumulates with atomics.

Which test runs which kernel path:
  k_huber + k_finish_loss, one block and less (count 1 .. 257), the capped 512-block grid with a second grid-stride trip
    (131 071 .. 131 073) and a ragged fourth (393 221), with and without d_grad ................. test_huber_loss_every_count
  ... the double accumulator cleared per call (two calls queued back to back) ................... test_huber_two_calls_back_to_back
  ... NaN / +inf inputs, the count = 0 refusal .................................................. test_huber_nan_inf_and_refusal
  k_mask_grad, src = NULL (nrf_mask_sigma_grad): p 1 .. 1000 x c 1, 4, 7 x five keep patterns ..... test_mask_sigma_grad_touches_only_masked_sigma_words
  k_mask_grad, src != NULL (nrf_mask_sigma_grad_src): keep by column, shorter and longer than p .. test_mask_sigma_grad_src_reads_the_mask_by_column
  k_tv_loss<1>, <2>, <4>, <8>: every F x log2_t 4, 10, 14 x cube 1, 5, 6, 7, 16 at one min_vertex, plus the other min_vertex (the one whose uint32 products wrap
    included), weights, levels, a repeated-row table and a random prefill of d_g_table per F; each case once with d_g_table and once with NULL ... test_tv_loss_every_case
    No F is left out: nrf_hash_create accepts 1, 2, 4, 8 in NGP mode.  It refuses every other width (asserted for 3), so nrf_hash_tv_loss's NRF_ERR_UNSUPPORTED
    answer cannot be reached through the API and is not tested.
  ... refusals (cube 0 and 512, level = n_levels, a CuHashEmbedder-mode grid) ................... test_tv_loss_refusals
  k_adam, n_flags = 0 (nrf_adam_step): n 1 .. 65 537 x t 1 .. 200 000 x betas x eps x lr .......... test_adam_step_bit_for_bit
  ... t = 1 then t = 2 from zero moments ........................................................ test_adam_two_consecutive_steps
  k_adam, n_flags = 1, 2, 16 (nrf_adam_step_guarded): all clear, every single position set ...... test_adam_guarded_every_flag_position
  ... n = 0 and the refusals .................................................................... test_adam_empty_and_refusals
  Trainer.add_tv_loss (tv_cuboids -> one k_tv_loss<2> per level) ................................ test_trainer_add_tv_loss_equals_the_model_on_its_cuboids,
                                                                                                 test_trainer_add_tv_loss_is_off_without_a_weight_or_on_a_cu_grid
Adam's inputs are exactly zero or far from the subnormals (|g| >= 1e-12: the smallest intermediate, g^2 (1 - beta2), is 1e-27; the host file checks every intermediate
of every case), so the comparison does not depend on how either side treats subnormal numbers.  Every GPU step runs once."""
import ctypes as C

import numpy as np
import pytest
import torch

import train_tail_ref as TT
from train_tail_ref import bits, f32

pytestmark = pytest.mark.gpu

NRF_OK, NRF_ERR_INVALID_ARG = 0, 1          # include/nerfpp_hip.h
host = lambda t: t.detach().cpu().numpy()
P = lambda t: None if t is None else t.data_ptr()
SENTINEL = np.array([0x7FC0BEEF], np.uint32).view(f32)[0]          # a NaN with a payload: a word that is written shows


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from types import SimpleNamespace
    from nerfpp_amd import _lib as L, modules as M, scene as S
    return SimpleNamespace(L=L, M=M, S=S, lib=L.lib())


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def same_bits(got, want, what):
    g, w = bits(got).reshape(-1), bits(want).reshape(-1)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.nonzero(g != w)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} words differ, first at {bad[:5]}: {np.asarray(got).reshape(-1)[bad[:3]]!r} vs {np.asarray(want).reshape(-1)[bad[:3]]!r}"


def sentinels(n):
    return np.full(n, SENTINEL, f32)


# ------------------------------------------------------------------ nrf_huber_loss
def loss_words_ok(got2, loss64, mse64, what):
    """the kernel's double partial sums differ from the exact sum by ~count * 2^-53 relative, far below half a float32 ulp: the float result is the correctly rounded
    value or its neighbour"""
    for name, got, want in (("loss", got2[0], loss64), ("mse", got2[1], mse64)):
        d = abs(int(bits(f32(got))[0]) - int(bits(f32(want))[0]))
        print(f"{what} {name}: got {float(got)!r}, model {want!r}, {d} ulp apart")
        assert np.isfinite(got) and got > 0 and d <= 1, (what, name, float(got), want)


def run_huber(api, pred, target, with_grad=True, pad=3):
    n = pred.size
    pd, td = dev(pred), dev(target)
    lm = dev(sentinels(2)); g = dev(sentinels(n + pad)) if with_grad else None
    api.L.check(api.lib.nrf_huber_loss(P(pd), P(td), n, P(lm), P(g), None))
    torch.cuda.synchronize()
    return host(lm), (host(g) if with_grad else None)


@pytest.mark.parametrize("count", TT.HUBER_COUNTS)
def test_huber_loss_every_count(api, count):
    """gradient bit for bit (the planted |d| = 1 neighbours, +0 and -0.0 included; nothing past `count` written), both loss words within one float32 ulp of the float64
    model -- with d_grad and with d_grad = NULL"""
    pred, target = TT.huber_case(count)
    loss64, mse64, grad = TT.huber(pred, target)
    lm, g = run_huber(api, pred, target)
    same_bits(g[:count], grad, f"d huber / d pred, count {count}")
    same_bits(g[count:], sentinels(3), "words past the gradient")
    loss_words_ok(lm, loss64, mse64, f"count {count}")
    lm2, _ = run_huber(api, pred, target, with_grad=False)
    loss_words_ok(lm2, loss64, mse64, f"count {count}, d_grad = NULL")


def test_huber_two_calls_back_to_back(api):
    """two calls queued on one stream with different inputs, no wait between them: each is right (the scratch accumulator is cleared per call)"""
    cases = [TT.huber_case(131073, seed=1), TT.huber_case(257, seed=2), TT.huber_case(131073, seed=3)]
    bufs = []
    for pred, target in cases:
        pd, td, lm, g = dev(pred), dev(target), dev(sentinels(2)), dev(sentinels(pred.size))
        api.L.check(api.lib.nrf_huber_loss(P(pd), P(td), pred.size, P(lm), P(g), None))
        bufs.append((pd, td, lm, g))
    torch.cuda.synchronize()
    for i, ((pred, target), (_, _, lm, g)) in enumerate(zip(cases, bufs)):
        loss64, mse64, grad = TT.huber(pred, target)
        same_bits(host(g), grad, f"call {i}: gradient")
        loss_words_ok(host(lm), loss64, mse64, f"call {i}")


def test_huber_nan_inf_and_refusal(api):
    count = 257
    norm = f32(1) / f32(count)
    pred, target = TT.huber_case(count)
    _, _, clean = TT.huber(pred, target)
    pred[-1] = np.nan
    lm, g = run_huber(api, pred, target)
    assert np.isnan(lm[0]) and np.isnan(lm[1]) and np.isnan(g[count - 1]), (lm, g[count - 1])
    same_bits(g[:count - 1], clean[:count - 1], "NaN in the last element: every other gradient element")
    pred, target = TT.huber_case(count)
    pred[100] = np.inf
    lm, g = run_huber(api, pred, target)
    assert lm[0] == np.inf and lm[1] == np.inf, lm
    want = clean.copy(); want[100] = norm
    same_bits(g[:count], want, "+inf in pred: that element is exactly norm, the others unchanged")
    # count = 0
    pd, td, lmd, gd = dev(pred), dev(target), dev(sentinels(2)), dev(sentinels(count))
    rc = api.lib.nrf_huber_loss(P(pd), P(td), 0, P(lmd), P(gd), None)
    torch.cuda.synchronize()
    assert rc == NRF_ERR_INVALID_ARG, rc
    same_bits(host(lmd), sentinels(2), "count = 0: loss words"); same_bits(host(gd), sentinels(count), "count = 0: gradient")


# ------------------------------------------------------------------ nrf_mask_sigma_grad(_src)
@pytest.mark.parametrize("p", TT.MASK_P)
def test_mask_sigma_grad_touches_only_masked_sigma_words(api, p):
    """column c - 1 holds +0.0 bits exactly where keep is 0 (true stored as 1, 2 or 255 alike); every other word of the buffer -- NaN payloads, -0.0, the row behind the
    last -- keeps its bits"""
    for c in TT.MASK_C:
        g = TT.mask_grad_buffer(p + 1, c)          # one row more than the call is told about
        for name in TT.MASK_KEEPS:
            keep = TT.mask_keep(name, p)
            want = g.copy(); want[:p] = TT.mask_sigma(g[:p], keep, c)
            gd, kd = dev(g), dev(keep, np.uint8)
            api.L.check(api.lib.nrf_mask_sigma_grad(P(kd), p, c, P(gd), None))
            torch.cuda.synchronize()
            same_bits(host(gd), want, f"p {p} c {c} keep {name}")


@pytest.mark.parametrize("p", TT.MASK_P)
def test_mask_sigma_grad_src_reads_the_mask_by_column(api, p):
    """the keep array is by COLUMN, of a length other than p; point i is masked by keep[src[i]] (repeats, column 0, the last column)"""
    for m in TT.mask_src_lengths(p):
        keep_cols, src = TT.mask_src_case(p, m)
        assert src.min() >= 0 and src.max() < m
        for c in TT.MASK_C:
            g = TT.mask_grad_buffer(p + 1, c)
            want = g.copy(); want[:p] = TT.mask_sigma(g[:p], keep_cols, c, src=src)
            gd, kd, sd = dev(g), dev(keep_cols, np.uint8), dev(src, np.int32)
            api.L.check(api.lib.nrf_mask_sigma_grad_src(P(kd), P(sd), p, c, P(gd), None))
            torch.cuda.synchronize()
            same_bits(host(gd), want, f"p {p} m {m} c {c}")


# ------------------------------------------------------------------ nrf_hash_tv_loss
_embedders = {}


def tv_embedder(api, F, T, cu=False):
    key = (F, T, cu)
    if key not in _embedders:
        _embedders[key] = (api.M.CuHashEmbedder if cu else api.M.HashEmbedder)("embedder", api.S.LEGO_BBOX, TT.TV_LEVELS, F, T, 16, 64)
    return _embedders[key]


def tv_call(api, e, td, level, mv, cube, weight, loss, gd):
    mv = np.ascontiguousarray(mv, np.int32)
    return api.lib.nrf_hash_tv_loss(e._h, P(td), level, mv.ctypes.data_as(C.c_void_p), cube, weight, P(loss), P(gd), None)


def other_levels_sentinel(c):
    """[3, 2^T, F] distinct words; the case's own level is filled in by the caller"""
    n = TT.TV_LEVELS * (1 << c["T"]) * c["F"]
    return (np.uint32(0x40000000) + np.arange(n, dtype=np.uint32)).view(f32).reshape(TT.TV_LEVELS, 1 << c["T"], c["F"]).copy()


@pytest.mark.parametrize("case", TT.TV_CASES, ids=TT.tv_case_id)
def test_tv_loss_every_case(api, case):
    """d_loss ends at prefill + weight * loss within (W + 2) 2^-24 loss (W waves: each partial rounded once, then one float atomic each; plus one ulp of the sum where the
    running sum starts at 2.5); every entry of the level's slice of d_g_table within (k + 1) 2^-23 A of prefill + the float64 scatter of the model's float32 addends
    (k addends, A their absolute sum, a non-zero prefill one more), entries no addend reaches keep the prefill's bits; the other levels' slices keep theirs (the
    level * 2^T * F offset).  With d_g_table = NULL the loss is the same."""
    c = case
    e = tv_embedder(api, c["F"], c["T"])
    table = TT.tv_table(c)
    ex = TT.tv_expect(c, table)
    g0 = other_levels_sentinel(c); g0[c["level"]] = ex["prefill"]
    td, gd, loss = dev(table), dev(g0), dev([c["loss_prefill"]])
    api.L.check(tv_call(api, e, td, c["level"], c["mv"], c["cube"], c["weight"], loss, gd))
    loss_null = dev([0.0])
    api.L.check(tv_call(api, e, td, c["level"], c["mv"], c["cube"], c["weight"], loss_null, None))
    torch.cuda.synchronize()
    got = host(gd).reshape(g0.shape)
    for l in range(TT.TV_LEVELS):
        if l != c["level"]:
            same_bits(got[l], g0[l], f"level {l}'s slice (the call is for level {c['level']})")
    mine = got[c["level"]]
    k = ex["model"]["k"]
    same_bits(mine[k == 0], ex["prefill"][k == 0], "entries no addend reaches")
    err = np.abs(mine.astype(np.float64) - ex["want_grad"])
    worst = float((err / np.maximum(ex["grad_budget"], 1e-300))[k > 0].max())
    got_loss, got_null = float(host(loss)[0]), float(host(loss_null)[0])
    print(f"{TT.tv_case_id(c)}: loss {got_loss!r} vs {ex['want_loss']!r} (budget {ex['loss_budget']:.3e}), NULL-gradient loss {got_null!r} vs {ex['weighted_loss']!r}, "
          f"worst gradient error / budget {worst:.3f}, most addends on an entry {int(k.max())}")
    assert np.isfinite(mine).all() and (err <= ex["grad_budget"]).all(), (worst, int(np.argmax(err - ex["grad_budget"])))
    assert abs(got_loss - ex["want_loss"]) <= ex["loss_budget"], (got_loss, ex["want_loss"], ex["loss_budget"])
    assert abs(got_null - ex["weighted_loss"]) <= TT.tv_loss_budget(ex["model"]["W"], ex["weighted_loss"]), (got_null, ex["weighted_loss"])


def test_tv_loss_refusals(api):
    """cube 0, cube 512, level = n_levels, a CuHashEmbedder-mode grid: NRF_ERR_INVALID_ARG, nothing written.  A width of 3 features cannot be created at all."""
    c = next(c for c in TT.TV_CASES if c["F"] == 2 and c["T"] == 10)
    F, T = c["F"], c["T"]
    table = TT.tv_table(c)
    g0 = other_levels_sentinel(c)
    td = dev(table)
    ngp, cu = tv_embedder(api, F, T), tv_embedder(api, F, T, cu=True)
    for what, e, level, cube in (("cube 0", ngp, 1, 0), ("cube 512", ngp, 1, 512), ("level = n_levels", ngp, TT.TV_LEVELS, 5), ("cu-mode grid", cu, 1, 5)):
        gd, loss = dev(g0), dev(sentinels(1))
        rc = tv_call(api, e, td, level, (3, 1, 2), cube, 1.0, loss, gd)
        torch.cuda.synchronize()
        assert rc == NRF_ERR_INVALID_ARG and b"nrf_hash_tv_loss" in api.lib.nrf_last_error(), (what, rc)
        same_bits(host(gd), g0, f"{what}: d_g_table"); same_bits(host(loss), sentinels(1), f"{what}: d_loss")
    desc = api.L.HashDesc(api.L.NRF_HASH_NGP, TT.TV_LEVELS, 3, 10, 16, 64, (C.c_float * 6)(*np.asarray(api.S.LEGO_BBOX, np.float32).reshape(6).tolist()))
    h = C.c_void_p()
    assert api.lib.nrf_hash_create(C.byref(desc), C.byref(h)) == NRF_ERR_INVALID_ARG and not h.value


# ------------------------------------------------------------------ nrf_adam_step(_guarded)
def run_adam(api, state, case, t=None, flags=None, n_flags=None, pad=2):
    """one call on fresh device copies of (p, g, m, v), each with `pad` sentinel words behind it -> (rc, p, m, v) as they are afterwards"""
    p, g, m, v = state
    n = p.size
    dp, dg, dm, dv = (dev(np.concatenate([a, sentinels(pad)])) for a in (p, g, m, v))
    t = case["t"] if t is None else t
    if flags is None and n_flags is None:
        rc = api.lib.nrf_adam_step(P(dp), P(dg), P(dm), P(dv), n, case["lr"], case["b1"], case["b2"], case["eps"], t, None)
    else:
        df = None if flags is None else dev(np.asarray(flags, np.uint32).view(np.int32), np.int32)
        rc = api.lib.nrf_adam_step_guarded(P(dp), P(dg), P(dm), P(dv), n, case["lr"], case["b1"], case["b2"], case["eps"], t, P(df), len(flags) if n_flags is None else n_flags, None)
    torch.cuda.synchronize()
    out = [host(a) for a in (dp, dm, dv)]
    for a in out:
        same_bits(a[n:], sentinels(pad), "words past the array")
    return (rc,) + tuple(a[:n] for a in out)


@pytest.mark.parametrize("n", TT.ADAM_N)
def test_adam_step_bit_for_bit(api, n):
    """p, m and v equal the model's bits at every t, beta, eps and lr: every operation of the kernel is one correctly rounded IEEE float32 operation (the library is built
    with -ffp-contract=off and no fast-math flag), in the model's order, with the bias corrections formed in double on the host"""
    for case in (c for c in TT.ADAM_CASES if c["n"] == n):
        state = TT.adam_state(case)
        p1, m1, v1 = TT.adam(*state, case["lr"], case["b1"], case["b2"], case["eps"], case["t"])
        rc, gp, gm, gv = run_adam(api, state, case)
        assert rc == NRF_OK, (case, rc)
        same_bits(gm, m1, f"m {case}"); same_bits(gv, v1, f"v {case}"); same_bits(gp, p1, f"p {case}")


def test_adam_two_consecutive_steps(api):
    """t = 1 then t = 2 from zero moments on the same device buffers, without a wait between: the model applied twice"""
    case = dict(n=257, lr=5e-4, b1=0.9, b2=0.99, eps=1e-15)
    p, g1, _, _ = TT.adam_state(dict(case, t=1), seed=1)
    _, g2, _, _ = TT.adam_state(dict(case, t=2), seed=2)
    z = np.zeros_like(p)
    dp, dm, dv, dg1, dg2 = dev(p), dev(z), dev(z), dev(g1), dev(g2)
    for t, dg in ((1, dg1), (2, dg2)):
        api.L.check(api.lib.nrf_adam_step(P(dp), P(dg), P(dm), P(dv), p.size, case["lr"], case["b1"], case["b2"], case["eps"], t, None))
    torch.cuda.synchronize()
    pa, ma, va = TT.adam(p, g1, z, z, case["lr"], case["b1"], case["b2"], case["eps"], 1)
    pb, mb, vb = TT.adam(pa, g2, ma, va, case["lr"], case["b1"], case["b2"], case["eps"], 2)
    same_bits(host(dm), mb, "m after two steps"); same_bits(host(dv), vb, "v after two steps"); same_bits(host(dp), pb, "p after two steps")


@pytest.mark.parametrize("n_flags", (1, 2, 16))
def test_adam_guarded_every_flag_position(api, n_flags):
    """all words zero: the unguarded call's bits; any single word set, to 1 or to 0x80000000, at any position: p, m and v keep their bits (257 elements: two blocks)"""
    case = dict(n=257, t=10, lr=1e-2, b1=0.9, b2=0.999, eps=1e-8)
    state = TT.adam_state(case, seed=n_flags)
    p, g, m, v = state
    p1, m1, v1 = TT.adam(*state, case["lr"], case["b1"], case["b2"], case["eps"], case["t"], flags=[0] * n_flags)
    rc, gp, gm, gv = run_adam(api, state, case, flags=[0] * n_flags)
    assert rc == NRF_OK
    same_bits(gm, m1, "flags clear: m"); same_bits(gv, v1, "flags clear: v"); same_bits(gp, p1, "flags clear: p")
    _, up, um, uv = run_adam(api, state, case)
    same_bits(gp, up, "flags clear == unguarded: p"); same_bits(gm, um, "flags clear == unguarded: m"); same_bits(gv, uv, "flags clear == unguarded: v")
    assert (bits(p1) != bits(p)).any()
    for pos in range(n_flags):
        for word in (1, 0x80000000):
            flags = [0] * n_flags; flags[pos] = word
            rc, gp, gm, gv = run_adam(api, state, case, flags=flags)
            assert rc == NRF_OK
            same_bits(gp, p, f"flag {pos} = {word:#x}: p"); same_bits(gm, m, f"flag {pos} = {word:#x}: m"); same_bits(gv, v, f"flag {pos} = {word:#x}: v")


def test_adam_empty_and_refusals(api):
    """n = 0 is NRF_OK and touches nothing; n_flags = 17, n_flags = 2 without flags, t = 0 and n = -1 are NRF_ERR_INVALID_ARG with the buffers untouched"""
    case = dict(n=257, t=3, lr=1e-2, b1=0.9, b2=0.99, eps=1e-8)
    state = TT.adam_state(case)
    p, g, m, v = state
    dp, dg, dm, dv = (dev(a) for a in state)
    rc = api.lib.nrf_adam_step(P(dp), P(dg), P(dm), P(dv), 0, case["lr"], case["b1"], case["b2"], case["eps"], 3, None)
    torch.cuda.synchronize()
    assert rc == NRF_OK
    same_bits(host(dp), p, "n = 0: p"); same_bits(host(dm), m, "n = 0: m"); same_bits(host(dv), v, "n = 0: v")
    rc = api.lib.nrf_adam_step(P(dp), P(dg), P(dm), P(dv), -1, case["lr"], case["b1"], case["b2"], case["eps"], 3, None)
    torch.cuda.synchronize()
    assert rc == NRF_ERR_INVALID_ARG
    same_bits(host(dp), p, "n = -1: p"); same_bits(host(dm), m, "n = -1: m"); same_bits(host(dv), v, "n = -1: v")
    for what, kw in (("n_flags = 17", dict(flags=[0] * 17)), ("n_flags = 2 with NULL flags", dict(n_flags=2)), ("t = 0", dict(t=0))):
        rc, gp, gm, gv = run_adam(api, state, case, **kw)
        assert rc == NRF_ERR_INVALID_ARG, (what, rc)
        same_bits(gp, p, f"{what}: p"); same_bits(gm, m, f"{what}: m"); same_bits(gv, v, f"{what}: v")


# ------------------------------------------------------------------ Trainer.add_tv_loss
def test_trainer_add_tv_loss_equals_the_model_on_its_cuboids(api):
    """a 4-level HashEmbedder scene (2^10 rows, weight 0.37), g_table zeroed, step count 3: g_table is the sum over the levels of the model's gradients for
    tv_cuboids(...) at that step count, entry by entry within the per-entry budgets (each level has its own slice), and tv_loss the sum of the weighted level losses within
    the sum of their budgets"""
    from nerfpp_amd.train import Trainer, tv_cuboids
    L, T, F, base, finest, seed, t, w = 4, 10, 2, 16, 128, 11, 3, 0.37
    sc = api.S.make_hash_scene(mode="ngp", n_levels=L, n_feat=F, log2_t=T, base=base, finest=finest, seed=321)
    table = np.asarray(sc["table"], np.float32).reshape(L, 1 << T, F)
    with Trainer(sc["embedder"], sc["embeddirs"], sc["mlp"], sc["table"], sc["mlp_blob"], tv_loss_weight=w, seed=seed) as tr:
        tr.t = t
        tr.g_table.zero_()
        tr.add_tv_loss()
        torch.cuda.synchronize()
        got, got_loss = host(tr.g_table).reshape(L, 1 << T, F), float(host(tr.tv_loss)[0])
    want_loss = budget = 0.0
    cub = tv_cuboids(base, finest, L, seed, t)
    assert [c[0] for c in cub] == list(range(L))
    for level, res, cube, mv in cub:
        m = TT.tv(table[level], T, mv, cube, w)
        err = np.abs(got[level].astype(np.float64) - m["grad"])
        assert (err <= TT.tv_grad_budget(m["k"], m["A"])).all(), (level, float(err.max()))
        assert (got[level][m["k"] == 0] == 0).all() and (m["k"] > 0).any()
        wl = float(f32(w)) * m["loss"]
        want_loss += wl; budget += TT.tv_loss_budget(m["W"], wl)
    print(f"tv_loss {got_loss!r} vs {want_loss!r}, budget {budget:.3e}; cuboids {cub}")
    assert want_loss > 0 and abs(got_loss - want_loss) <= budget, (got_loss, want_loss, budget)


@pytest.mark.parametrize("mode,weight", [("ngp", 0.0), ("cu", 0.37)])
def test_trainer_add_tv_loss_is_off_without_a_weight_or_on_a_cu_grid(api, mode, weight):
    """tv_loss_weight = 0, or a CuHashEmbedder scene (the reference defines the regulariser for the LibTorch HashEmbedder only): g_table and tv_loss keep their bits"""
    from nerfpp_amd.train import Trainer
    sc = api.S.make_hash_scene(mode=mode, log2_t=14, seed=322) if mode == "cu" else api.S.make_hash_scene(mode=mode, n_levels=4, log2_t=10, base=16, finest=128, seed=322)
    with Trainer(sc["embedder"], sc["embeddirs"], sc["mlp"], sc["table"], sc["mlp_blob"], tv_loss_weight=weight, seed=11) as tr:
        g0 = (np.uint32(0x40000000) + np.arange(tr.g_table.numel(), dtype=np.uint32)).view(f32)
        tr.g_table.copy_(dev(g0)); tr.tv_loss.copy_(dev(sentinels(1)))
        tr.add_tv_loss()
        torch.cuda.synchronize()
        same_bits(host(tr.g_table), g0, "g_table"); same_bits(host(tr.tv_loss), sentinels(1), "tv_loss")
