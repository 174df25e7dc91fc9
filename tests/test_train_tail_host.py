"""CPU tests of the models in tests/train_tail_ref.py (huber, sigma mask, TV, Adam) against what the project already trusts -- the C oracle and the reference's goldens --
so that tests/test_train_tail_gpu.py's comparison of the kernels with those models rests on something; of the shared case lists (they hold the edges they claim to hold);
and of nerfpp_amd.train.tv_cuboids, the per-level cuboid arithmetic of Trainer.add_tv_loss."""
import inspect

import numpy as np
import pytest

from conftest import load_golden
from nerfpp_amd import synth
from oracle import capi as O
import train_tail_ref as TT
from train_tail_ref import bits, f32


def ulps_apart(a, b):
    """distance in float32 steps between two finite, same-sign float32 numbers"""
    return abs(int(bits(f32(a))[0]) - int(bits(f32(b))[0]))


def same_bits(got, want, what):
    g, w = bits(got).reshape(-1), bits(want).reshape(-1)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.nonzero(g != w)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} words differ, first at {bad[:5]}"


# ------------------------------------------------------------------ huber
@pytest.mark.parametrize("count", TT.HUBER_COUNTS)
def test_huber_model_equals_oracle(count):
    """gradient bit for bit; loss and mse within one float32 ulp (the oracle sums sequentially in double, the model with math.fsum)"""
    pred, target = TT.huber_case(count)
    loss64, mse64, grad = TT.huber(pred, target)
    ol, om, og = O.huber_loss(pred, target)
    same_bits(grad, og, f"d huber / d pred, count {count}")
    print(f"count {count}: loss {ol!r} vs {loss64!r}, mse {om!r} vs {mse64!r}")
    assert ulps_apart(loss64, ol) <= 1 and ulps_apart(mse64, om) <= 1, (count, loss64, ol, mse64, om)


def test_huber_model_equals_oracle_on_nan_and_inf():
    pred, target = TT.huber_case(257)
    pred[-1] = np.nan
    loss64, mse64, grad = TT.huber(pred, target)
    ol, om, og = O.huber_loss(pred, target)
    assert np.isnan(loss64) and np.isnan(mse64) and np.isnan(ol) and np.isnan(om) and np.isnan(grad[-1]) and np.isnan(og[-1])
    same_bits(grad[:-1], og[:-1], "NaN: the other gradient elements")
    pred, target = TT.huber_case(257)
    pred[100] = np.inf
    loss64, mse64, grad = TT.huber(pred, target)
    ol, om, og = O.huber_loss(pred, target)
    assert loss64 == np.inf and ol == np.inf and mse64 == np.inf and om == np.inf and grad[100] == f32(1) / f32(257)
    same_bits(grad, og, "+inf: gradient")


def test_huber_cases_hold_every_branch_boundary():
    """each of the eight planted differences sits on the very last element at some count, d is exact there, and every count of 64 or more holds all eight"""
    last = set()
    for count in TT.HUBER_COUNTS:
        pred, target = TT.huber_case(count)
        d = pred - target
        last.add(int(bits(d[-1:])[0]))
        if count >= 64:
            assert {int(b) for b in bits(np.array(TT.HUBER_PLANTS, f32))} <= {int(b) for b in bits(d)}, count
    assert last == {int(b) for b in bits(np.array(TT.HUBER_PLANTS, f32))}
    assert len({int(b) for b in bits(np.array(TT.HUBER_PLANTS, f32))}) == 8


# ------------------------------------------------------------------ sigma mask
def test_mask_model_and_cases():
    """the model zeroes exactly the masked sigma words; the buffers hold distinct words with NaN and -0.0 around the sigma column; the _src cases read by column"""
    for p in TT.MASK_P:
        for c in TT.MASK_C:
            g = TT.mask_grad_buffer(p, c)
            if p * c > 8:
                assert len(set(bits(g).reshape(-1).tolist())) > p * c * 0.55 and np.isnan(g[:, c - 1]).any() and (bits(g[:, c - 1]) == 0x80000000).any()
            for name in TT.MASK_KEEPS:
                k = TT.mask_keep(name, p)
                out = TT.mask_sigma(g, k, c)
                changed = bits(out) != bits(g)
                assert not changed[:, :c - 1].any() and (bits(out[k == 0, c - 1]) == 0).all() and not changed[k != 0].any(), (p, c, name)
        for m in TT.mask_src_lengths(p):
            keep_cols, src = TT.mask_src_case(p, m)
            assert src.dtype == np.int32 and (p == 1 or src.min() == 0)
            assert src.max() == m - 1 and len(keep_cols) == m != p
            if p >= 255:
                assert len(set(src.tolist())) < p and (keep_cols[src] != 0).any() and (keep_cols[src] == 0).any()
                assert ((keep_cols[src] == 0) != (np.resize(keep_cols, p) == 0)).any(), "reading the mask by POINT would not give the same answer"


# ------------------------------------------------------------------ TV
@pytest.mark.parametrize("case", TT.TV_CASES, ids=TT.tv_case_id)
def test_tv_model_equals_oracle(case):
    """the tensor formulation against the oracle's per-vertex loop (sequential float32 accumulation of the same addends), within the budgets the GPU test uses"""
    table = TT.tv_table(case)
    m = TT.tv(table[case["level"]], case["T"], case["mv"], case["cube"], case["weight"])
    ol, og = O.tv_loss(table[case["level"]], case["T"], case["mv"], case["cube"], weight=case["weight"])
    assert abs(ol - m["loss"]) <= TT.tv_loss_budget(m["W"], m["loss"]), (ol, m["loss"])
    err = np.abs(og.astype(np.float64) - m["grad"])
    assert (err <= TT.tv_grad_budget(m["k"], m["A"])).all(), (err.max(), np.abs(m["grad"]).max())
    assert (og[m["k"] == 0] == 0).all() and m["k"].sum() == 2 * 3 * case["cube"] * (case["cube"] + 1) ** 2 * case["F"]
    assert m["W"] == -(-(case["cube"] + 1) ** 3 // 64)
    if case["loss_prefill"]:
        # the running float32 sum then starts at the prefill: W roundings of <= 2^-24 (prefill + loss) each stay inside the loss budget plus one ulp of the sum
        # when W prefill <= 2 loss + prefill
        assert float(f32(case["weight"])) * m["loss"] >= case["loss_prefill"] * (m["W"] - 1) / 2, (m["loss"], m["W"])
    if case["T"] == 4 and case["cube"] >= 5:
        assert m["k"].min() >= 3 * case["cube"] and (m["A"] > 0).all(), "16 rows: every entry takes many addends"


def test_tv_cases_cover_every_axis_value():
    C = TT.TV_CASES
    assert {c["F"] for c in C} == {1, 2, 4, 8} and {c["T"] for c in C} == {4, 10, 14} and {c["cube"] for c in C} == {1, 5, 6, 7, 16}
    assert {c["mv"] for c in C} == {(0, 0, 0), (3, 1, 2), TT.TV_BIG} and {c["weight"] for c in C} == {1.0, 0.37, 1e-6} and {c["level"] for c in C} == {0, 1, 2}
    product = {(c["F"], c["T"], c["cube"]) for c in C if c["mv"] == (3, 1, 2) and c["weight"] == 1.0 and c["level"] == 1 and c["table"] == "normal"}
    assert len(product) == 60
    assert {c["F"] for c in C if c["g_prefill"] == "random"} == {1, 2, 4, 8} and {c["loss_prefill"] for c in C} == {0.0, 2.5}
    assert any(c["table"] == "repeated" for c in C)
    # the big min_vertex makes the 32-bit products wrap
    assert TT.TV_BIG[1] * 2654435761 >= 1 << 32 and TT.TV_BIG[2] * 805459861 >= 1 << 32
    # 16 rows: the 4913 vertices pile onto every row.  Lattice NEIGHBOURS never share a row, whatever the table size: a step along an axis changes one hash term by an odd
    # number (1 or an odd prime), so its lowest bit flips -- u == v pairs cannot arise in this hash, and the model and the kernel need no case for them
    c4 = next(c for c in C if c["T"] == 4 and c["cube"] == 16)
    n = 17
    ax = [c4["mv"][a] + np.arange(n, dtype=np.int64) for a in range(3)]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    rows = (X ^ (Y * 2654435761) ^ (Z * 805459861)) & 15
    assert np.bincount(rows.reshape(-1), minlength=16).min() > 200
    assert not ((rows[1:] == rows[:-1]).any() or (rows[:, 1:] == rows[:, :-1]).any() or (rows[:, :, 1:] == rows[:, :, :-1]).any())
    rep = TT.tv_table(next(c for c in C if c["table"] == "repeated"))
    assert (rep[:, 1:] == rep[:, :-1]).all(-1).mean() > 0.4


def test_tv_model_equals_reference_golden(manifest):
    """... and the reference's own autograd at levels 0, 3, 5 of the tv_loss golden, within the same budgets"""
    g = load_golden("tv_loss")
    ent = manifest["tv_loss"]
    for level in (0, 3, 5):
        table = synth.blob_from_manifest([ent[level]]).reshape(1 << 14, 2)
        m = TT.tv(table, 14, g[f"l{level}_min_vertex"], int(g[f"l{level}_res_cube"][1]), 1.0)
        ref_loss, ref_grad = float(g[f"l{level}_loss"][0]), g[f"l{level}_grad"].astype(np.float64)
        err = np.abs(ref_grad - m["grad"])
        print(f"level {level}: loss {ref_loss!r} vs {m['loss']!r} (budget {TT.tv_loss_budget(m['W'], m['loss']):.3e}), worst gradient error / budget "
              f"{(err / np.maximum(TT.tv_grad_budget(m['k'], m['A']), 1e-300)).max():.3f}")
        assert abs(ref_loss - m["loss"]) <= TT.tv_loss_budget(m["W"], m["loss"])
        assert (err <= TT.tv_grad_budget(m["k"], m["A"])).all()
        assert (ref_grad[m["k"] == 0] == 0).all()


# ------------------------------------------------------------------ Adam
@pytest.mark.parametrize("n", TT.ADAM_N)
def test_adam_model_equals_oracle(n):
    """bit for bit on every case, planted rows included; no intermediate of any case is subnormal"""
    for case in (c for c in TT.ADAM_CASES if c["n"] == n):
        p, g, m, v = TT.adam_state(case)
        trace = []
        p1, m1, v1 = TT.adam(p, g, m, v, case["lr"], case["b1"], case["b2"], case["eps"], case["t"], trace=trace)
        po, mo, vo = p.copy(), m.copy(), v.copy()
        O.adam_step(po, g, mo, vo, case["lr"], case["t"], b1=case["b1"], b2=case["b2"], eps=case["eps"])
        same_bits(m1, mo, f"m {case}"); same_bits(v1, vo, f"v {case}"); same_bits(p1, po, f"p {case}")
        assert not any(TT.is_subnormal(a).any() for a in trace + [p, g, m, v]), case
        assert all(np.isfinite(a).all() for a in trace), case
        if n >= 6:
            assert p1[0] == p[0] and p1[-1] == p[-1] and m1[0] == 0 and v1[0] == 0, "g = m = v = 0: the parameter does not move"
            assert g[1] == 0 and m[1] != 0 and v[1] != 0 and v[2] == 0 and g[2] != 0
    assert TT.adam(p, g, m, v, 1e-2, 0.9, 0.99, 1e-8, 3, flags=[0, 0])[0].tobytes() == TT.adam(p, g, m, v, 1e-2, 0.9, 0.99, 1e-8, 3)[0].tobytes()
    for a, b in zip(TT.adam(p, g, m, v, 1e-2, 0.9, 0.99, 1e-8, 3, flags=[0, 0x80000000]), (p, m, v)):
        same_bits(a, b, "a set flag returns the inputs")


def test_adam_model_reproduces_the_reference_step(manifest):
    """the golden's step-1 parameters from its step-1 gradients, at test_adam_two_steps_vs_reference's bar (atol 2e-7)"""
    g = load_golden("train_hash")
    ent = manifest["train_hash"]
    names = ["sigma_net_0", "sigma_net_1", "sigma_net_2", "color_net_0", "color_net_1", "color_net_2"]
    blob = synth.blob_from_manifest([e for e in ent if "embeddings" not in e[0]])
    table = synth.blob_from_manifest([e for e in ent if "embeddings" in e[0]])
    lr = float(g["lr"][0])
    for p0, grad, ref in ((blob, np.concatenate([g[f"s1_grad_model_{n}.weight"].reshape(-1) for n in names]), np.concatenate([g[f"s1_param_model_{n}.weight"].reshape(-1) for n in names])),
                          (table, np.stack([g[f"s1_grad_embedder_embeddings_{l}.weight"] for l in range(4)]).reshape(-1),
                           np.stack([g[f"s1_param_embedder_embeddings_{l}.weight"] for l in range(4)]).reshape(-1))):
        p1, _, _ = TT.adam(p0, grad, np.zeros_like(p0), np.zeros_like(p0), lr, 0.9, 0.99, 1e-15, 1)
        np.testing.assert_allclose(p1, ref, rtol=0, atol=2e-7)


# ------------------------------------------------------------------ Trainer geometry
LADDERS = {"golden": (16, 256, 6), "workload": (16, 512, 16),
           "low-clip": (4, 2048, 12),        # floor(res / 10) lies below base - 1 = 3 on the coarse levels (clipped up) and above it, unclipped, from res = 40 on
           "both-ends": (2, 2, 2)}           # base - 1 = finest - 1 = 1: the clip's two ends meet and res / 10 = 0.2 lands on them.  (floor(res / 10) > finest - 1 alone needs
                                             # res <= finest < 10 / 9, a one-cell lattice with cube 0, which nrf_hash_tv_loss refuses: the upper end is reachable only like this)


def test_tv_cuboids_equal_the_reference_resolutions():
    from nerfpp_amd.train import tv_cuboids
    g = load_golden("tv_loss")
    cub = tv_cuboids(16, 256, 6, 0, 0)
    assert [c[0] for c in cub] == list(range(6))
    for level in (0, 3, 5):
        assert (cub[level][1], cub[level][2]) == tuple(int(x) for x in g[f"l{level}_res_cube"]), level


@pytest.mark.parametrize("ladder", LADDERS, ids=list(LADDERS))
def test_tv_cuboids_stay_inside_the_lattice_and_draw_afresh(ladder):
    from nerfpp_amd.train import tv_cuboids
    base, finest, n_levels = LADDERS[ladder]
    per_step = []
    for t in range(51):
        cub = tv_cuboids(base, finest, n_levels, 5, t)
        assert len(cub) == n_levels and cub == tv_cuboids(base, finest, n_levels, 5, t), "same (seed, t), same draws"
        for level, res, cube, mv in cub:
            assert base <= res <= finest and base - 1 <= cube <= finest - 1 and cube == min(max(res // 10, base - 1), finest - 1), (level, res, cube)
            assert len(mv) == 3 and all(isinstance(x, int) for x in mv)
            for a in range(3):
                assert 0 <= mv[a] < max(res - cube, 1) and mv[a] + cube <= res, (t, level, res, cube, mv)
        per_step.append([c[3] for c in cub])
    assert [c[1] for c in cub][0] == base and [c[1] for c in cub][-1] in (finest - 1, finest)
    if ladder == "low-clip":
        assert any(res // 10 < base - 1 for _, res, _, _ in cub) and any(res // 10 > base - 1 and cube == res // 10 for _, res, cube, _ in cub)
    if ladder == "both-ends":
        assert all(cube == base - 1 == finest - 1 for _, _, cube, _ in cub)
        return          # res - cube = 1: the only lattice position is 0, nothing to draw
    wide = [l for l, res, cube, _ in cub if res - cube >= 8]          # levels with room for the draws to differ
    assert len(wide) >= 2
    for t in range(50):
        assert [per_step[t][l] for l in wide] != [per_step[t + 1][l] for l in wide], "another step draws other cuboids"
        assert len({per_step[t][l] for l in wide}) > 1, "levels draw their own cuboids"
    assert [c[3] for c in tv_cuboids(base, finest, n_levels, 6, 0)] != per_step[0], "another seed draws other cuboids"
    # every position of a span is reached: the draw is randint's [0, res - cube)
    l0 = wide[0]
    span = cub[l0][1] - cub[l0][2]
    xs = {tv_cuboids(base, finest, n_levels, s, t)[l0][3][0] for s in range(40) for t in range(0, 50, 7)}
    assert min(xs) == 0 or span > 40
    assert max(xs) < span


def test_add_tv_loss_goes_through_tv_cuboids():
    from nerfpp_amd import train
    src = inspect.getsource(train.Trainer.add_tv_loss)
    assert "tv_cuboids(e.BaseResolution, e.FinestResolution, e.NLevels, self.seed, self.t)" in src and "math." not in src and "_rng_u32" not in src
