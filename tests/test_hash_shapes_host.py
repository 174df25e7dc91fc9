"""CPU tests of tests/hash_shapes_ref.py, the case list of the level-major hash encoder tests (tests/test_hash_shapes_gpu.py runs the kernels on it):
  coverage   CASES is exactly the 28 named cases, each holding the property it is named for (removing or altering any of them fails here), and together they reach
             every value of every decision dispatch() restates;
  yardstick  the C oracle (O.hash_cu, O.hash_ngp) equals an independent numpy float32 restatement of the two encoders bit for bit, keep mask included, on every
             case's points -- biases, non-cubic boxes and injected scales have no compiled reference, so this second statement is what stands behind the oracle there;
  inputs     every named kind of point is present, and every case's keep mask is false for some points and true for most."""
import numpy as np
import pytest

from conftest import load_golden
from nerfpp_amd import synth
from oracle import capi as O
import hash_shapes_ref as HS

bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, want, kinds, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((bits(got) != bits(want)).reshape(got.shape[0], -1).any(1))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {got.shape[0]} points differ, first {bad[:5]} ({HS.kind_of(kinds, bad[0])}): {got[bad[0]]} vs {want[bad[0]]}"


_same_box = lambda c, box: np.array_equal(c.bbox, np.asarray(box, np.float32))
_grid = lambda c: (c.mode, c.L, c.F, c.T, c.base, c.finest)
_plain = lambda c: c.biases is None and c.scales is None and c.budget == HS.ALL and _same_box(c, HS.LEGO_BBOX)
_l16 = lambda c: _grid(c) == ("cu", 16, 2, 10, 4, 64)
# what each case is named for, as a property of the case itself (its grid, box, biases, scales, budget) and of its dispatch: a case that is removed, renamed or
# quietly changed into a twin of another fails check_cases()
NAMED_FOR = {
    "cu-L16": lambda c, d: _l16(c) and _plain(c) and d["straight"] and d["n_baked"] == 16,
    "cu-L8": lambda c, d: c.L == 8 and c.F == 2 and _plain(c) and d["lc"] == 4,
    "cu-L9": lambda c, d: c.L == 9 and c.F == 2 and _plain(c) and (c.L - d["lc"]) % 2 == 1 and d["fine_lpt"] == 1 and d["n_baked"] == 9,
    "cu-L12": lambda c, d: c.L == 12 and c.F == 2 and _plain(c) and d["lc"] == 8,
    "cu-L20": lambda c, d: c.L == 20 and c.F == 2 and _plain(c) and d["lc"] == 12 and c.L - d["lc"] == 8,
    "cu-L24": lambda c, d: c.L == 24 and c.F == 2 and _plain(c) and d["lc"] == 16 and d["coarse_lpt"] == 4,
    "cu-L32": lambda c, d: c.L == HS.MAX_LEVELS and c.F == 2 and _plain(c) and d["lc"] == 24 and d["coarse_lpt"] == 12,
    "cu-L16-budget-through-5": lambda c, d: _l16(c) and d["n_baked"] == 6 and c.budget == d["baked_bytes"] and d["coarse_kind"] == "mixed",
    "cu-L16-budget-through-5-less-1": lambda c, d: _l16(c) and d["n_baked"] == 5 and c.budget == HS.BY_NAME["cu-L16-budget-through-5"].budget - 1,
    "cu-L16-budget-through-13": lambda c, d: _l16(c) and d["n_baked"] == 14 and c.budget == d["baked_bytes"] and d["fine_kind"] == "mixed",
    "cu-L16-budget-through-13-less-1": lambda c, d: _l16(c) and d["n_baked"] == 13 and c.budget == HS.BY_NAME["cu-L16-budget-through-13"].budget - 1,
    "cu-L16-budget-0": lambda c, d: _l16(c) and c.budget == 0 and c.biases is None and d["n_baked"] == 0,
    "cu-L16-bias": lambda c, d: _l16(c) and c.budget == HS.ALL and c.biases.shape == (16, 3) and (c.biases > 0).all() and (c.biases < 1).all() and d["n_baked"] == 0,
    "cu-L16-box": lambda c, d: _l16(c) and _same_box(c, HS.NONCUBIC) and c.biases is None and d["straight"],
    "cu-L16-T4": lambda c, d: _grid(c) == ("cu", 16, 2, 4, 4, 64) and _plain(c) and HS.local_size_of(c) == 16,
    "cu-L16-T5": lambda c, d: _grid(c) == ("cu", 16, 2, 5, 4, 64) and _plain(c) and HS.local_size_of(c) == 32,
    "cu-L16-scales-integers": lambda c, d: _l16(c) and c.scales.min() == 1.0 and (c.scales == np.floor(c.scales)).sum() >= 4 and (c.scales != np.floor(c.scales)).any() and d["dim"][0] == 3,
    "cu-L16-scales-64bit": lambda c, d: _l16(c) and c.scales[-1] == HS.SCALE_64 and d["lookup"].count("baked64") == 1 and not d["straight"] and d["n_baked"] == 16,
    "lmf-L2-F1": lambda c, d: _grid(c)[:4] == ("cu", 2, 1, 4) and _plain(c) and d["fine"] == "k_hash_cu_lmf<1, 1>",
    "lmf-L5-F1-bias-box": lambda c, d: (_grid(c)[:4] == ("cu", 5, 1, 6) and _same_box(c, HS.NONCUBIC) and c.biases.shape == (5, 3) and (c.biases >= 100).all()
                                        and (c.biases < 1100).all() and d["fine"] == "k_hash_cu_lmf<1, 1>"),
    "lmf-L3-F4": lambda c, d: _grid(c)[:4] == ("cu", 3, 4, 8) and _plain(c) and d["fine"] == "k_hash_cu_lmf<4, 1>",
    "lmf-L7-F2": lambda c, d: _grid(c)[:4] == ("cu", 7, 2, 10) and _plain(c) and d["fine"] == "k_hash_cu_lmf<2, 1>",
    "lmf-L16-F8": lambda c, d: _grid(c)[:4] == ("cu", 16, 8, 12) and _plain(c) and d["fine"] == "k_hash_cu_lmf<8, 1>",
    "ngp-4-64": lambda c, d: _grid(c) == ("ngp", 16, 2, 12, 4, 64) and _plain(c) and d["n_baked"] == 16 and d["coarse_kind"] == d["fine_kind"] == "baked",
    "ngp-2-30": lambda c, d: _grid(c) == ("ngp", 16, 2, 10, 2, 30) and _plain(c) and d["n_baked"] == 16 and (d["scales"][:3] == 2).all() and d["scales"][4] == d["scales"][5],
    "ngp-16-2048": lambda c, d: _grid(c) == ("ngp", 16, 2, 14, 16, 2048) and _plain(c) and d["n_baked"] == 13 and d["entries"][13] >= 1 << 30,
    "ngp-box": lambda c, d: _grid(c) == ("ngp", 16, 2, 12, 4, 64) and _same_box(c, HS.NONCUBIC) and c.budget == HS.ALL and d["n_baked"] == 16,
    "ngp-budget-0": lambda c, d: _grid(c) == ("ngp", 16, 2, 12, 4, 64) and _same_box(c, HS.LEGO_BBOX) and c.budget == 0 and d["n_baked"] == 0,
}


def check_cases(cases):
    """the list is exactly the named cases, and each is what its name says"""
    names = [c.name for c in cases]
    assert len(set(names)) == len(names) and set(names) == set(NAMED_FOR), sorted(set(names) ^ set(NAMED_FOR))
    for c in cases:
        try:
            ok = bool(NAMED_FOR[c.name](c, HS.dispatch(c)))
        except (AttributeError, TypeError):          # biases / scales that the property reads are None
            ok = False
        assert ok, c.name + " is no longer the case it is named for"


def test_every_case_is_the_one_it_is_named_for():
    assert len(HS.CASES) == 28 and HS.BY_NAME == {c.name: c for c in HS.CASES}
    assert HS.CU_CASES + HS.NGP_CASES == HS.CASES          # what the GPU tests parametrise over is the whole list
    check_cases(HS.CASES)


def test_removing_or_twinning_any_case_fails_the_check():
    """the removal experiment, for all 28: the list without case i fails check_cases; so does the list with case i replaced by a renamed copy of its neighbour"""
    for i, c in enumerate(HS.CASES):
        with pytest.raises(AssertionError):
            check_cases(HS.CASES[:i] + HS.CASES[i + 1:])
        twin = HS.CASES[(i + 1) % len(HS.CASES)]._replace(name=c.name)
        with pytest.raises(AssertionError):
            check_cases(HS.CASES[:i] + [twin] + HS.CASES[i + 1:])


def test_case_list_reaches_every_branch():
    """Every value of every host decision is taken by at least one case, and by the case named for it."""
    d = {c.name: HS.dispatch(c) for c in HS.CASES}
    lm = {n: v for n, v in d.items() if v["path"] == "lm"}
    reach = lambda key, src=lm: {v[key] for v in src.values()}
    assert reach("lc") == {4, 8, 12, 16, 24}
    assert reach("coarse_lpt") == {4, 12} and reach("fine_lpt") == {1, 2}
    assert reach("straight") == {True, False}
    assert reach("coarse") == {"k_hash_cu_lm<1, 0, 4>", "k_hash_cu_lm<1, 0, 12>", "k_hash_cu_lm<1, 0, 12, 3>"}
    assert reach("fine") == {"k_hash_cu_lm<1, 0, 1>", "k_hash_cu_lm<1, 0, 2>", "k_hash_cu_lm<1, 0, 2, 2>"}
    assert reach("coarse_kind") == {"baked", "hashed", "mixed"} and reach("fine_kind") == {"baked", "hashed", "mixed"}
    assert {k for v in lm.values() for k in v["lookup"]} == {"straight", "baked32", "baked64", "hashed"}
    assert {v["fine"] for v in d.values() if v["path"] == "lmf"} == {"k_hash_cu_lmf<%d, 1>" % f for f in (1, 2, 4, 8)}
    assert {(v["coarse"], v["fine"]) for v in d.values() if v["path"] == "ngp"} == {("k_hash_ngp_lm<4>", "k_hash_ngp_lm<1>")}
    assert {v["fine_kind"] for v in d.values() if v["path"] == "ngp"} == {"baked", "hashed", "mixed"} and {v["coarse_kind"] for v in d.values() if v["path"] == "ngp"} == {"baked", "hashed"}
    # the cases named for a branch take it
    pair = lambda n: (d[n]["coarse"], d[n]["fine"])
    assert pair("cu-L16") == ("k_hash_cu_lm<1, 0, 12, 3>", "k_hash_cu_lm<1, 0, 2, 2>") and d["cu-L16"]["lc"] == 12
    assert pair("cu-L8") == ("k_hash_cu_lm<1, 0, 4>", "k_hash_cu_lm<1, 0, 2, 2>") and d["cu-L8"]["lc"] == 4
    assert pair("cu-L9") == ("k_hash_cu_lm<1, 0, 4>", "k_hash_cu_lm<1, 0, 1>") and d["cu-L9"]["lc"] == 4 and d["cu-L9"]["straight"]
    assert pair("cu-L12") == ("k_hash_cu_lm<1, 0, 4>", "k_hash_cu_lm<1, 0, 2, 2>") and d["cu-L12"]["lc"] == 8
    assert pair("cu-L20") == ("k_hash_cu_lm<1, 0, 12, 3>", "k_hash_cu_lm<1, 0, 2, 2>") and d["cu-L20"]["lc"] == 12
    assert pair("cu-L24") == ("k_hash_cu_lm<1, 0, 4>", "k_hash_cu_lm<1, 0, 2, 2>") and d["cu-L24"]["lc"] == 16
    assert pair("cu-L32") == ("k_hash_cu_lm<1, 0, 12, 3>", "k_hash_cu_lm<1, 0, 2, 2>") and d["cu-L32"]["lc"] == 24 and HS.BY_NAME["cu-L32"].L == HS.MAX_LEVELS
    for n in ("cu-L16-budget-0", "cu-L16-bias"):
        assert pair(n) == ("k_hash_cu_lm<1, 0, 4>", "k_hash_cu_lm<1, 0, 1>") and d[n]["n_baked"] == 0 and d[n]["baked_bytes"] == 0
    for n in ("cu-L16-box", "cu-L16-T4", "cu-L16-T5", "cu-L16-scales-integers"):
        assert d[n]["straight"] and d[n]["n_baked"] == 16, n
    assert d["cu-L16-scales-integers"]["dim"][0] == 3 and d["cu-L16-scales-integers"]["nby"][0] == 1
    big = d["cu-L16-scales-64bit"]
    assert pair("cu-L16-scales-64bit") == ("k_hash_cu_lm<1, 0, 12>", "k_hash_cu_lm<1, 0, 2>") and big["n_baked"] == 16 and not big["straight"]
    assert big["lookup"].count("baked64") == 1 and big["lookup"][15] == "baked64" and (4 << 30) < big["baked_bytes"] < (9 << 29)
    assert d["ngp-16-2048"]["n_baked"] == 13 and d["ngp-16-2048"]["entries"][13] >= 1 << 30 and d["ngp-16-2048"]["baked_bytes"] < (24 << 30)
    assert d["lmf-L7-F2"]["n_baked"] == 7          # hash_fast_prepare bakes an F = 2 grid whatever its depth; k_hash_cu_lmf does not read the image
    # every large image belongs to a case that is named for it: everything else costs kilobytes to a few megabytes
    assert all(v["baked_bytes"] < (32 << 20) for n, v in d.items() if n not in ("cu-L16-scales-64bit", "ngp-16-2048"))
    # the store form (hash_lm_body): 32-bit below 4 GB of feature planes
    assert HS.dispatch(HS.BY_NAME["cu-L32"], pstride=(1 << 25) - 1)["store32"] and not HS.dispatch(HS.BY_NAME["cu-L32"], pstride=1 << 25)["store32"]


def test_64bit_addressing_boundary():
    s = HS.SCALE_64
    assert ((s + 5) // 4) ** 2 * (s + 2) >= 1 << 24 > ((s + 4) // 4) ** 2 * (s + 1)
    assert ((s + 5) // 4) ** 2 * (s + 2) * 16 < 1 << 30, "the level is still baked"


@pytest.mark.parametrize("k", [5, 13])
def test_budget_boundary_has_both_outcomes(k):
    """budget == cumulative bytes through level k bakes level k; one byte less does not (the `>` of hash_fast_prepare)"""
    at, below = HS.BY_NAME["cu-L16-budget-through-%d" % k], HS.BY_NAME["cu-L16-budget-through-%d-less-1" % k]
    full = HS.dispatch(HS.BY_NAME["cu-L16"])
    cum = np.cumsum(full["entries"]) * 16
    assert at.budget == cum[k] and below.budget == cum[k] - 1
    da, db = HS.dispatch(at), HS.dispatch(below)
    assert (da["n_baked"], da["baked_bytes"]) == (k + 1, cum[k]) and (db["n_baked"], db["baked_bytes"]) == (k, cum[k - 1])
    assert (k < full["lc"]) == (da["coarse_lpt"] == 4) and (k < full["lc"]) == (da["coarse_kind"] == "mixed") and (k >= full["lc"]) == (da["fine_kind"] == "mixed")
    assert not da["straight"] and not db["straight"]


def test_held_bytes_rule():
    assert HS.held_bytes(0, 100) == 100 and HS.held_bytes(100, 60) == 100 and HS.held_bytes(100, 49) == 49 and HS.held_bytes(100, 101) == 101 and HS.held_bytes(100, 0) == 0


@pytest.mark.parametrize("case", HS.CASES, ids=HS.case_id)
def test_points_and_keep_mask(case):
    x, kinds, emb, keep = HS.expected(case.name)
    assert x.dtype == np.float32 and 5900 <= x.shape[0] <= 6100 and tuple(kinds) == HS.KINDS
    at = 0
    for name in HS.KINDS:
        s = kinds[name]
        assert s.start == at and s.stop > s.start, name
        at = s.stop
    assert at == x.shape[0]
    mn, mx = case.bbox[:3], case.bbox[3:]
    inside = ((x >= mn) & (x <= mx)).all(1)
    assert np.array_equal(keep, inside)
    assert inside[kinds["inside"]].all() and inside[kinds["on a face"]].all() and inside[kinds["corners and centre"]].all()
    assert inside[kinds["coarsest lattice"]].all() and inside[kinds["finest lattice"]].all()
    assert 0.2 < (~inside[kinds["outside"]]).mean() < 0.9
    f = x[kinds["on a face"]]
    assert (((f == mn) | (f == mx)).sum(1) >= 1).all() and (f == mn).any() and (f == mx).any()
    nz = x[kinds["negative zero"]]
    assert ((nz == 0) & np.signbit(nz)).any(1).all()
    assert (~keep).sum() >= 100 and keep.mean() > 0.5
    assert np.isfinite(emb).all() and np.abs(emb).max() > 0.05


@pytest.mark.parametrize("case", HS.CU_CASES, ids=HS.case_id)
def test_oracle_cu_equals_the_numpy_restatement(case):
    x, kinds, emb, keep = HS.expected(case.name)
    ref, rkeep = HS.ref_hash_cu(case, x)
    assert np.array_equal(keep, rkeep)
    same_bits(emb, ref, kinds, case.name)
    assert emb.shape == (x.shape[0], case.L * case.F)
    assert len(np.unique(emb[kinds["inside"]], axis=0)) > 0.9 * (kinds["inside"].stop - kinds["inside"].start)


@pytest.mark.parametrize("case", HS.NGP_CASES, ids=HS.case_id)
def test_oracle_ngp_equals_the_numpy_restatement(case):
    x, kinds, emb, keep = HS.expected(case.name)
    assert np.array_equal(HS.ngp_resolutions(case.L, case.base, case.finest), O.hash_ngp_resolutions(case.L, case.base, case.finest))
    ref, rkeep = HS.ref_hash_ngp(x, HS.table_of(case), case.bbox, case.L, case.F, case.T, case.base, case.finest)
    assert np.array_equal(keep, rkeep)
    same_bits(emb, ref, kinds, case.name)


def test_ngp_resolutions_repeat_where_the_case_says_so():
    c = HS.BY_NAME["ngp-2-30"]
    r = HS.dispatch(c)["scales"]
    assert np.array_equal(r, O.hash_ngp_resolutions(c.L, c.base, c.finest)) and len(set(r.tolist())) < 16 and r[0] == 2 and r[-1] >= 29


def test_ngp_restatement_reproduces_the_reference_golden(manifest):
    """... and the restatement is the reference's HashEmbedder: its recorded LibTorch embedding (tests/golden/hash_small), bit for bit"""
    g = load_golden("hash_small")
    L, F, T, base, fine = (int(v) for v in g["cfg"])
    ref, keep = HS.ref_hash_ngp(g["x"], synth.blob_from_manifest(manifest["hash_small"]), g["bbox"], L, F, T, base, fine)
    assert np.array_equal(keep, g["mask"].astype(bool).reshape(-1))
    assert np.array_equal(bits(ref), bits(g["emb"].reshape(ref.shape)))


def test_exchanged_level_scales_are_visible():
    """What the bit comparisons are for: with the scales of levels 3 and 4 exchanged the restatement differs from the oracle on most points of level 3 and on none of
    level 5"""
    case = HS.BY_NAME["cu-L16-T4"]
    x, kinds, emb, _ = HS.expected(case.name)
    sc = HS.level_scales(case).copy(); sc[[3, 4]] = sc[[4, 3]]
    moved, _ = HS.ref_hash_cu(case, x, scales=sc)
    lv = emb.reshape(-1, case.L, case.F)
    assert (moved.reshape(lv.shape)[:, 3] != lv[:, 3]).any(1).mean() > 0.5 and np.array_equal(moved.reshape(lv.shape)[:, 5], lv[:, 5])
