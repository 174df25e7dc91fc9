"""GPU tests of the level-major hash-grid encoders at every grid shape their host dispatch distinguishes (hash_fast.hip: hash_fast_prepare, launch_hash_lm,
launch_hash_ngp_lm; encode.hip: nrf_hash_encode_lm_f16, nrf_hash_encode_lm_f16_strided).  Cases, points and the expected dispatch are tests/hash_shapes_ref.py's,
which tests/test_hash_shapes_host.py checks on the CPU; the yardstick is the C oracle (O.hash_cu, O.hash_ngp) and every comparison is equality of bits.

Which test executes which instantiation (HS.dispatch(case) names it; the baked byte count read back from the handle proves the bake the case is named for):
  k_hash_cu_lm<1, 0, 12, 3> + <1, 0, 2, 2>  straight-line pair ........ cu-L16, cu-L20, cu-L32 (grid.y 2), cu-L16-box, -T4, -T5, -scales-integers; tails; rebake
  k_hash_cu_lm<1, 0, 4> + <1, 0, 2, 2>      lc 4 / 8 / 16 ............. cu-L8, cu-L12, cu-L24
  k_hash_cu_lm<1, 0, 4> + <1, 0, 1>         baked, odd fine count ..... cu-L9; tails
                                            baked and hashed mixed .... cu-L16-budget-through-5, -through-5-less-1; rebake
                                            every level hashed ........ cu-L16-budget-0, cu-L16-bias (q + bias); rebake
  k_hash_cu_lm<1, 0, 12> + <1, 0, 2>        fine launch mixed ......... cu-L16-budget-through-13, -through-13-less-1; rebake
                                            one level on 64-bit loads . cu-L16-scales-64bit
  the pointer-store form of hash_lm_body (L * pstride * 4 == 2^32) .... test_level_major_64bit_stores on cu-L32
  k_hash_cu_lmf<1, 1>, <2, 1>, <4, 1>, <8, 1> ......................... lmf-L2-F1, lmf-L5-F1-bias-box, lmf-L7-F2, lmf-L3-F4, lmf-L16-F8
  k_hash_ngp_lm<4> + <1>: hi + lo planes, hi + lo + fp32, F32OUT ...... test_ngp_fast_path_vs_generic_encoder on the five ngp cases (baked, hashed and both)
  k_hash_cu<F> / k_hash_ngp<F> rows form on every case's grid ......... test_level_major_cu_vs_oracle (step 8), test_ngp_fast_path_vs_generic_encoder
Device memory: every image is kilobytes to 23 MB except two -- cu-L16-scales-64bit bakes 4.3 GB (the smallest level on the 64-bit path) and ngp-16-2048 bakes 24.4 GB
(13 levels at 32 B per entry: the entries >= 2^30 stop is not reached with less), each once; test_level_major_64bit_stores allocates 4 GiB and touches 2 MB of it.
The peak is the 24.4 GB image.  Every GPU step runs once."""
import ctypes as C

import numpy as np
import pytest
import torch

import hash_shapes_ref as HS
from split_fine_pass_check import check_default_split_fine_pass

pytestmark = pytest.mark.gpu

host = lambda t: t.detach().cpu().numpy()
P = lambda t: None if t is None else t.data_ptr()
F16_SENTINEL, KEEP_SENTINEL = 0x5A5A, 0xA5          # fp16 203.25: no feature of a table within +-0.5 has these bits; keep bytes are 0 or 1


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from types import SimpleNamespace
    from nerfpp_amd import _lib as L, modules as M, renderer as R, scene as S
    return SimpleNamespace(L=L, M=M, R=R, S=S, lib=L.lib())


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()          # (a copy: the shared expected() arrays are read-only)


def baked_bytes(api, e):
    tb, bb = C.c_int64(-1), C.c_int64(-1)
    api.L.check(api.lib.nrf_hash_memory_bytes(e._h, C.byref(tb), C.byref(bb)))
    assert tb.value == e.table_elems() * (2 if e.mode == api.L.NRF_HASH_CU else 4)
    return int(bb.value)


def make_cu(api, case, budget=None):
    """A fresh CuHashEmbedder on the case's grid.  Level scales and budget go in before the table and the primes complete the handle: its FIRST bake is then the case's,
    and the image is allocated at exactly the baked size (a later re-bake may keep a larger allocation: HS.held_bytes)."""
    e = api.M.CuHashEmbedder("embedder", case.bbox, case.L, case.F, case.T, case.base, case.finest)
    default = e.level_scales()
    assert np.array_equal(default.view(np.uint32), HS.O.hash_cu_scales(case.L, case.base, case.finest).view(np.uint32)), "the handle's own level scales == the oracle's"
    if case.scales is not None:
        e.set_level_scales(case.scales)
    assert np.array_equal(e.level_scales().view(np.uint32), HS.level_scales(case).view(np.uint32))
    e.set_dense_budget(case.budget if budget is None else budget)
    e.set_table(HS.table_of(case))
    assert baked_bytes(api, e) == 0, "no image before the primes are set"
    e.set_primes(HS.primes_of(case), case.biases)
    return e


def encode_lm(api, e, xd, p, pstride, entry="strided"):
    """one level-major encode into sentinel-filled buffers -> (features [L, pstride, F] as fp16 bit patterns, keep bytes [p + 3])"""
    L, F = e.NLevels, e.NFeaturesPerLevel
    feats = torch.full((L, pstride, F), F16_SENTINEL, dtype=torch.int16, device="cuda")
    keep = torch.full((p + 3,), KEEP_SENTINEL, dtype=torch.uint8, device="cuda")
    if entry == "strided":
        api.L.check(api.lib.nrf_hash_encode_lm_f16_strided(e._h, P(xd), p, P(feats), pstride, P(keep), None))
    else:
        assert pstride == p
        api.L.check(api.lib.nrf_hash_encode_lm_f16(e._h, P(xd), p, P(feats), P(keep), None))
    torch.cuda.synchronize()
    return host(feats).view(np.uint16), host(keep)


def check_lm(got, keep, want_bits, want_keep, p, kinds, what):
    """features of columns < p == the oracle's, columns >= p untouched, keep bytes == the oracle's and untouched past p"""
    feats = got[:, :p]
    assert feats.shape == want_bits.shape, (what, feats.shape, want_bits.shape)
    bad = np.argwhere(feats != want_bits)
    assert bad.shape[0] == 0, (f"{what}: {bad.shape[0]} of {feats.size} values differ in levels {sorted(set(bad[:, 0].tolist()))}; first (level, point, feature) {bad[0].tolist()}"
                               f"{' -- ' + HS.kind_of(kinds, bad[0, 1]) if kinds else ''}: {feats[tuple(bad[0])]:#06x} vs {want_bits[tuple(bad[0])]:#06x}")
    assert (got[:, p:] == F16_SENTINEL).all(), f"{what}: columns past the batch were written"
    assert np.array_equal(keep[:p], want_keep.astype(np.uint8)), f"{what}: keep mask"
    assert (keep[p:] == KEEP_SENTINEL).all(), f"{what}: keep bytes past the batch were written"


# ------------------------------------------------------------------ (a) every CU case against the oracle
@pytest.mark.parametrize("case", HS.CU_CASES, ids=HS.case_id)
def test_level_major_cu_vs_oracle(api, case):
    """nrf_hash_encode_lm_f16_strided (pstride = p + 37), nrf_hash_encode_lm_f16 and the rows form nrf_hash_encode on one handle against O.hash_cu on the case's ~6000
    points; the handle's baked byte count == dispatch()'s, so the instance the case is named for is the one that ran."""
    d = HS.dispatch(case)
    x, kinds, emb, keep_o = HS.expected(case.name)
    e = make_cu(api, case)
    got_bytes = baked_bytes(api, e)
    print(f"{case.name}: {d['coarse']} + {d['fine']}, {d['n_baked']} of {case.L} levels baked, {got_bytes} bytes (dispatch: {d['baked_bytes']})")
    assert got_bytes == d["baked_bytes"], (case.name, got_bytes, d["baked_bytes"], d["n_baked"])
    want = HS.level_major(HS.f16_bits(emb), case.L, case.F)
    xd, p = dev(x), x.shape[0]
    assert HS.dispatch(case, pstride=p + 37)["store32"] in (True, None)
    got, keep = encode_lm(api, e, xd, p, p + 37)
    check_lm(got, keep, want, keep_o, p, kinds, case.name + " strided")
    got2, keep2 = encode_lm(api, e, xd, p, p, entry="plain")
    check_lm(got2, keep2, want, keep_o, p, kinds, case.name + " pstride = p")
    rows, mask = e.forward(xd)
    rows = host(rows)
    assert np.array_equal(host(mask), keep_o), case.name + ": keep mask of the rows form"
    bad = np.argwhere(rows.view(np.uint32) != emb.view(np.uint32))
    assert bad.shape[0] == 0, f"{case.name} rows form: {bad.shape[0]} values differ, first (point, column) {bad[0].tolist()} -- {HS.kind_of(kinds, bad[0, 0])}"


# ------------------------------------------------------------------ (b) tails
@pytest.mark.parametrize("name", ["cu-L16", "cu-L9"])
def test_level_major_tails(api, name):
    """p = 1, 255, 256, 257, 513 (one point; both sides of the 256-point block edge; a third block) through both entries, points drawn across all kinds; p = 0 is OK and
    writes nothing"""
    case = HS.BY_NAME[name]
    x, kinds, emb, keep_o = HS.expected(name)
    e = make_cu(api, case)
    assert baked_bytes(api, e) == HS.dispatch(case)["baked_bytes"]
    want_all = HS.f16_bits(emb)
    for p in (1, 255, 256, 257, 513):
        idx = (np.arange(p) * 37 + 11 * p) % x.shape[0]          # a stride through every kind of point
        xd = dev(x[idx])
        want = HS.level_major(want_all[idx], case.L, case.F)
        for pstride, entry in ((p + 37, "strided"), (p, "plain")):
            got, keep = encode_lm(api, e, xd, p, pstride, entry)
            check_lm(got, keep, want, keep_o[idx], p, None, f"{name} p {p} {entry}")
    xd = dev(x[:4])
    feats = torch.full((case.L, 4, case.F), F16_SENTINEL, dtype=torch.int16, device="cuda")
    keep = torch.full((4,), KEEP_SENTINEL, dtype=torch.uint8, device="cuda")
    assert api.lib.nrf_hash_encode_lm_f16_strided(e._h, P(xd), 0, P(feats), 4, P(keep), None) == api.L.NRF_OK
    assert api.lib.nrf_hash_encode_lm_f16(e._h, P(xd), 0, P(feats), P(keep), None) == api.L.NRF_OK
    torch.cuda.synchronize()
    assert bool((feats == F16_SENTINEL).all()) and bool((keep == KEEP_SENTINEL).all()), "p = 0 writes nothing"


# ------------------------------------------------------------------ (c) the 64-bit store form
def test_level_major_64bit_stores(api):
    """cu-L32, p = 1000, pstride = 2^25: L * pstride * 4 == 2^32, so hash_lm_body stores through pointers instead of the 32-bit buffer resource.  The 4 GiB buffer is
    only ever touched in its first 1064 columns per level."""
    case = HS.BY_NAME["cu-L32"]
    x, kinds, emb, keep_o = HS.expected(case.name)
    p, pstride = 1000, 1 << 25
    assert HS.dispatch(case, pstride=pstride)["store32"] is False and HS.dispatch(case, pstride=pstride - 1)["store32"] is True
    idx = (np.arange(p) * 5 + 3) % x.shape[0]
    e = make_cu(api, case)
    xd = dev(x[idx])
    want = HS.level_major(HS.f16_bits(emb)[idx], case.L, case.F)
    big = torch.empty((case.L, pstride, case.F), dtype=torch.int16, device="cuda")
    assert big.numel() * 2 == 1 << 32
    big[:, :p + 64] = F16_SENTINEL
    keep = torch.full((p + 3,), KEEP_SENTINEL, dtype=torch.uint8, device="cuda")
    api.L.check(api.lib.nrf_hash_encode_lm_f16_strided(e._h, P(xd), p, P(big), pstride, P(keep), None))
    torch.cuda.synchronize()
    got = host(big[:, :p + 64].contiguous()).view(np.uint16)
    del big
    check_lm(got, host(keep), want, keep_o[idx], p, None, "cu-L32 pstride 2^25")
    got2, keep2 = encode_lm(api, e, xd, p, p, entry="plain")
    assert np.array_equal(got2, got[:, :p]) and np.array_equal(keep2, host(keep)), "pointer stores == buffer stores"


# ------------------------------------------------------------------ (d) re-bakes on one handle
def test_rebake_follows_the_handle(api):
    """One cu-L16 handle through the budgets all -> through level 5 -> one byte less -> 0 -> one byte less than through level 5 again -> through level 13 -> 0 -> one byte
    less than through level 13 -> all, then new level scales, then a new table.  After every change the features equal the oracle's for that state and the handle holds
    the bytes hash_fast_prepare's allocation rule gives (HS.held_bytes over dispatch()'s baked bytes).  Baked and hashed lookups return the same bits, so it is the byte
    count that says how many levels were baked -- and only where the image is allocated anew (held == baked bytes): every step but the third, which keeps the larger
    image of the step before and pins the allocation rule alone; its budget comes back after the 0, on an empty handle, where the count is exact.  A stale image, or
    stale dense offsets / extents, shows as wrong features in the scales and table steps."""
    case = HS.BY_NAME["cu-L16"]
    x, kinds, emb, keep_o = HS.expected(case.name)
    xd, p = dev(x), x.shape[0]
    e = make_cu(api, case)
    held = baked_bytes(api, e)
    assert held == HS.dispatch(case)["baked_bytes"]
    want = HS.level_major(HS.f16_bits(emb), case.L, case.F)
    walk = (("cu-L16", True), ("cu-L16-budget-through-5", True), ("cu-L16-budget-through-5-less-1", False), ("cu-L16-budget-0", True), ("cu-L16-budget-through-5-less-1", True),
            ("cu-L16-budget-through-13", True), ("cu-L16-budget-0", True), ("cu-L16-budget-through-13-less-1", True), ("cu-L16", True))
    for step, (name, exact) in enumerate(walk):
        budget = HS.BY_NAME[name].budget
        e.set_dense_budget(budget)
        need = HS.dispatch(case, budget)["baked_bytes"]
        held = HS.held_bytes(held, need)
        assert (held == need) == exact, (step, name, held, need)
        assert baked_bytes(api, e) == held, (step, name, baked_bytes(api, e), held)
        got, keep = encode_lm(api, e, xd, p, p + 37)
        check_lm(got, keep, want, keep_o, p, kinds, f"step {step}, budget of {name}")
    scaled = case._replace(scales=HS.SCALES_INTEGERS)
    e.set_level_scales(scaled.scales)
    held = HS.held_bytes(held, HS.dispatch(scaled)["baked_bytes"])
    assert baked_bytes(api, e) == held
    emb2, keep2 = HS.oracle_cu(scaled, x)
    got, keep = encode_lm(api, e, xd, p, p + 37)
    check_lm(got, keep, HS.level_major(HS.f16_bits(emb2), case.L, case.F), keep2, p, kinds, "after new level scales")
    assert (emb2 != emb).any()
    table = HS.table_of(case, seed=1234)
    e.set_table(table)
    assert baked_bytes(api, e) == held
    emb3, keep3 = HS.oracle_cu(scaled, x, table=table)
    got, keep = encode_lm(api, e, xd, p, p + 37)
    check_lm(got, keep, HS.level_major(HS.f16_bits(emb3), case.L, case.F), keep3, p, kinds, "after a new table")
    assert (emb3 != emb2).mean() > 0.9


# ------------------------------------------------------------------ (e) HashEmbedder mode through the renderer
def rays_at(case, n=1500):
    """n rays from one camera outside the box, each through a point inside it: every ray crosses the box (a ray that misses has no depth range to sample)"""
    f = np.float32
    mn, mx = case.bbox[:3], case.bbox[3:]
    ctr, ext = (mn + mx) * f(0.5), mx - mn
    o = np.tile((ctr + np.array([3.0, 2.0, 2.5], f)).astype(f), (n, 1))
    tgt = ctr + (HS.synth.synth_u01(4711, n * 3).reshape(n, 3) - f(0.5)) * ext * f(0.9)
    d = (tgt - o).astype(f)
    d = (d / np.sqrt((d * d).sum(1, keepdims=True))).astype(f)
    return dev(o), dev(d)


@pytest.mark.parametrize("case", HS.NGP_CASES, ids=HS.case_id)
def test_ngp_fast_path_vs_generic_encoder(api, case):
    """k_hash_ngp_lm on the case's grid, as test_ngp_fast_path_features_equal_generic_encoder checks it on the default scene: 1500 rays at 64 + 128 in two ragged chunks.
    Raw == the stage-wise split MLP on the generic encoder's features (zeros outside the box) bit for bit; the default split render passes
    check_default_split_fine_pass and its coarse weights and z_fine are the NRF_PREC_F32 render's bit for bit (the F32OUT instance); the generic encoder == O.hash_ngp
    on the case's points."""
    d = HS.dispatch(case)
    table = HS.table_of(case)
    sc = api.S.make_hash_scene(mode="ngp", n_levels=case.L, n_feat=case.F, log2_t=case.T, base=case.base, finest=case.finest, bbox=case.bbox, table=table,
                               dense_budget=case.budget)          # budget and table in force at the first bake: the image (24.4 GB for ngp-16-2048) is baked once
    e = sc["embedder"]
    assert np.array_equal(e.level_scales().view(np.uint32), d["scales"].view(np.uint32))
    got_bytes = baked_bytes(api, e)
    print(f"{case.name}: {d['coarse']} + {d['fine']}, {d['n_baked']} of {case.L} levels baked, {got_bytes} bytes (dispatch: {d['baked_bytes']})")
    assert got_bytes == d["baked_bytes"], (case.name, got_bytes, d["baked_bytes"])
    # the generic encoder on the case's points
    x, kinds, emb_o, keep_o = HS.expected(case.name)
    emb, mask = e.forward(dev(x))
    assert np.array_equal(host(mask), keep_o)
    bad = np.argwhere(host(emb).view(np.uint32) != emb_o.view(np.uint32))
    assert bad.shape[0] == 0, f"{case.name} generic encoder vs O.hash_ngp: {bad.shape[0]} values differ, first (point, column) {bad[0].tolist()} -- {HS.kind_of(kinds, bad[0, 0])}"
    # through the renderer
    o, dirs = rays_at(case)
    rp = api.S.lego_render_params(case.bbox, chunk=1000, precision=api.L.NRF_PREC_F16_SPLIT, ReturnRaw=True, KeepIntermediates=True)
    res = sc["renderer"].Render(0, 0, None, rp, rays=(o, dirs, None))
    rays, zf = res.Extras["rays_flat"], res.Extras["z_fine"]
    n, s = zf.shape
    assert (n, s) == (1500, 192)
    pts = (rays[:, None, 0:3] + rays[:, None, 3:6] * zf[..., None]).reshape(-1, 3)
    emb, keep = e.forward(pts)
    print(f"{case.name}: {float((~keep).float().mean()):.3f} of the fine depths lie outside the box")
    assert float(keep.float().mean()) > 0.9 and float(res.Extras["weights_coarse"].max()) > 0
    dd, _ = sc["embeddirs"].forward(rays[:, 8:11].contiguous())
    emb[~keep] = 0
    xin = torch.cat([emb, dd[:, None, :].expand(n, s, dd.shape[1]).reshape(n * s, -1)], 1).contiguous()
    ref = sc["mlp"].forward(xin, api.L.NRF_PREC_F16_SPLIT)
    ref[~keep, 3] = 0
    got, ref = host(res.Raw).reshape(-1, 4), host(ref)
    bad = np.nonzero((got.view(np.uint32) != ref.view(np.uint32)).any(1))[0]
    assert bad.size == 0, f"{case.name}: fast path Raw != stage-wise split MLP at {bad.size} of {n * s} depths, first {bad[:5]}"
    assert np.ptp(ref[:, 3]) > 0
    rp2 = api.S.lego_render_params(case.bbox, chunk=1000, precision=api.L.NRF_PREC_F16_SPLIT, ReturnRaw=True, KeepIntermediates="depths")
    res2 = sc["renderer"].Render(0, 0, None, rp2, rays=(o, dirs, None))
    check_default_split_fine_pass(api, sc, res2, rays, case.name + ", default split render")
    f32 = sc["renderer"].Render(0, 0, None, api.S.lego_render_params(case.bbox, chunk=1000, precision=api.L.NRF_PREC_F32, KeepIntermediates=True), rays=(o, dirs, None))
    for k in ("weights_coarse", "z_fine"):
        a, b = host(res2.Extras[k]), host(f32.Extras[k])
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{case.name}: {k} of the default split render != NRF_PREC_F32's"
