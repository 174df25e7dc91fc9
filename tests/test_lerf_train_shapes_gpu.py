"""The LeRF head's training backward on the MI355X at every shape and path it takes (nerfpp_amd/csrc/lerf_train.hip), through the C entries nrf_lerf_head_backward and
nrf_huber_rows_nanmean, against the float64 model of tests/lerf_train_ref.py (which tests/test_lerf_train_shapes_host.py holds to the reference-autograd goldens).
Workspaces of exactly *_workspace_bytes, a guard block behind them and behind every output; outputs start as NaN, so an element that is never written shows.

Bars (none taken from the code under test; the measured figures: profiles/lerf_train_shapes/measured_errors.txt):
  fp32 products (mode 0, and every case below the 256-point threshold of the split products): per tensor max(8 e_oracle, 16 * 2^-24) * max|ref|, e_oracle = the CPU fp32
    oracle's own error against the model on the same case, computed here;
  bf16x3 / f16x3 (modes 1 / 2; the default is f16x3): the bars of test_classic_and_lerf_train_steps_in_the_split_gemm_modes_follow_the_fp32_chain, now against float64 --
    every parameter tensor norm-wise 2e-3 / 2e-4; g_emb per ray of the ray's largest entry, weights absolute, rendered per component 3e-3 / 3e-4;
  the language loss: 2e-6 relative, its gradient rtol 1e-5 where finite."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import lerf_train_ref as T
import per_ray_ref as PR
from test_lerf_train_shapes_host import check_loss

pytestmark = pytest.mark.gpu

GUARD = 256
BAR_PARAM_NORM = {1: 2e-3, 2: 2e-4}          # norm-wise; measured worst 7.7e-5 / 1.3e-5: profiles/lerf_train_shapes/measured_errors.txt
BAR_VALUES = {1: 3e-3, 2: 3e-4}              # g_emb per ray, weights, rendered: measured worst 1.5e-4 / 2.5e-5 (g_emb; same file)
ORACLE_FACTOR, F32_FLOOR = 8.0, 16 * 2.0 ** -24          # fp32 products: measured worst 0.64 of this bar (same file)
BAR_ATOMICS_ORDER = 2e-6                     # float atomics in another order, x max|ref| (the `same` lambda of test_gpu_parity.py); measured 4.7e-7 (same file)
NRF_ERR_UNSUPPORTED = 3                      # include/nerfpp_hip.h
WORST = {}


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from nerfpp_amd import _lib as L
    from nerfpp_amd.modules import LeRF
    L.lib().nrf_dbg_lerf_train_gram.restype = C.c_int
    return L, LeRF


@pytest.fixture(scope="module")
def O():
    from oracle import capi
    return capi


@pytest.fixture(scope="module")
def heads(api):
    """(dims, blob seed) -> LeRF handle on lerf_train_ref.net's blob, created once."""
    _, LeRF = api
    made = {}

    def get(dims, seed=0):
        if (dims, seed) not in made:
            made[(dims, seed)] = LeRF(dims[3], dims[1], dims[2], dims[4], dims[0], "lang_model", params=T.net(dims, seed).blob)
        return made[(dims, seed)]
    return get


@contextlib.contextmanager
def settings(L, mode, gram):
    lib = L.lib()
    prev_mode, prev_gram = lib.nrf_get_train_gemm(), lib.nrf_dbg_lerf_train_gram(int(gram))
    try:
        L.check(lib.nrf_set_train_gemm(int(mode)))
        yield
    finally:
        lib.nrf_set_train_gemm(prev_mode)
        lib.nrf_dbg_lerf_train_gram(prev_gram)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Guarded:
    """nbytes of 0xFF (fp32 NaN) with GUARD more behind them."""

    def __init__(self, nbytes, init=None):
        self.n = int(nbytes)
        self.t = torch.full((self.n + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
        if init is not None:
            self.t[:self.n] = torch.from_numpy(np.ascontiguousarray(init).view(np.uint8).reshape(-1)).cuda()

    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def host(self, what):
        h = self.t.cpu().numpy()
        assert (h[self.n:] == 0xFF).all(), f"wrote behind {what}"
        return h[:self.n].view(np.float32).copy()


def run_head(L, h, c, prefill=None, null=(), n=None, expect=None):
    """nrf_lerf_head_backward on case c -> dict(weights, rendered, g_emb, g_params) of numpy arrays (None for an output in `null`).  n: the ray count passed (0: the
    empty call); expect: the status the call must return instead of NRF_OK (then every output must be untouched)."""
    lib = L.lib()
    dims, s = c["dims"], c["s"]
    n = c["n"] if n is None else n
    np_ = T.param_count(dims)
    ins = [_dev(c["emb"]), _dev(c["keep"]), _dev(c["z"]), _dev(c["d"]), _dev(c["noise"]), _dev(c["g_rendered"])]
    out = dict(g_params=Guarded(4 * np_, np.zeros(np_, np.float32) if prefill is None else prefill), g_emb=Guarded(4 * c["n"] * s * dims[0]),
               rendered=Guarded(4 * c["n"] * dims[4]), weights=Guarded(4 * c["n"] * s))
    nb = int(lib.nrf_lerf_head_backward_workspace_bytes(h._m, n, s))
    ws = Guarded(nb)
    ptr = lambda k: None if k in null else out[k].ptr()
    rc = lib.nrf_lerf_head_backward(h._m, _p(ins[0]), _p(ins[1]), _p(ins[2]), _p(ins[3]), c["d_stride"], n, s, _p(ins[4]), float(c["noise_std"]), _p(ins[5]),
                                    ptr("g_params"), ptr("g_emb"), ptr("rendered"), ptr("weights"), ws.ptr(), nb, None)
    torch.cuda.synchronize()
    ws.host("the workspace")
    res = {k: v.host(k) for k, v in out.items()}
    if expect is not None or n == 0:
        assert rc == (L.NRF_OK if expect is None else expect), (rc, L.lib().nrf_last_error())
        for k in ("g_emb", "rendered", "weights"):
            assert np.isnan(res[k]).all(), f"{k} was written by a call that does nothing"
        assert np.array_equal(res["g_params"], np.zeros(np_, np.float32) if prefill is None else prefill)
        return None
    L.check(rc)
    return {k: (None if k in null else v) for k, v in res.items()}


def effective_mode(c, mode, gram):
    """0 where every product of this call is an fp32 one (mode 0, or fewer than 256 points per pass), else 1 (bf16x3) / 2 (f16x3; the default)."""
    d = T.dispatch(c["dims"], c["n"], c["s"], mode, gram)
    return (2 if mode < 0 else mode) if d["split_fwd"] else 0


def oracle_figures(O, c, ref):
    if "e_oracle" not in c:
        d = c["dims"]
        o = O.lerf_head_backward(c["blob"], c["emb"], c["keep"], c["z"], np.ascontiguousarray(c["d"][:, :3]), c["g_rendered"], in_ch=d[0], n_layers=d[1], hidden=d[2],
                                 geo=d[3], embed=d[4], noise=c["noise"], noise_std=c["noise_std"])
        c["e_oracle"] = T.compare(c, ref, o["weights"], o["rendered"], o["g_emb"], o["g_params"])
    return c["e_oracle"]


def check(O, c, ref, got, mode, gram, group):
    """One result against the model at the bar of its arithmetic; the figures go to WORST[group, arithmetic, tensor] (printed by every test: pytest -s)."""
    scales = T.scale_model(c, ref)
    e = T.compare(c, ref, got["weights"], got["rendered"], got["g_emb"], got["g_params"], scales)
    arith = effective_mode(c, mode, gram)
    names = list(T.param_slices(c["dims"]))
    fails = []
    if arith == 0:
        eo = oracle_figures(O, c, ref)
        for k in [k for k in ("weights_rel", "rendered_rel", "g_emb") if k in e] + names:
            bar = max(ORACLE_FACTOR * eo[k], F32_FLOOR)
            note(group, "fp32", k, e[k] / bar)
            if not e[k] <= bar:
                fails.append((k, e[k], bar, eo[k]))
    else:
        for k in [k for k in ("weights", "rendered", "g_emb") if k in e]:
            note(group, ("bf16x3", "f16x3")[arith - 1], k, e[k])
            if not e[k] <= BAR_VALUES[arith]:
                fails.append((k, e[k], BAR_VALUES[arith]))
        for k in names:
            note(group, ("bf16x3", "f16x3")[arith - 1], "params (norm-wise)", e[k + "_norm"])
            if not e[k + "_norm"] <= BAR_PARAM_NORM[arith]:
                fails.append((k, e[k + "_norm"], BAR_PARAM_NORM[arith]))
    assert not fails, f"{c['tag']} mode {mode} gram {gram} (arithmetic {arith}): (tensor, error, bar[, oracle's error]) {fails}"
    return e


def note(group, arith, tensor, v):
    key = (group, arith, tensor if not tensor.startswith(("sigma_", "le_")) else "params (max-wise)")
    WORST[key] = max(WORST.get(key, 0.0), float(v))


def report(group):
    for (g, a, t), v in sorted(WORST.items()):
        if g == group:
            print(f"MEASURED {g:16s} {a:7s} {t:20s} {v:.3e}" + ("  (x the bar max(8 e_oracle, 16 * 2^-24))" if a == "fp32" else ""))


# ------------------------------------------------------------------------------------------------ sample counts
@pytest.mark.parametrize("s", T.SAMPLE_COUNTS)
def test_every_sample_count_and_density_kind(api, O, heads, s):
    """The wave scan at one and several samples per lane, forward and reverse, odd and even s (the 8-byte alignment pad), s = 1; every density kind of
    per_ray_ref.COMPOSITE_KINDS; a fully masked ray, dead points, keep = NULL and d_stride = 8 by the seeded draw.  Both forms of the last layer."""
    L, _ = api
    for sp in [sp for sp in T.sample_count_specs() if sp[2] == s]:
        c = T.make_case(*sp)
        ref = T.case_model(c)
        for gram in (1, 0):
            with settings(L, -1, gram):
                check(O, c, ref, run_head(L, heads(c["dims"]), c), -1, gram, "sample counts")
    report("sample counts")


# ------------------------------------------------------------------------------------------------ thresholds
@pytest.mark.parametrize("spec", T.threshold_specs(), ids=lambda sp: ("main" if sp[0] == T.MAIN else "small") + f"-{sp[1]}x{sp[2]}")
def test_both_sides_of_every_size_threshold_in_every_mode(api, O, heads, spec):
    """c = 256 (split forward / back-propagation, fused masks), c = 4096 (the Gram form's split products, beta_only, the two-segment weight gradient), rays = 256 (the
    per-ray split products) in nrf_set_train_gemm modes 0, 1, 2 and the default, both forms of the last layer."""
    L, _ = api
    c = T.make_case(*spec)
    ref = T.case_model(c)
    assert T.kink_census(c, ref).mean() <= T.MAX_KINK_SHARE
    for mode in T.MODES:
        for gram in (1, 0):
            with settings(L, mode, gram):
                check(O, c, ref, run_head(L, heads(c["dims"]), c), mode, gram, "thresholds")
    report("thresholds")


# ------------------------------------------------------------------------------------------------ head shapes
@pytest.mark.parametrize("dims", [d for d, _ in T.HEAD_SHAPES], ids=lambda d: "-".join(str(v) for v in d))
def test_head_shapes(api, O, heads, dims):
    """Every width that changes a path: L.out < 32, W % 4 != 0 (yo = 0), yo = 3 with geo & 3 != 0 and == 0, ragged and full hidden widths, the Gram form's refusals
    (hidden 257, one layer), three layers, embed 1 .. 768, in_ch 3 .. 128; each below and above c = 4096 in modes 0, 1, 2."""
    L, _ = api
    for sp in [sp for sp in T.head_shape_specs() if sp[0] == dims]:
        c = T.make_case(*sp)
        ref = T.case_model(c)
        assert T.kink_census(c, ref).mean() <= T.MAX_KINK_SHARE
        for mode in (0, 1, 2):
            with settings(L, mode, 1):
                check(O, c, ref, run_head(L, heads(dims), c), mode, 1, "head shapes")
    report("head shapes")


def test_zero_geo_width(api, O, heads):
    """geo = 0 (the LE net on the features alone; k_lt_copy_cols would be launched on an empty grid, every cat[geo, x] product gets an empty first segment): the call
    works and matches the model, below and above c = 4096, in every mode and both forms."""
    L, _ = api
    dims = T.GEO0
    h = heads(dims)
    for n, s in T.HEAD_SHAPE_SIZES:
        c = T.make_case(dims, n, s, "ordinary", T.SEED0 + 900 + n + s)
        ref = T.case_model(c)
        for mode in (0, 1, 2):
            for gram in (1, 0):
                with settings(L, mode, gram):
                    check(O, c, ref, run_head(L, h, c), mode, gram, "zero geo")
    report("zero geo")


# ------------------------------------------------------------------------------------------------ LDS bounds
def test_lds_bounds(api, O, heads):
    """s = 1500 at hidden 256 leaves the Gram form for the layer-wise one; the largest s of the Gram form at hidden 32; one sample over (7 s + 2 E) * 4 > 60 KiB
    returns NRF_ERR_UNSUPPORTED and writes nothing."""
    L, _ = api
    for dims, n, s in (T.LDS_LAYERWISE, T.LDS_GRAM):
        c = T.make_case(dims, n, s, "ordinary", T.SEED0 + 900 + n + s)
        ref = T.case_model(c)
        assert T.kink_census(c, ref).mean() <= T.MAX_KINK_SHARE
        for mode in (0, -1):
            with settings(L, mode, 1):
                check(O, c, ref, run_head(L, heads(dims), c), mode, 1, "LDS bounds")
    c = T.make_case(T.SMALL, 2, T.UNSUPPORTED_S, "ordinary", T.SEED0 + 990)
    with settings(L, -1, 1):
        run_head(L, heads(T.SMALL), c, expect=NRF_ERR_UNSUPPORTED)
    report("LDS bounds")


# ------------------------------------------------------------------------------------------------ several passes
@pytest.fixture(scope="module")
def pass_refs():
    """The float64 model of the three batches just over a pass cap, once."""
    out = {}
    for dims, n, s, gram in T.PASS_CASES:
        c = T.make_case(dims, n, s, "ordinary", T.SEED0 + 950 + n + s)
        out[(n, s)] = (c, T.case_model(c))
    return out


@pytest.mark.parametrize("case", T.PASS_CASES, ids=lambda p: f"{p[1]}x{p[2]}-gram{p[3]}")
def test_batches_cut_into_several_passes(api, O, heads, pass_refs, case):
    """Two and three passes layer-wise (cap 2^17 / s rays), two in the Gram form (2^20 / s), cut evenly: against the model of the WHOLE batch, and the rows of the last
    ray of each pass and of the first ray of the next one by one."""
    L, _ = api
    dims, n, s, gram = case
    c, ref = pass_refs[(n, s)]
    assert T.kink_census(c, ref).mean() <= T.MAX_KINK_SHARE
    d = T.dispatch(dims, n, s, -1, gram)
    assert d["passes"] >= 2 and d["gram"] == bool(gram)
    for mode in (0, -1):
        with settings(L, mode, gram):
            got = run_head(L, heads(dims), c)
            check(O, c, ref, got, mode, gram, "several passes")
        arith = effective_mode(c, mode, gram)
        eo = oracle_figures(O, c, ref)
        bar = {k: (BAR_VALUES[arith] if arith else max(ORACLE_FACTOR * eo[k], F32_FLOOR)) for k in ("weights_rel", "rendered_rel", "g_emb")}
        w, rd, ge = got["weights"].reshape(n, s), got["rendered"].reshape(n, -1), got["g_emb"].reshape(n, -1)
        for p in range(1, d["passes"]):
            for ray in (p * d["rays"] - 1, p * d["rays"]):          # the last ray of a pass, the first of the next: each row against the whole tensor's bar
                assert np.abs(w[ray] - ref["weights"][ray]).max() <= bar["weights_rel"] * np.abs(ref["weights"]).max(), ("weights", ray)
                assert np.abs(rd[ray] - ref["rendered"][ray]).max() <= bar["rendered_rel"] * np.abs(ref["rendered"]).max(), ("rendered", ray)
                rg = ref["g_emb"].reshape(n, -1)[ray]
                assert np.abs(rg).max() > 0 and np.abs(ge[ray] - rg).max() <= bar["g_emb"] * np.abs(rg).max(), ("g_emb", ray)
    report("several passes")


# ------------------------------------------------------------------------------------------------ one-hot rays
def one_hot_check(L, O, h, c, ray, mode, gram, group):
    """g_rendered zero except for `ray`: every other ray adds exact zeros, so the model of that ray ALONE is the reference of the whole call."""
    n, s, in_ch = c["n"], c["s"], c["dims"][0]
    hot = dict(c, g_rendered=np.where((np.arange(n) == ray)[:, None], c["g_rendered"], np.float32(0)).astype(np.float32))
    hot.pop("e_oracle", None)
    got = run_head(L, h, hot)
    a, b = ray * s, (ray + 1) * s
    one = dict(c, n=1, emb=c["emb"][a:b], keep=None if c["keep"] is None else c["keep"][a:b], z=c["z"][ray:ray + 1], d=c["d"][ray:ray + 1],
               noise=None if c["noise"] is None else c["noise"][ray:ray + 1], g_rendered=c["g_rendered"][ray:ray + 1], tag=c["tag"] + f" one-hot ray {ray}")
    one.pop("e_oracle", None)
    ref = T.case_model(one)
    ge = got["g_emb"].reshape(n, -1)
    others = np.arange(n) != ray
    assert not ge[others].any(), "a ray with a zero upstream gradient got a feature gradient"
    sub = dict(weights=got["weights"].reshape(n, s)[ray], rendered=got["rendered"].reshape(n, -1)[ray], g_emb=ge[ray], g_params=got["g_params"])
    # the arithmetic is the whole call's (its point count picks the products), the reference the one ray's
    arith = effective_mode(c, mode, gram)
    e = T.compare(one, ref, sub["weights"], sub["rendered"], sub["g_emb"], sub["g_params"])
    names = list(T.param_slices(c["dims"]))
    if arith == 0:
        eo = oracle_figures(O, one, ref)
        for k in ["weights_rel", "rendered_rel", "g_emb"] + names:
            bar = max(ORACLE_FACTOR * eo[k], F32_FLOOR)
            note(group, "fp32", k, e[k] / bar)
            assert e[k] <= bar, (one["tag"], mode, k, e[k], bar)
    else:
        for k in ("weights", "rendered", "g_emb"):
            note(group, ("bf16x3", "f16x3")[arith - 1], k, e[k])
            assert e[k] <= BAR_VALUES[arith], (one["tag"], mode, k, e[k])
        for k in names:
            note(group, ("bf16x3", "f16x3")[arith - 1], "params (norm-wise)", e[k + "_norm"])
            assert e[k + "_norm"] <= BAR_PARAM_NORM[arith], (one["tag"], mode, k, e[k + "_norm"])


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_one_hot_rays_first_and_last(api, O, heads, mode):
    """c >= 4096, rays >= 256: the first and the last ray's whole contribution to every dW stands alone; a dropped tail row cannot hide under a norm-wise bar."""
    L, _ = api
    dims, n, s = T.ONE_HOT
    c = T.make_case(dims, n, s, "opaque_at", T.SEED0 + 900 + n + s)
    for gram in (1, 0):
        for ray in (0, n - 1):
            with settings(L, mode, gram):
                one_hot_check(L, O, heads(dims), c, ray, mode, gram, "one-hot rays")
    report("one-hot rays")


@pytest.mark.parametrize("case", [T.PASS_CASES[0], T.PASS_CASES[2]], ids=lambda p: f"{p[1]}x{p[2]}-gram{p[3]}")
def test_one_hot_rays_either_side_of_a_pass_boundary(api, O, heads, pass_refs, case):
    L, _ = api
    dims, n, s, gram = case
    c, _ = pass_refs[(n, s)]
    rays = T.dispatch(dims, n, s, -1, gram)["rays"]
    for mode in (0, 1, 2, -1):
        for ray in (rays - 1, rays):
            with settings(L, mode, gram):
                one_hot_check(L, O, heads(dims), c, ray, mode, gram, "one-hot boundary")
    report("one-hot boundary")


# ------------------------------------------------------------------------------------------------ edges of the calling convention
@pytest.mark.parametrize("n,s", T.HEAD_SHAPE_SIZES)
def test_null_outputs_empty_call_and_accumulation(api, O, heads, n, s):
    """d_g_emb, d_rendered, d_weights null one at a time (the others unchanged); n = 0 returns OK and touches nothing; a prefilled d_g_params ends as prefill +
    gradient, to the bar of the mode."""
    L, _ = api
    c = T.make_case(T.SMALL, n, s, "opaque_at", T.SEED0 + 800 + n, keep_mode="null", d_stride=8)
    ref = T.case_model(c)
    h = heads(T.SMALL)
    for mode in (0, -1):
        for gram in (1, 0):
            with settings(L, mode, gram):
                for null in ("g_emb", "rendered", "weights"):
                    got = run_head(L, h, c, null=(null,))
                    assert got[null] is None
                    check(O, c, ref, got, mode, gram, "edges")
                run_head(L, h, c, n=0)
                # a prefill of each tensor's own size (draws clipped to +-4 of its largest entry), to the bar of the mode: the fp32 roundings of adding to it (at most two
                # accumulating products per tensor at |value| <= 5 x that entry, 10 * 2^-24 of it) are inside the bar's floor of 16 * 2^-24
                prefill = np.zeros(ref["g_params"].size, np.float32)
                draws = np.clip(np.random.default_rng(7).standard_normal(prefill.size), -4, 4)
                for k, (off, (o_, k_)) in T.param_slices(c["dims"]).items():
                    prefill[off:off + o_ * k_] = draws[off:off + o_ * k_] * np.abs(ref["g_params"][off:off + o_ * k_]).max()
                got = run_head(L, h, c, prefill=prefill)
                got["g_params"] = got["g_params"].astype(np.float64) - prefill.astype(np.float64)
                e = T.compare(c, ref, got["weights"], got["rendered"], got["g_emb"], got["g_params"])
                arith = effective_mode(c, mode, gram)
                for k in T.param_slices(c["dims"]):
                    bar = BAR_PARAM_NORM[arith] if arith else max(ORACLE_FACTOR * oracle_figures(O, c, ref)[k], F32_FLOOR)
                    v = e[k + "_norm"] if arith else e[k]
                    note("accumulation", ("fp32", "bf16x3", "f16x3")[arith], "params (norm-wise)" if arith else k, v / (1 if arith else bar))
                    assert v <= bar, (c["tag"], mode, gram, k, v, bar)
    report("edges"); report("accumulation")


# ------------------------------------------------------------------------------------------------ the Gram matrix after a parameter upload
def test_gram_matrix_after_a_parameter_upload(api, O):
    """Main.cpp head created with blob A, nrf_mlp_set_params with blob B on the device (the device packer forms W^T W, which the backward then copies) and from the
    host (the W^T W product of the call itself); the same case on a fresh handle of blob B.  All against the model of blob B: a stale Gram matrix is blob A's."""
    L, LeRF = api
    dims, n, s = T.UPLOAD
    mk = lambda blob: LeRF(dims[3], dims[1], dims[2], dims[4], dims[0], "lang_model", params=blob)
    A, B = T.net(dims, 0).blob, T.net(dims, 1).blob
    c = T.make_case(dims, n, s, "opaque_at", T.SEED0 + 900 + n + s, blob_seed=1)
    ref = T.case_model(c)
    assert T.kink_census(c, ref).mean() <= T.MAX_KINK_SHARE and T.dispatch(dims, n, s)["gram_from_packer"]
    stale = T.case_model(c, blob=np.concatenate([B[:-dims[4] * dims[2]], A[-dims[4] * dims[2]:]]))
    assert np.abs(stale["rendered"] - ref["rendered"]).max() > 1e-2, "the two last layers differ enough for a stale matrix to show"
    cA = T.make_case(dims, n, s, "opaque_at", T.SEED0 + 900 + n + s, blob_seed=0)
    refA = T.case_model(cA)
    assert T.kink_census(cA, refA).mean() <= T.MAX_KINK_SHARE
    lib = L.lib()

    def upload(h, blob, on_device):
        b = _dev(blob) if on_device else None
        L.check(lib.nrf_mlp_set_params(h._m, _p(b) if on_device else blob.ctypes.data_as(C.c_void_p), int(on_device), None))

    def backward(h, c, ref, modes=(0, -1)):
        for mode in modes:
            with settings(L, mode, 1):
                check(O, c, ref, run_head(L, h, c), mode, 1, "after an upload")

    h = mk(A)                                  # create runs the device packer to verify it: its matrix is blob A's (a fresh handle takes the packer's matrix too)
    assert lib.nrf_mlp_device_repack_images(h._m) == 3, "the handle's uploads stay on the device: the packer forms W^T W and the backward copies it"
    upload(h, B, on_device=False)              # host re-pack: no current matrix, the call forms W^T W itself; a stale one would be A's
    backward(h, c, ref)
    upload(h, A, on_device=True)
    upload(h, B, on_device=True)               # the device packer's matrix of blob B
    backward(h, c, ref)
    upload(h, A, on_device=False)              # ... which a host re-pack of blob A must not leave in use
    backward(h, cA, refA)
    backward(mk(B), c, ref)                    # a fresh handle
    report("after an upload")


# ------------------------------------------------------------------------------------------------ the language loss
def run_loss(L, pred, target, want_grad=True):
    n, e = pred.shape
    loss, grad = Guarded(4), Guarded(4 * n * e)
    p, t = _dev(pred), _dev(target)
    L.check(L.lib().nrf_huber_rows_nanmean(_p(p), _p(t), n, e, float(T.DELTA), loss.ptr(), grad.ptr() if want_grad else None, None))
    torch.cuda.synchronize()
    g = grad.host("the gradient")
    return float(loss.host("the loss")[0]), g.reshape(n, e)


@pytest.mark.parametrize("n", T.LOSS_N)
def test_language_loss(api, n):
    """nrf_huber_rows_nanmean at every row count either side of its 4 rows per block and of the 256-thread row loop, every width either side of the 64 lanes; |d| exactly
    at, just under and just over delta; no NaN row, one, NaN rows at the block edges (3, 4, 255, 256), every row NaN (loss NaN, and LibTorch's gradient is NaN throughout)."""
    L, _ = api
    for e in T.LOSS_E:
        for nan in ("none", "one", "edges", "all"):
            pred, target, rows = T.loss_case(n, e, nan)
            loss, grad = run_loss(L, pred, target)
            check_loss(pred, target, loss, grad)
            if nan == "none":
                l2, g2 = run_loss(L, pred, target, want_grad=False)
                assert l2 == loss and np.isnan(g2).all(), "d_grad = NULL: the same loss, nothing written"


# ------------------------------------------------------------------------------------------------ the points entry over a pass boundary
def test_backward_points_over_a_pass_boundary_equals_the_composed_stages(api):
    """nrf_lerf_backward_points with n just over a pass cap (2049 rays x 64 samples, layer-wise: two passes) against the same stages composed on the device over the
    whole batch: nrf_hash_encode -> nrf_lerf_head_backward -> nrf_hash_backward_rays.  Float atomics in another order: 2e-6 * max|ref|."""
    L, _ = api
    from nerfpp_amd import scene as S
    lib = L.lib()
    sc = S.make_lerf_scene(log2_t=14, sigma_scale=20.0)
    r, emb_h, head = sc["renderer"], sc["embedder"], sc["lerf"]
    n, s, E = 2049, 64, 768
    rng = np.random.default_rng(5)
    bb = sc["bbox"]
    o = rng.uniform(bb[:3] * 0.3, bb[3:] * 0.3, (n, 3)).astype(np.float32)
    d = PR._dirs(rng, n)
    z = np.sort(rng.uniform(0.0, 1.5, (n, s)).astype(np.float32), axis=1)
    pts = (o[:, None, :] + d[:, None, :] * z[..., None]).astype(np.float32).reshape(-1, 3)
    g_r = (rng.standard_normal((n, E)) * 1e-2).astype(np.float32)
    dp, dz, dd, dg = _dev(pts), _dev(z), _dev(d), _dev(g_r)
    nparams, ntable = int(head.n_params), int(emb_h.table_elems())
    with settings(L, -1, 0):
        assert T.dispatch(T.MAIN, n, s, -1, 0)["passes"] == 2
        gp1, gt1 = torch.zeros(nparams, device="cuda"), torch.zeros(ntable, device="cuda")
        nb = int(lib.nrf_lerf_backward_points_workspace_bytes(r._r, n, s))
        ws = Guarded(nb)
        L.check(lib.nrf_lerf_backward_points(r._r, _p(dp), _p(dz), _p(dd), 3, n, s, None, 0.0, _p(dg), _p(gp1), _p(gt1), ws.ptr(), nb, None))
        torch.cuda.synchronize()
        ws.host("the workspace of nrf_lerf_backward_points")
        feats = torch.empty((n * s, 128), device="cuda")
        keep = torch.empty((n * s,), dtype=torch.uint8, device="cuda")
        L.check(lib.nrf_hash_encode(emb_h._h, _p(dp), n * s, _p(feats), _p(keep), None))
        gp2, gt2, ge = torch.zeros(nparams, device="cuda"), torch.zeros(ntable, device="cuda"), torch.empty((n * s, 128), device="cuda")
        nb2 = int(lib.nrf_lerf_head_backward_workspace_bytes(head._m, n, s))
        ws2 = Guarded(nb2)
        L.check(lib.nrf_lerf_head_backward(head._m, _p(feats), _p(keep), _p(dz), _p(dd), 3, n, s, None, 0.0, _p(dg), _p(gp2), _p(ge), None, None, ws2.ptr(), nb2, None))
        L.check(lib.nrf_hash_backward_rays(emb_h._h, _p(dp), n, s, _p(ge), _p(gt2), None))
        torch.cuda.synchronize()
        ws2.host("the workspace of nrf_lerf_head_backward")
    for what, a, b in (("head gradients", gp1, gp2), ("table gradients", gt1, gt2)):
        a, b = a.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64)
        assert np.abs(b).max() > 0 and np.isfinite(a).all()
        err = np.abs(a - b).max() / np.abs(b).max()
        print(f"MEASURED points entry     f16x3   {what:20s} {err:.3e}")
        assert err <= BAR_ATOMICS_ORDER, (what, err)

