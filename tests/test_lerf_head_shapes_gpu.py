"""The LeRF head's matrix-core passes on the MI355X at every size they dispatch (mlp_lerf_mfma.hip, mlp_lerf_split_mfma.hip, sigma_lerf_f32.hip) against the float64
model of tests/lerf_head_ref.py: both forms of kernel A, the three of kernel B, the two of kernel C and the exact-fp32 density kernel, through the C entries.

On the INTEGER network (tests/test_lerf_head_shapes_host.py proves the conditions) sigma and the geo planes are compared bit for bit and the ray sums against bars
derived element-wise from the roundings that remain; on the random network of the existing stage tests the project's bars of those tests hold.  Sizes: ragged point and
ray counts, several tiles per ray, the second and third iteration of every persistent loop, strided tables with guard columns, merge maps with repeats."""
import ctypes as C

import numpy as np
import pytest
import torch

import lerf_head_ref as H

pytestmark = pytest.mark.gpu

PRECS = ["f16", "split"]
EPS = {"f16": 2.0 ** -11, "split": 2.0 ** -22}          # what kernel C's operand keeps of asum: one fp16 rounding / a (hi, lo) pair
# Integer network: |got - ref| <= C_SUM * EPS * (|W| @ sum_s |f_s a_s|) element-wise.  The roundings left are those of fp32 (sqrt, division, the sums) and EPS; the
# constants are 2 x the worst ratio measured over all integer cases against the float64 projection form (the margin covers summation order):
C_SUM = {"f16": 0.38, "split": 0.35}                    # measured worst 0.189 (f16), 0.175 (split): profiles/lerf_head_shapes/measured_errors.txt
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from nerfpp_amd import _lib as L
    from nerfpp_amd.modules import LeRF
    return L, LeRF


@pytest.fixture(scope="module")
def nets(api, manifest):
    """kind -> (Net, LeRF handle): the integer network, the random one on fp16 features and on fp32 features that are not fp16 numbers (same handle)."""
    L, LeRF = api
    blob = H.random_blob(manifest)
    inet, rnet, xnet = H.integer_net(), H.Net("rand", blob, H.random_pool_f16()), H.Net("rand", blob, H.random_pool_f32())
    mk = lambda b: LeRF(32, 2, 256, 768, 128, "lang_model", params=b)
    hi, hr = mk(inet.blob), mk(blob)
    assert L.lib().nrf_lerf_mfma_available(hi._m) and L.lib().nrf_lerf_sigma_exact_available(hi._m)
    return {"int": (inet, hi), "rand": (rnet, hr), "xlo": (xnet, hr)}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    """fp32 bit patterns, the sign of zero aside."""
    return (np.ascontiguousarray(a, np.float32) + np.float32(0)).view(np.uint32)


def _set(L, h, prec):
    L.check(L.lib().nrf_lerf_set_precision(h._m, L.NRF_PREC_F16_MFMA if prec == "f16" else L.NRF_PREC_F16_SPLIT))


def _sentinel(nbytes):
    return torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")


# ------------------------------------------------------------------------------------------------ density entries
GUARD = 16


def _sigma(L, h, entry, x_rows, keep, want_geo=False, rc_only=False):
    """One density entry on rows x_rows [p, 128] -> (sigma [p], geo bytes or None, geo_stride); sigma and every geo plane have guard columns of sentinel bytes behind them,
    checked here.  entry: rows | lm | lm_strided | geo | exact."""
    lib = L.lib()
    p = x_rows.shape[0]
    pstride = p + H.PSTRIDE_PAD if entry in ("lm_strided", "geo", "exact") else p
    gs = p + H.GEO_STRIDE_PAD
    sig = _sentinel(4 * (p + GUARD))
    kd = _dev(keep) if keep is not None else None
    geo = _sentinel(int(lib.nrf_lerf_geo_bytes(C.c_int64(gs)))) if want_geo else None
    if entry == "rows":
        x = _dev(x_rows)
        rc = lib.nrf_lerf_sigma(h._m, _p(x), _p(kd), p, _p(sig), None)
    else:
        x = _dev(H.to_level_major(x_rows, pstride))
        if entry == "lm":
            rc = lib.nrf_lerf_sigma_lm(h._m, _p(x), _p(kd), p, _p(sig), None)
        elif entry == "lm_strided":
            rc = lib.nrf_lerf_sigma_lm_strided(h._m, _p(x), pstride, _p(kd), p, _p(sig), None)
        elif entry == "geo":
            rc = lib.nrf_lerf_sigma_geo_lm_strided(h._m, _p(x), pstride, _p(kd), p, _p(sig), _p(geo), gs, None)
        else:
            rc = lib.nrf_lerf_sigma_exact_lm_strided(h._m, _p(x), pstride, _p(kd), p, _p(sig), _p(geo), gs if want_geo else 0, None)
    L.check(rc)
    s = _host(sig)
    assert (s[4 * p:] == SENTINEL).all(), f"{entry}: wrote behind sigma[{p}]"
    g = None
    if want_geo:
        g = _host(geo)
        assert (g.reshape(6, gs, 32)[:, p:, :] == SENTINEL).all(), f"{entry}: wrote behind column {p} of a geo plane"
    return s[:4 * p].view(np.float32).copy(), g, gs


def _sigma_entries(prec):
    return ["rows", "lm", "lm_strided"] + (["geo"] if prec == "split" else [])


def _check_integer_density(L, net, h, p, precs=PRECS, exact=True):
    c = H.density_case(net, p)
    m = net.model
    x = net.pool[c["idx"]]
    unmasked = m["sigma"][c["idx"]]
    ref = _bits(np.where(c["keep"] == 1, unmasked, 0.0))
    planes = np.concatenate([unmasked[:, None], m["geo"][c["idx"]], np.zeros((p, 15))], axis=1)          # rows 0..47 of the chained operand

    def check_planes(g, gs, what):
        hi, lo = H.decode_geo(g[:192 * gs].reshape(6, gs, 32)[:, :p, :].copy().reshape(-1), p)
        assert np.array_equal(hi, planes), f"{what}: hi planes != [sigma (unmasked), geo, zeros]"
        assert (lo == 0).all(), f"{what}: lo planes of integers must be zero"

    for prec in precs:
        _set(L, h, prec)
        for entry in _sigma_entries(prec):
            sig, g, gs = _sigma(L, h, entry, x, c["keep"], want_geo=entry == "geo")
            assert np.array_equal(_bits(sig), ref), f"p {p} {prec} {entry}: sigma differs from the float64 model in {(_bits(sig) != ref).sum()} of {p} points"
            if g is not None:
                check_planes(g, gs, f"p {p} {prec} {entry}")
        if p <= 513:
            sig, _, _ = _sigma(L, h, "lm", x, None)
            assert np.array_equal(_bits(sig), _bits(unmasked)), f"p {p} {prec}: sigma without a keep mask"
    if exact:
        for want_geo in (False, True):
            sig, g, gs = _sigma(L, h, "exact", x, c["keep"], want_geo=want_geo)
            assert np.array_equal(_bits(sig), ref), f"p {p} exact (geo {want_geo}): sigma differs from the float64 model"
            if g is not None:
                check_planes(g, gs, f"p {p} exact")


@pytest.mark.parametrize("p", H.DENSITY_SMALL)
def test_integer_sigma_and_geo_planes_bit_for_bit(api, nets, p):
    _check_integer_density(api[0], *nets["int"], p)


def test_integer_sigma_third_persistent_iteration_split(api, nets):
    _check_integer_density(api[0], *nets["int"], H.DENSITY_SPLIT_PERSISTENT, precs=["split"], exact=False)


def test_integer_sigma_third_persistent_iteration_f16(api, nets):
    _check_integer_density(api[0], *nets["int"], H.DENSITY_F16_PERSISTENT, precs=["f16"], exact=False)


def test_integer_sigma_second_persistent_iteration_exact(api, nets):
    _check_integer_density(api[0], *nets["int"], H.DENSITY_EXACT_PERSISTENT, precs=[], exact=True)


def _check_random_density(L, net, h, p, precs, entries=None, exact=False):
    from oracle import capi as O
    c = H.density_case(net, p)
    m = net.model
    x = net.pool[c["idx"]]
    unmasked = m["sigma"][c["idx"]]
    ref = np.where(c["keep"] == 1, unmasked, 0.0)
    scale = np.abs(ref).max() if p > 1 else np.abs(m["sigma"]).max()
    geo_ref = np.concatenate([unmasked[:, None], m["geo"][c["idx"]], np.zeros((p, 15))], axis=1)
    gscale = np.maximum(np.abs(np.concatenate([m["sigma"][:, None], m["geo"]], axis=1)).max(0), 1e-30)

    def check_planes(g, gs, what):
        hi, lo = H.decode_geo(g[:192 * gs].reshape(6, gs, 32)[:, :p, :].copy().reshape(-1), p)
        err = (np.abs(hi + lo - geo_ref)[:, :33] / gscale).max()
        print(f"{what}: geo planes hi + lo, worst error {err:.3e} of a row's scale")
        assert err <= H.BAR_GEO_PLANES and (hi[:, 33:] == 0).all() and (lo[:, 33:] == 0).all()

    for prec in precs:
        _set(L, h, prec)
        same = None
        for entry in entries or _sigma_entries(prec):
            sig, g, gs = _sigma(L, h, entry, x, c["keep"], want_geo=entry == "geo")
            err = np.abs(sig - ref).max() / scale
            print(f"random p {p} {prec} {entry}: sigma worst error {err:.3e} of max|sigma| (bar {H.BAR_SIGMA[prec]:.0e})")
            assert err <= H.BAR_SIGMA[prec]
            assert (sig[c["keep"] == 0] == 0).all()
            if net.pool is nets_f16_pool(net):
                assert same is None or np.array_equal(_bits(sig), same), f"random p {p} {prec} {entry}: the entries run the same arithmetic on the same fp16 features"
                same = _bits(sig)
            if g is not None:
                check_planes(g, gs, f"random p {p} {prec} {entry}")
    if exact:
        rows = np.arange(p) if p <= 2048 else np.unique(np.concatenate([np.arange(600), np.arange(p - 600, p), np.arange(0, p, 37)]))
        oracle = O.lerf_sigma_net(net.blob, x[rows])
        for want_geo in (False, True):
            sig, g, gs = _sigma(L, h, "exact", x, c["keep"], want_geo=want_geo)
            want = np.where(c["keep"][rows] == 1, oracle[:, 0], np.float32(0))
            assert np.array_equal(_bits(sig[rows]), _bits(want)), f"random p {p}: exact sigma != the oracle's fp32 chain"
            assert (sig[c["keep"] == 0] == 0).all() and np.abs(sig - ref).max() <= H.BAR_SIGMA["split"] * scale
            if g is not None:
                check_planes(g, gs, f"random p {p} exact")


def nets_f16_pool(net):
    """The pool itself if its features are fp16 numbers (then level-major and row-major inputs carry the same values), else None."""
    return net.pool if np.array_equal(net.pool.astype(np.float16).astype(np.float32), net.pool) else None


@pytest.mark.parametrize("p", H.DENSITY_SMALL)
def test_random_sigma_within_the_project_bars_and_exact_equals_oracle(api, nets, p):
    _check_random_density(api[0], *nets["rand"], p, PRECS, exact=True)


def test_random_sigma_persistent_iterations(api, nets):
    L = api[0]
    _check_random_density(L, *nets["rand"], H.DENSITY_SPLIT_PERSISTENT, ["split"], entries=["lm_strided", "geo"])
    _check_random_density(L, *nets["rand"], H.DENSITY_F16_PERSISTENT, ["f16"], entries=["lm_strided"])
    _check_random_density(L, *nets["rand"], H.DENSITY_EXACT_PERSISTENT, [], exact=True)


@pytest.mark.parametrize("p", H.DENSITY_XLO)
def test_random_sigma_from_fp32_rows_that_are_not_fp16(api, nets, p):
    _check_random_density(api[0], *nets["xlo"], p, PRECS, entries=["rows"])


# ------------------------------------------------------------------------------------------------ ray-sum entries
class RayInputs:
    """Device inputs of one ray case, built once and shared by the entries."""

    def __init__(self, net, c):
        self.c, self.net = c, net
        self.rows = net.pool[c["idx"]]
        self.w = _dev(c["w"])
        self.src = _dev(c["src"])
        self.table_rows = net.pool[c["col_idx"]]
        self._cache = {}

    def get(self, name):
        if name not in self._cache:
            self._cache[name] = _dev({"rows": lambda: self.rows, "lm": lambda: H.to_level_major(self.rows), "table": lambda: H.to_level_major(self.table_rows),
                                      "identity": lambda: np.arange(self.c["n"] * self.c["s"], dtype=np.int32)}[name]())
        return self._cache[name]


def _embed(L, h, entry, ri, geo=None, n=None):
    """One ray-sum entry -> out [n, 768]; out is pre-filled with NaN.  entry: rows | lm | gather | gather_identity | geo.  n: the first n rays only."""
    lib, c = L.lib(), ri.c
    n, s = c["n"] if n is None else n, c["s"]
    out = torch.full((n, H.EMB), float("nan"), device="cuda")
    if entry == "rows":
        rc = lib.nrf_lerf_render_embedding(h._m, _p(ri.get("rows")), _p(ri.w), n, s, _p(out), None)
    elif entry == "lm":
        assert n == c["n"]
        rc = lib.nrf_lerf_render_embedding_lm(h._m, _p(ri.get("lm")), _p(ri.w), n, s, _p(out), None)
    elif entry == "gather_identity":
        rc = lib.nrf_lerf_render_embedding_lm_gather(h._m, _p(ri.get("lm")), c["n"] * s, _p(ri.get("identity")), _p(ri.w), n, s, _p(out), None)
    elif entry == "gather":
        rc = lib.nrf_lerf_render_embedding_lm_gather(h._m, _p(ri.get("table")), c["cols"], _p(ri.src), _p(ri.w), n, s, _p(out), None)
    else:
        rc = lib.nrf_lerf_render_embedding_lm_geo(h._m, _p(ri.get("table")), c["cols"], _p(ri.src), _p(geo), c["cols"], _p(ri.w), n, s, _p(out), None)
    L.check(rc)
    return _host(out)


def _geo_planes(L, h, ri, producer):
    """The geo planes over all columns of the case's table, from kernel A in split precision or from the exact kernel."""
    lib, cols = L.lib(), ri.c["cols"]
    geo = _sentinel(int(lib.nrf_lerf_geo_bytes(C.c_int64(cols))))
    sig = torch.empty((cols,), device="cuda")
    fn = lib.nrf_lerf_sigma_geo_lm_strided if producer == "split" else lib.nrf_lerf_sigma_exact_lm_strided
    L.check(fn(h._m, _p(ri.get("table")), cols, None, cols, _p(sig), _p(geo), cols, None))
    return geo


def _ray_entries(prec, n, s):
    e = ["rows", "lm", "gather"]
    return e + ["geo:split", "geo:exact"] if prec == "split" else e


def _run_entry(L, h, name, ri):
    if name.startswith("geo:"):
        return _embed(L, h, "geo", ri, geo=_geo_planes(L, h, ri, name[4:]))
    return _embed(L, h, name, ri)


RATIOS = {}          # (kind, precision) -> worst measured ratio / error, printed by every case


def _check_integer_rays(L, net, h, n, s, precs=PRECS, entries=None):
    c = H.ray_case(net, n, s)
    ri = RayInputs(net, c)
    ref, bound = net.render(c["idx"], c["w"])
    for prec in precs:
        _set(L, h, prec)
        for name in entries or _ray_entries(prec, n, s):
            out = _run_entry(L, h, name, ri).astype(np.float64)
            assert np.isfinite(out).all(), f"({n}, {s}) {prec} {name}: {np.isnan(out).any(1).sum()} rows not written"
            err = np.abs(out - ref)
            live = bound > 0
            ratio = (err[live] / (EPS[prec] * bound[live])).max()
            RATIOS[("int", prec)] = max(RATIOS.get(("int", prec), 0.0), ratio)
            print(f"integer ({n}, {s}) {prec} {name}: worst |got - ref| / (eps bound) = {ratio:.3f} (c = {C_SUM[prec]}); worst so far {RATIOS[('int', prec)]:.3f}")
            assert (out[~live] == 0).all(), f"({n}, {s}) {prec} {name}: a ray of dead samples or of zero weights must give exact zeros"
            bad = np.argwhere(err > C_SUM[prec] * EPS[prec] * bound)
            assert bad.size == 0, f"({n}, {s}) {prec} {name}: {len(bad)} elements over the bound, first (ray, o) = {bad[0]}, rays {np.unique(bad[:, 0])[:8]}"
        if prec == "split":
            a, b = _embed(L, h, "lm", ri), _embed(L, h, "gather_identity", ri)
            assert np.array_equal(_bits(a), _bits(b)), "the identity merge map changes nothing (split)"


@pytest.mark.parametrize("n,s", H.RAY_SMALL + H.RAY_KERNEL_C_EDGES)
def test_integer_ray_sums_within_the_derived_bound(api, nets, n, s):
    _check_integer_rays(api[0], *nets["int"], n, s)


@pytest.mark.parametrize("n,s", H.RAY_SPLIT_PERSISTENT)
def test_integer_ray_sums_second_persistent_iteration_split(api, nets, n, s):
    _check_integer_rays(api[0], *nets["int"], n, s, precs=["split"])


@pytest.mark.parametrize("n,s", H.RAY_F16_PERSISTENT)
def test_integer_ray_sums_persistent_iterations_f16(api, nets, n, s):
    _check_integer_rays(api[0], *nets["int"], n, s, precs=["f16"], entries=["lm", "gather"])


def _check_random_rays(L, net, h, n, s, precs=PRECS, entries=None, tag="random"):
    c = H.ray_case(net, n, s)
    ri = RayInputs(net, c)
    ref, _ = net.render(c["idx"], c["w"])
    scale = np.abs(ref).max()
    nz = np.abs(ref).max(1) > 0
    unit = lambda a: a / np.linalg.norm(a, axis=1, keepdims=True)
    worst = {}
    for prec in precs:
        _set(L, h, prec)
        for name in entries or _ray_entries(prec, n, s):
            out = _run_entry(L, h, name, ri).astype(np.float64)
            assert np.isfinite(out).all(), f"({n}, {s}) {prec} {name}: rows not written"
            err = np.abs(out - ref).max() / scale
            msg = f"{tag} ({n}, {s}) {prec} {name}: ray sums worst error {err:.3e} of max|ref| (bar {H.BAR_SUM[prec]:.0e})"
            assert (out[~nz] == 0).all(), "a ray of zero weights gives exact zeros"
            derr = None
            if prec == "split":
                derr = np.abs(unit(out[nz]) - unit(ref[nz])).max()
                msg += f", direction {derr:.3e} (bar {H.BAR_DIRECTION_SPLIT:.0e})"
            print(msg)
            worst[(prec, name)] = (err, derr)
            assert err <= H.BAR_SUM[prec], msg
            assert derr is None or derr <= H.BAR_DIRECTION_SPLIT, msg
        if nets_f16_pool(net) is not None:
            a, b = _embed(L, h, "lm", ri), _embed(L, h, "gather_identity", ri)
            if prec == "split" or s == 32:
                assert np.array_equal(_bits(a), _bits(b)), f"({n}, {s}) {prec}: the identity merge map changes nothing"
            else:
                assert np.abs(a - b).max() <= H.BAR_ATOMICS_ORDER * scale
    return worst


@pytest.mark.parametrize("n,s", H.RAY_SMALL + H.RAY_KERNEL_C_EDGES)
def test_random_ray_sums_within_the_project_bars(api, nets, n, s):
    _check_random_rays(api[0], *nets["rand"], n, s)


@pytest.mark.parametrize("n,s", H.RAY_SPLIT_PERSISTENT)
def test_random_ray_sums_second_persistent_iteration_split(api, nets, n, s):
    _check_random_rays(api[0], *nets["rand"], n, s, precs=["split"])


@pytest.mark.parametrize("n,s", H.RAY_F16_PERSISTENT)
def test_random_ray_sums_persistent_iterations_f16(api, nets, n, s):
    _check_random_rays(api[0], *nets["rand"], n, s, precs=["f16"], entries=["lm", "gather"])


@pytest.mark.parametrize("n,s", H.RAY_XLO)
def test_random_ray_sums_from_fp32_rows_that_are_not_fp16(api, nets, n, s):
    _check_random_rays(api[0], *nets["xlo"], n, s, entries=["rows"], tag="random fp32 rows")


# ------------------------------------------------------------------------------------------------ batch independence, stale scratch, determinism
@pytest.mark.parametrize("kind", ["int", "rand"])
def test_rows_do_not_depend_on_the_batch_or_on_stale_scratch(api, nets, kind):
    """Split precision has no atomics: a ray's row is a function of the ray alone.  The large call leaves its sums in the scratch pool; the five-ray call that follows
    takes the same scratch without a zero fill, and one wave of its second workgroup is dead (5 = 4 + 1)."""
    L = api[0]
    net, h = nets[kind]
    ri = RayInputs(net, H.ray_case(net, 1027, 64))
    _set(L, h, "split")
    geo = _geo_planes(L, h, ri, "exact")
    for entry, g in (("rows", None), ("gather", None), ("geo", geo)):
        big = _embed(L, h, entry, ri, geo=g)
        small = _embed(L, h, entry, ri, geo=g, n=5)
        again = _embed(L, h, entry, ri, geo=g)
        assert np.isfinite(small).all()
        assert np.array_equal(_bits(small), _bits(big[:5])), f"{kind} {entry}: the first five rays alone != the first five of 1027"
        assert np.array_equal(_bits(again), _bits(big)), f"{kind} {entry}: two runs of the same call differ"
    _set(L, h, "f16")
    ref, _ = net.render(ri.c["idx"], ri.c["w"])
    big, small = _embed(L, h, "gather", ri), _embed(L, h, "gather", ri, n=5)
    assert np.abs(small - big[:5]).max() <= H.BAR_ATOMICS_ORDER * np.abs(ref).max()
    r32 = RayInputs(net, H.ray_case(net, 1027, 32))          # one tile per ray: one add per element onto the zero fill
    big, small, again = _embed(L, h, "gather", r32), _embed(L, h, "gather", r32, n=5), _embed(L, h, "gather", r32)
    assert np.array_equal(_bits(small), _bits(big[:5])) and np.array_equal(_bits(again), _bits(big)), f"{kind}: fp16, s = 32"


# ------------------------------------------------------------------------------------------------ the LE1 scale
@pytest.mark.parametrize("k", H.LE1_SCALE_EXPONENTS)
def test_ray_sums_do_not_depend_on_the_scale_of_le1(api, nets, k):
    """out is invariant to the scale of LE1 (W a / ||W a||); the Gram matrix scales with its square, and the image holds it, LE1 and the ray's sum in fp16 pairs.
    With the Gram matrix only ever scaled down and LE1 stored as it came, 2^-8 missed the split bars (1.2e-4 of max|ref|, direction 1.2e-5): the packers now scale both
    (mlp_lerf_mfma.hip: lerf_gram_exponent, lerf_le1_exponent), and every k gives the figures of k = 0."""
    L, LeRF = api
    net = nets["rand"][0].with_le1_scaled(k)
    h = LeRF(32, 2, 256, 768, 128, "lang_model", params=net.blob)
    n, s = H.RAY_LE1_SCALE
    _check_random_rays(L, net, h, n, s, tag=f"LE1 x 2^{k}")


# ------------------------------------------------------------------------------------------------ parameter upload
def test_parameter_upload_from_device_memory(api, nets, manifest):
    """A handle created with the random blob, then nrf_mlp_set_params of the integer blob from device memory (k_lerf_gram_f64, k_lerf_gram_finish, k_lerf_fill and the
    exact kernel's image): the integer cases pass unchanged."""
    L, LeRF = api
    inet = nets["int"][0]
    h = LeRF(32, 2, 256, 768, 128, "lang_model", params=H.random_blob(manifest))
    blob = _dev(inet.blob)
    L.check(L.lib().nrf_mlp_set_params(h._m, _p(blob), 1, None))
    torch.cuda.synchronize()
    _check_integer_rays(L, inet, h, *H.RAY_UPLOAD)
    _check_integer_density(L, inet, h, H.DENSITY_UPLOAD)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_untouched(api, nets):
    L = api[0]
    lib = L.lib()
    net, h = nets["int"]
    p, n, s = 64, 2, 32
    x_rows = _dev(net.pool[1:1 + p + 1])
    lm = _dev(H.to_level_major(net.pool[1:1 + p], p + 8))
    w = _dev(np.ones((n, 48), np.float32))
    src = _dev(np.arange(p, dtype=np.int32))
    sig, out = _sentinel(4 * p), _sentinel(4 * n * H.EMB)
    geo = _sentinel(int(lib.nrf_lerf_geo_bytes(C.c_int64(p + 8))))
    off = lambda t, b: C.c_void_p(t.data_ptr() + b)
    _set(L, h, "split")
    refused = {
        "s = 48 (rows)": lambda: lib.nrf_lerf_render_embedding(h._m, _p(x_rows), _p(w), n, 48, _p(out), None),
        "s = 48 (lm)": lambda: lib.nrf_lerf_render_embedding_lm(h._m, _p(lm), _p(w), 1, 48, _p(out), None),
        "s = 48 (gather)": lambda: lib.nrf_lerf_render_embedding_lm_gather(h._m, _p(lm), p + 8, _p(src), _p(w), 1, 48, _p(out), None),
        "s = 48 (geo)": lambda: lib.nrf_lerf_render_embedding_lm_geo(h._m, _p(lm), p + 8, _p(src), _p(geo), p + 8, _p(w), 1, 48, _p(out), None),
        "pstride < p": lambda: lib.nrf_lerf_sigma_lm_strided(h._m, _p(lm), p - 1, None, p, _p(sig), None),
        "pstride < p (geo)": lambda: lib.nrf_lerf_sigma_geo_lm_strided(h._m, _p(lm), p - 1, None, p, _p(sig), _p(geo), p + 8, None),
        "pstride < p (exact)": lambda: lib.nrf_lerf_sigma_exact_lm_strided(h._m, _p(lm), p - 1, None, p, _p(sig), None, 0, None),
        "pstride < n s (lm, no map)": lambda: lib.nrf_lerf_render_embedding_lm_gather(h._m, _p(lm), p - 1, None, _p(w), n, s, _p(out), None),
        "geo_stride < p": lambda: lib.nrf_lerf_sigma_geo_lm_strided(h._m, _p(lm), p + 8, None, p, _p(sig), _p(geo), p - 1, None),
        "geo_stride < p (exact)": lambda: lib.nrf_lerf_sigma_exact_lm_strided(h._m, _p(lm), p + 8, None, p, _p(sig), _p(geo), p - 1, None),
        "misaligned rows (sigma)": lambda: lib.nrf_lerf_sigma(h._m, off(x_rows, 4), None, p, _p(sig), None),
        "misaligned rows (embedding)": lambda: lib.nrf_lerf_render_embedding(h._m, off(x_rows, 4), _p(w), n, s, _p(out), None),
        "misaligned features (lm)": lambda: lib.nrf_lerf_sigma_lm_strided(h._m, off(lm, 8), p + 7, None, p, _p(sig), None),
        "misaligned features (gather)": lambda: lib.nrf_lerf_render_embedding_lm_gather(h._m, off(lm, 8), p + 7, _p(src), _p(w), n, s, _p(out), None),
        "misaligned features (exact)": lambda: lib.nrf_lerf_sigma_exact_lm_strided(h._m, off(lm, 8), p + 7, None, p, _p(sig), None, 0, None),
        "misaligned geo": lambda: lib.nrf_lerf_sigma_geo_lm_strided(h._m, _p(lm), p + 8, None, p, _p(sig), off(geo, 8), p + 7, None),
    }
    for what, call in refused.items():
        assert call() != 0, f"{what}: accepted"
    _set(L, h, "f16")
    assert lib.nrf_lerf_sigma_geo_lm_strided(h._m, _p(lm), p + 8, None, p, _p(sig), _p(geo), p + 8, None) != 0, "the geo hand-over is split precision's"
    assert lib.nrf_lerf_render_embedding_lm_geo(h._m, _p(lm), p + 8, _p(src), _p(geo), p + 8, _p(w), n, s, _p(out), None) != 0
    for prec in PRECS:
        _set(L, h, prec)
        empty = {
            "p = 0 (rows)": lambda: lib.nrf_lerf_sigma(h._m, _p(x_rows), None, 0, _p(sig), None),
            "p = 0 (lm)": lambda: lib.nrf_lerf_sigma_lm(h._m, _p(lm), None, 0, _p(sig), None),
            "p = 0 (strided)": lambda: lib.nrf_lerf_sigma_lm_strided(h._m, _p(lm), p + 8, None, 0, _p(sig), None),
            "p = 0 (exact)": lambda: lib.nrf_lerf_sigma_exact_lm_strided(h._m, _p(lm), p + 8, None, 0, _p(sig), _p(geo), p + 8, None),
            "n = 0 (rows)": lambda: lib.nrf_lerf_render_embedding(h._m, _p(x_rows), _p(w), 0, s, _p(out), None),
            "n = 0 (lm)": lambda: lib.nrf_lerf_render_embedding_lm(h._m, _p(lm), _p(w), 0, s, _p(out), None),
            "n = 0 (gather)": lambda: lib.nrf_lerf_render_embedding_lm_gather(h._m, _p(lm), p + 8, _p(src), _p(w), 0, s, _p(out), None),
        }
        if prec == "split":
            empty["p = 0 (geo)"] = lambda: lib.nrf_lerf_sigma_geo_lm_strided(h._m, _p(lm), p + 8, None, 0, _p(sig), _p(geo), p + 8, None)
            empty["n = 0 (geo)"] = lambda: lib.nrf_lerf_render_embedding_lm_geo(h._m, _p(lm), p + 8, _p(src), _p(geo), p + 8, _p(w), 0, s, _p(out), None)
        for what, call in empty.items():
            assert call() == 0, f"{what} {prec}: {lib.nrf_last_error().decode()}"
    for name, t in (("sigma", sig), ("out", out), ("geo", geo)):
        assert (_host(t) == SENTINEL).all(), f"a refused or empty call wrote to {name}"
