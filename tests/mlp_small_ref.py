"""Cases and the float64 yardstick of the NeRFSmall shape tests (tests/test_mlp_small_shapes_host.py pins the C oracle against it on the CPU,
tests/test_mlp_small_shapes_gpu.py and tests/test_mlp_small_bwd_shapes_gpu.py run the kernels on the same cases).

A shape is (V, NL, NLC, G): input_ch_views, num_layers, num_layers_color, geo_feat_dim; input_ch = 32 and both hidden widths = 64 throughout -- the family
small_mfma_supported() (nerfpp_amd/csrc/mlp_small_mfma.hip) admits onto the matrix cores.  The parameter blob is scene.small_shapes' order: the sigma net's
layers, then the colour net's, each W [out][in] row-major, no biases."""
import itertools

import numpy as np

from nerfpp_amd import scene as S

IN_CH, HIDDEN = 32, 64
VIEWS, SIGMA_LAYERS, COLOUR_LAYERS, GEOS = (16, 64), (2, 3), (2, 3, 4), (0, 1, 7, 14, 15)
SHAPES = list(itertools.product(VIEWS, SIGMA_LAYERS, COLOUR_LAYERS, GEOS))          # 60
INSTANTIATIONS = list(itertools.product(VIEWS, SIGMA_LAYERS, COLOUR_LAYERS))        # the twelve NRF_CASE(V / 16, NL, NLC) of dispatch_small()
BWD_REFUSED = [(64, 3, 4, 15), (16, 3, 2, 15), (16, 3, 4, 7)]                        # outside bwd_supported() (mlp_small_bwd_mfma.hip): views 16, geo 15, NLC 3 or 4


def shape_id(shape):
    return "v%d-nl%d-nlc%d-g%d" % tuple(shape)


def layer_dims(shape):
    """-> [(in, out)] in blob order"""
    v, nl, nlc, g = shape
    return ([(IN_CH if l == 0 else HIDDEN, 1 + g if l == nl - 1 else HIDDEN) for l in range(nl)] +
            [(v + g if l == 0 else HIDDEN, 3 if l == nlc - 1 else HIDDEN) for l in range(nlc)])


def n_params(shape):
    return sum(i * o for i, o in layer_dims(shape))


def oracle_kw(shape):
    """keyword arguments of oracle.capi.mlp_small / mlp_small_backward behind (params, x[, g_out])"""
    v, nl, nlc, g = shape
    return dict(in_ch=IN_CH, in_views=v, n_layers=nl, hidden=HIDDEN, geo=g, n_layers_c=nlc, hidden_c=HIDDEN)


def matrices(blob, shape):
    """-> float64 W [out][in] per layer"""
    blob = np.asarray(blob).reshape(-1)
    assert blob.size == n_params(shape), (blob.size, n_params(shape))
    out, off = [], 0
    for i, o in layer_dims(shape):
        out.append(blob[off:off + i * o].astype(np.float64).reshape(o, i))
        off += i * o
    return out


def _forward(mats, x, shape):
    """-> (out [p, 4] = [rgb, sigma], the input of every layer, every pre-activation)"""
    v, nl, nlc, g = shape
    x = np.asarray(x, np.float64)
    assert x.shape[1] == IN_CH + v
    ins, pres = [], []
    h = x[:, :IN_CH]
    for l in range(nl):
        ins.append(h)
        h = h @ mats[l].T
        pres.append(h)
        if l < nl - 1:
            h = np.maximum(h, 0.0)          # ReLU between the layers, none after the last (NeRF.cpp:372-381)
    sig = h                                 # [sigma, geo_feat]
    c = np.concatenate([x[:, IN_CH:], sig[:, 1:]], 1)          # cat[views, geo]
    for l in range(nlc):
        ins.append(c)
        c = c @ mats[nl + l].T
        pres.append(c)
        if l < nlc - 1:
            c = np.maximum(c, 0.0)
    return np.concatenate([c, sig[:, :1]], 1), ins, pres


def forward64(blob, x, shape):
    """NeRFSmallImpl::forward (NeRF.cpp:322-412) in float64 -> [p, 4] = [rgb, sigma]"""
    return _forward(matrices(blob, shape), x, shape)[0]


def backward64(blob, x, g_out, shape):
    """Gradients of sum(out * g_out) -> (dW as one blob in parameter order, d / d x[:, :32]) in float64"""
    v, nl, nlc, g = shape
    mats = matrices(blob, shape)
    _, ins, pres = _forward(mats, x, shape)
    g_out = np.asarray(g_out, np.float64)
    grads = [None] * (nl + nlc)
    gc = g_out[:, :3]
    for l in range(nlc - 1, -1, -1):
        if l < nlc - 1:
            gc = gc * (pres[nl + l] > 0)
        grads[nl + l] = gc.T @ ins[nl + l]
        gc = gc @ mats[nl + l]
    gs = np.concatenate([g_out[:, 3:4], gc[:, v:]], 1)          # d / d [sigma, geo_feat]
    for l in range(nl - 1, -1, -1):
        if l < nl - 1:
            gs = gs * (pres[l] > 0)
        grads[l] = gs.T @ ins[l]
        gs = gs @ mats[l]
    return np.concatenate([w.reshape(-1) for w in grads]), gs


def _integer_candidate(shape, rng, rows):
    v, nl, nlc, g = shape
    mats = []
    for li, (i, o) in enumerate(layer_dims(shape)):
        w = np.zeros((o, i), np.float32)
        nz = rng.random((o, i)) < (3.0 if li < nl else 5.0) / i          # (the colour net a little denser: more of its neurons reach rgb)
        w[nz] = rng.choice([-1.0, 1.0], size=int(nz.sum()))
        if li == nl - 1 or li == nl + nlc - 1:             # the last layers: every row (sigma, each geo feature; r, g, b) reads something
            for r in range(o):
                if not w[r].any():
                    w[r, rng.integers(0, i)] = rng.choice([-1.0, 1.0])
        mats.append(w)
    # colour layer 0: every geo column V..V+G-1 is read by two neurons from which weights lead on to rgb
    alive = np.ones(3, bool)
    for li in range(nl + nlc - 1, nl, -1):
        alive = (mats[li][alive] != 0).any(0)
    alive = np.nonzero(alive)[0]
    for c in range(v, v + g):
        for r in rng.choice(alive, size=min(2, alive.size), replace=False):
            if not mats[nl][r, c]:
                mats[nl][r, c] = rng.choice([-1.0, 1.0])
    x = np.concatenate([rng.integers(-2, 3, (rows, IN_CH)), rng.integers(-1, 2, (rows, v))], 1).astype(np.float32)
    return mats, x


def check_integer_network(blob, x, shape, want_varied=True):
    """The properties the exact tests rest on, in float64: every weight is -1 / 0 / +1, every activation an integer below 2048 (fp16 holds it exactly, fp32 sums of
    them are exact in any order), no pre-activation within 1/2 of the ReLU kink unless it is 0 itself, the geo columns and rows all in use -> out"""
    v, nl, nlc, g = shape
    mats = matrices(blob, shape)
    assert all(np.isin(w, (-1.0, 0.0, 1.0)).all() for w in mats)
    assert all(mats[nl][:, c].any() for c in range(v, v + g)), "every geo column of colour layer 0 is non-zero"
    assert all(mats[nl - 1][r].any() for r in range(1, 1 + g)), "every geo row of the last sigma layer is non-zero"
    out, ins, pres = _forward(mats, x, shape)
    for a in ins + pres:
        assert np.array_equal(a, np.rint(a)) and np.abs(a).max() < 2048
    for a in pres:
        assert not ((a != 0) & (np.abs(a) <= 0.5)).any()
    if want_varied:
        for c in range(4):
            assert np.ptp(out[:, c]) > 0, f"output column {c} is constant over the batch"
    return out


def geo_columns_matter(blob, x, shape):
    """zeroing any one geo column of colour layer 0 changes rgb somewhere in the batch (float64)"""
    v, nl, nlc, g = shape
    mats = matrices(blob, shape)
    base = _forward(mats, x, shape)[0]
    for c in range(v, v + g):
        w = mats[nl].copy()
        w[:, c] = 0.0
        if np.array_equal(_forward(mats[:nl] + [w] + mats[nl + 1:], x, shape)[0][:, :3], base[:, :3]):
            return False
    return True


def integer_network(shape, seed, p):
    """Sparse -1 / 0 / +1 weights, features in -2..2 and view inputs in -1..1 -> (blob float32, x float32 [p, 32 + V], forward64 of them [p, 4]).
    The network depends on (shape, seed) alone: the first candidate on whose 64-row probe batch each of r, g, b and sigma varies and every single geo column
    moves rgb (so each geo input is carried by a column of its own that a wrong column map would show).  The batch is drawn for max(p, 64) rows, on which the
    outputs vary again, and ordered so that the first row has a non-zero sigma and a non-zero colour (the one-point case then still tells a result from a
    cleared buffer)."""
    for attempt in range(256):
        rng = np.random.default_rng([int(seed), attempt] + [int(q) for q in shape])
        mats, probe = _integer_candidate(shape, rng, 64)
        blob = np.concatenate([w.reshape(-1) for w in mats])
        out = forward64(blob, probe, shape)
        if all(np.ptp(out[:, c]) > 0 for c in range(4)) and geo_columns_matter(blob, probe, shape):
            break
    else:
        raise AssertionError(f"no integer network for {shape} seed {seed}")
    rows = max(int(p), 64)
    rng = np.random.default_rng([int(seed), 977, rows] + [int(q) for q in shape])
    x = np.concatenate([rng.integers(-2, 3, (rows, IN_CH)), rng.integers(-1, 2, (rows, shape[0]))], 1).astype(np.float32)
    out = check_integer_network(blob, x, shape)
    good = np.nonzero((out[:, 3] != 0) & (out[:, :3] != 0).any(1))[0]
    assert good.size, "no row with a non-zero sigma and colour"
    order = np.concatenate([good[:1], np.delete(np.arange(rows), good[0])])
    x = np.ascontiguousarray(x[order][:p])
    return blob, x, check_integer_network(blob, x, shape, want_varied=False)


def random_network(shape, seed, sigma_scale=None):
    """scene.synth_linear_stack with gain 1.6 (make_hash_scene's fill); sigma_scale multiplies the last sigma layer (x 30 in the scenes) -> blob float32"""
    v, nl, nlc, g = shape
    params = S.synth_linear_stack(S.small_shapes(IN_CH, v, nl, HIDDEN, g, nlc, HIDDEN), seed, 1.6, 0.0, {f"sigma_net_{nl - 1}": sigma_scale} if sigma_scale else None)
    return np.concatenate([a.reshape(-1) for _, a in params])


def random_inputs(shape, seed, p):
    """features as the CuHashEmbedder produces them (fp16 numbers in [-1, 1]) next to fp32 view features in [-1, 1] -> x float32 [p, 32 + V]"""
    rng = np.random.RandomState(seed)
    x = rng.uniform(-1, 1, (p, IN_CH + shape[0])).astype(np.float32)
    x[:, :IN_CH] = x[:, :IN_CH].astype(np.float16).astype(np.float32)
    return x


def group_errors(got, ref):
    """-> {group: (max |got - ref| / max |ref|, mean |got - ref| / max |ref|)} for the rgb columns and the sigma column, each on its own scale"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    out = {}
    for name, cols in (("rgb", slice(0, 3)), ("sigma", slice(3, 4))):
        scale = np.abs(ref[:, cols]).max()
        d = np.abs(got[:, cols] - ref[:, cols])
        out[name] = (d.max() / scale, d.mean() / scale)
    return out


# ------------------------------------------------------------------ the training backward: exact integer cases, the fused kernel's arithmetic, level-major packers
FUSED_SHAPES = [(16, nl, nlc, 15) for nl in (2, 3) for nlc in (3, 4)]          # bwd_supported() (mlp_small_bwd_mfma.hip): k_small_bwd<NL, NLC>
LOSS_SCALE = 8.0          # the fused kernel scales max |g_out| into [16, 32): with max |gk| = 2 that is x 8


def tensors(shape):
    """-> [(name, offset, (out, in))] of the parameter blob, in blob order"""
    v, nl, nlc, g = shape
    names = ["sigma_net_%d" % l for l in range(nl)] + ["color_net_%d" % l for l in range(nlc)]
    out, off = [], 0
    for name, (i, o) in zip(names, layer_dims(shape)):
        out.append((name, off, (o, i)))
        off += i * o
    return out


def _chain64(blob, x, g_out, shape):
    """backward64's chain with every tensor kept -> (d / d each layer's output behind its ReLU mask, each layer's input, every product g . W before its mask; the last is g_x)"""
    v, nl, nlc, g = shape
    mats = matrices(blob, shape)
    _, ins, pres = _forward(mats, x, shape)
    g_out = np.asarray(g_out, np.float64)
    outg, chained = [None] * (nl + nlc), []
    gc = g_out[:, :3]
    for l in range(nlc - 1, -1, -1):
        if l < nlc - 1:
            gc = gc * (pres[nl + l] > 0)
        outg[nl + l] = gc
        gc = gc @ mats[nl + l]
        chained.append(gc)
    gs = np.concatenate([g_out[:, 3:4], gc[:, v:]], 1)
    for l in range(nl - 1, -1, -1):
        if l < nl - 1:
            gs = gs * (pres[l] > 0)
        outg[l] = gs
        gs = gs @ mats[l]
        chained.append(gs)
    return outg, ins, chained


def integer_backward_case(shape, seed, p, unit=2.0 ** -22, s=None):
    """integer_network(shape, seed, p) with output gradients g_out = gk * unit, gk integers in -2..2: row 0 is non-zero in all four columns, and the largest |gk| = 2
    occurs in the last row's sigma column (so the device's loss scale 2^(4 - e) is x 8 / unit whatever the draw) -> (blob, x, g_out float32, (want_params, want_x) =
    backward64 of them).  `unit` is a power of two.
    With s given the view columns are one integer row per ray, constant over each run of s consecutive points (the last ray may be partial), and every eleventh point
    from the fifth on carries the features of an earlier point (so a column table has columns that several points read): the batch can then be fed in level-major form
    (pack_level_major, pack_ray_views, pack_column_table); check_integer_network is run again on it.
    Asserted in float64, in units of `unit`: every chained gradient at every layer x 8 is an integer below 2048 (fp16 holds it exactly under the loss scale); for every
    weight-gradient entry the sum of |terms| x 8 is below 2^24 (fp32 sums are exact in any order); every layer's gradient tensor and g_x are non-zero somewhere."""
    v, nl, nlc, g = shape
    shape, seed, p = tuple(int(q) for q in shape), int(seed), int(p)
    assert np.frexp(unit)[0] == 0.5, "unit is a power of two"
    blob, x, _ = integer_network(shape, seed, p)
    if s is not None:
        s = int(s)
        assert s >= 1
        rng = np.random.default_rng([seed, 1301, p, s] + list(shape))
        x = x.copy()
        x[:, IN_CH:] = np.repeat(rng.integers(-1, 2, (-(-p // s), v)), s, 0)[:p]
        dup = np.arange(5, p, 11)
        x[dup, :IN_CH] = x[dup // 3, :IN_CH]
        check_integer_network(blob, x, shape, want_varied=False)
    rng = np.random.default_rng([seed, 1303, p] + list(shape))
    gk = rng.integers(-2, 3, (p, 4)).astype(np.float64)
    gk[0] = rng.choice([-1.0, 1.0], 4)
    gk[p - 1, 3] = 2.0 * rng.choice([-1.0, 1.0])
    assert gk[0].all() and np.abs(gk).max() == 2 == abs(gk[p - 1, 3])
    outg, ins, chained = _chain64(blob, x, gk, shape)
    what = f"{shape_id(shape)} seed {seed} p {p} s {s}"
    for t in outg + chained:
        assert np.array_equal(t, np.rint(t)) and LOSS_SCALE * np.abs(t).max() < 2048, (what, np.abs(t).max())
    for li, (go, a) in enumerate(zip(outg, ins)):
        if go.shape[1] and a.shape[1]:
            assert LOSS_SCALE * (np.abs(go).T @ np.abs(a)).max() < 2 ** 24, (what, li)
            assert (go.T @ a).any(), f"{what}: the gradient of layer {li} is all zero"
    assert chained[-1].any(), f"{what}: g_x is all zero"
    g_out = (gk * unit).astype(np.float32)
    assert np.array_equal(g_out.astype(np.float64), gk * unit)
    want_p, want_x = backward64(blob, x, g_out, shape)
    assert np.array_equal(want_x, chained[-1] * unit) and np.array_equal(want_p, np.concatenate([(go.T @ a).reshape(-1) for go, a in zip(outg, ins)]) * unit)
    for a in (blob, x, g_out, want_p, want_x):
        a.setflags(write=False)
    return blob, x, g_out, (want_p, want_x)


def prefill(n, unit):
    """a gradient blob that is not zero to start from: small integer multiples of `unit`"""
    return (((np.arange(n) % 7) - 3) * unit).astype(np.float32)


def model16(blob, x, g_out, shape, acc=np.float64):
    """The fused backward's arithmetic (k_small_bwd, mlp_small_bwd_mfma.hip) restated: rounded to fp16 are the weights, x, the view features, every hidden activation
    behind its ReLU and [sigma, geo] on its way into the colour net; the loss scale is S = 2^(4 - e), e the exponent of max |g_out|; rounded to fp16 behind it are
    g_out[:, :3] * S and [g_sigma * S, the geo gradient]; every masked chained gradient is rounded to fp16; a mask is 'the fp16 activation > 0'.  Products accumulate in
    `acc`; g_x leaves unrounded; everything is divided by S at the end.  -> (g_params, g_x, the pre-activations under every ReLU: sigma net's, then colour net's)"""
    v, nl, nlc, g = shape
    assert tuple(shape) in FUSED_SHAPES, shape
    h16 = lambda a: np.asarray(a).astype(np.float16).astype(acc)
    mats = [h16(w) for w in matrices(blob, shape)]
    x, g_out = np.asarray(x, np.float32), np.asarray(g_out, np.float32)
    ins, pres = [], []
    h = h16(x[:, :IN_CH])
    for l in range(nl):
        ins.append(h)
        a = h @ mats[l].T
        if l < nl - 1:
            pres.append(a)
            h = h16(np.maximum(a, 0))
    c = np.concatenate([h16(x[:, IN_CH:]), h16(a)[:, 1:]], 1)
    for l in range(nlc - 1):
        ins.append(c)
        a = c @ mats[nl + l].T
        pres.append(a)
        c = h16(np.maximum(a, 0))
    ins.append(c)
    finite = np.abs(g_out[np.isfinite(g_out)])
    gmax = float(finite.max()) if finite.size else 0.0
    S = np.float32(1.0 if gmax == 0 else 2.0 ** (4 - int(np.clip(np.frexp(np.float32(gmax))[1] - 1, -100, 100))))
    grads = [None] * (nl + nlc)
    gc = h16(g_out[:, :3] * S)
    for l in range(nlc - 1, -1, -1):
        grads[nl + l] = gc.T @ ins[nl + l]
        gc = gc @ mats[nl + l]
        if l > 0:
            gc = h16(gc * (ins[nl + l] > 0))
    gs = h16(np.concatenate([(g_out[:, 3:4] * S).astype(acc), gc[:, v:]], 1))
    for l in range(nl - 1, -1, -1):
        grads[l] = gs.T @ ins[l]
        gs = gs @ mats[l]
        if l > 0:
            gs = h16(gs * (ins[l] > 0))
    return np.concatenate([w.reshape(-1) for w in grads]).astype(np.float64) / float(S), gs.astype(np.float64) / float(S), pres


def relu_masks16(pres):
    """model16's masks from its pre-activations: the fp16 activation > 0"""
    return [np.maximum(np.asarray(a), 0).astype(np.float16) > 0 for a in pres]


def kink_free16(blob, shape, seed, p, margin, candidates=4096):
    """The first p rows of random_inputs(shape, seed, candidates) on which no model16 pre-activation under a ReLU lies within `margin` of zero -> x float32 [p, 32 + V]"""
    x = random_inputs(shape, seed, candidates)
    pres = model16(blob, x, np.zeros((candidates, 4), np.float32), shape)[2]
    ok = np.all([(np.abs(a) >= margin).all(1) for a in pres], 0)
    assert ok.sum() >= p, (ok.sum(), p)
    return np.ascontiguousarray(x[ok][:p])


def pack_level_major(x):
    """x[:, :32] -> the level-major fp16 features [16 levels][cols] half2, as float16 [16, cols, 2] (level l carries features 2 l and 2 l + 1)"""
    f = np.asarray(x)[:, :IN_CH].astype(np.float16)
    assert np.array_equal(f.astype(np.float32), np.asarray(x)[:, :IN_CH]), "the features are fp16 numbers"
    return np.ascontiguousarray(f.reshape(-1, IN_CH // 2, 2).transpose(1, 0, 2))


def pack_ray_views(x, s):
    """the view columns, constant over each run of s points -> one fp16 row per ray [rays, V]"""
    views = np.asarray(x)[:, IN_CH:]
    assert np.array_equal(views, np.repeat(views[::s], s, 0)[:len(views)]), "one view row per ray"
    return np.ascontiguousarray(views[::s].astype(np.float16))


def pack_column_table(x, seed, unused=9, slack=5, filler=77.0):
    """The column-map form: -> (table float16 [16, pstride, 2], src int32 [p], pstride) with x[q, :32] = column src[q] of the table.  Points with equal features share
    a column, `unused` columns are read by nobody, the columns are shuffled (the map is not monotonic) and pstride exceeds the column count by `slack`; what no point
    reads holds `filler`, which no integer batch contains."""
    f = np.asarray(x)[:, :IN_CH]
    uniq, inv = np.unique(f, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    rng = np.random.default_rng([int(seed), 1307, len(f)])
    cols = len(uniq) + unused
    where = rng.permutation(cols)[:len(uniq)]          # unique row u sits in column where[u]
    rows = np.full((cols + slack, IN_CH), filler, np.float32)
    rows[where] = uniq
    src = where[inv].astype(np.int32)
    counts = np.bincount(src, minlength=cols)
    assert np.array_equal(rows[src], f)
    assert len(f) < 8 or ((np.diff(src) < 0).any() and counts.max() > 1 and (counts == 0).any()), "the map is not monotonic; columns read by several points and by none"
    return pack_level_major(rows), src, cols + slack


# ---- the cases of tests/test_mlp_small_bwd_shapes_gpu.py (tests/test_mlp_small_shapes_host.py asserts the integer conditions for every one of them on the CPU)
BWD_SEED = 11
BWD_UNIT = 2.0 ** -22
FUSED_COUNTS = (1, 31, 32, 33, 127, 128, 129, 257, 32769)          # one point; both sides of the 32-point wave tile and of the 128-point workgroup block; two blocks and
                                                                    # a point; 256 workgroups x 128 points + 1: workgroup 0 takes a second iteration of the persistent loop
FUSED_UNITS_AT = 129
FUSED_UNITS = (2.0 ** -40, 1.0, 2.0 ** 20)
FUSED_PREFILLED = (1, 129)
LM_CASES = ((129, 24), (4097, 64))                                  # (points, points per ray): the last ray is partial in both
CHAIN_COUNTS = (1, 255, 256, 257)                                   # both sides of the 256-point switch between mlp.hip's kernels and the library / split products
CHAIN_MODE_SHAPES = FUSED_SHAPES + BWD_REFUSED + [(16, 2, 2, 0), (64, 2, 3, 1), (64, 3, 4, 14)]
CHAIN_MODE_COUNTS = (257, 4097)                                     # 4 097: one past the threshold of the split-precision weight-gradient products
CHAIN_SLICED_COUNT = 16400                                          # mode 0 with rocBLAS: 32 slices of 512 points and a remainder of 16
RANDOM_SHAPES = [(16, 3, 4, 15), (16, 2, 3, 15)]
RANDOM_POINTS, RANDOM_SEED, RANDOM_MARGIN, RANDOM_MARGIN64 = 700, 5, 1e-4, 1e-4


def backward_cases():
    """-> every (shape, points, unit, points per ray or None) the GPU module runs on integer networks"""
    out = [(sh, p, BWD_UNIT, None) for sh in FUSED_SHAPES for p in FUSED_COUNTS]
    out += [(sh, FUSED_UNITS_AT, u, None) for sh in FUSED_SHAPES for u in FUSED_UNITS]
    out += [(sh, p, BWD_UNIT, s) for sh in FUSED_SHAPES for p, s in LM_CASES]
    out += [(sh, p, BWD_UNIT, None) for sh in SHAPES for p in CHAIN_COUNTS]
    out += [(sh, p, BWD_UNIT, None) for sh in CHAIN_MODE_SHAPES for p in CHAIN_MODE_COUNTS + (CHAIN_SLICED_COUNT,)]
    return list(dict.fromkeys(out))


def random_backward_case(shape):
    """random_network(shape, 7000, 30.0) with output gradients of 1e-3 on 700 rows of kink_free16 (no model16 pre-activation under a ReLU within 1e-4 of zero) that
    also keep clear of the kink in float64: no pre-activation of forward64 within 1e-4 of its layer's largest.  The second condition is for the fp32 chain in its
    split-precision modes: bf16x3 carries 16 significant bits, 1.5e-5 of a layer's magnitude, and a mask decided the other way moves a tensor by whole terms (the
    classic network's random test met exactly that; profiles/mlp_nerf_shapes/measured_errors.txt).  -> (blob, x, g_out float32)"""
    v, nl, nlc, g = shape
    blob = random_network(shape, 7000, 30.0)
    x = kink_free16(blob, shape, RANDOM_SEED, 2 * RANDOM_POINTS, RANDOM_MARGIN)
    pres = _forward(matrices(blob, shape), x, shape)[2]
    under = [pres[l] for l in range(nl - 1)] + [pres[nl + l] for l in range(nlc - 1)]
    ok = np.all([(np.abs(a) >= RANDOM_MARGIN64 * np.abs(a).max()).all(1) for a in under], 0)
    assert ok.sum() >= RANDOM_POINTS, (ok.sum(), RANDOM_POINTS)
    x = np.ascontiguousarray(x[ok][:RANDOM_POINTS])
    g_out = (np.random.RandomState(9).standard_normal((RANDOM_POINTS, 4)) * 1e-3).astype(np.float32)
    return blob, x, g_out


def tensor_errors(got_p, got_x, ref_p, ref_x, shape):
    """-> {tensor name or 'g_x': max |got - ref| / max |ref|}"""
    out = {}
    for name, off, (o, i) in tensors(shape):
        a, b = np.asarray(got_p, np.float64)[off:off + o * i], np.asarray(ref_p, np.float64)[off:off + o * i]
        out[name] = np.abs(a - b).max() / np.abs(b).max()
    if got_x is not None:
        out["g_x"] = np.abs(np.asarray(got_x, np.float64) - ref_x).max() / np.abs(ref_x).max()
    return out
