"""Cases and the float64 yardstick of the NeRFSmall shape tests (tests/test_mlp_small_shapes_host.py pins the C oracle against it on the CPU,
tests/test_mlp_small_shapes_gpu.py runs the kernels on the same cases).

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
