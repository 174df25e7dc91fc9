"""Cases and the float64 yardstick of the classic-NeRF shape tests (tests/test_mlp_nerf_shapes_host.py pins the C oracle against it on the CPU,
tests/test_mlp_nerf_shapes_gpu.py runs the kernels on the same cases).  Plain numpy: nothing here comes from the library.

A shape is (d, w, in_ch, in_views, out_ch, skip, use_viewdirs) of NeRFImpl (NeRF.cpp:41-126): d layers of width w on input_pts, h = cat[input_pts, h] after layer
`skip`; with view directions alpha_linear(h), feature_linear(h) (no ReLU), relu(views_linears_0(cat[feature, views])), rgb_linear -> [rgb, alpha]; without them
output_linear(cat[h, input_pts]) -> out_ch columns.  The parameter blob is NeRF.cpp's order -- pts_linears, then views_linears_0, feature_linear, alpha_linear,
rgb_linear or else output_linear -- each as weight [out][in] row-major followed by its bias."""
import functools

import numpy as np

SHAPES = [(8, 256, 63, 27, 5, 4, True),           # the built matrix-core family and the bench network; ReLU masks travel as bits
          (4, 64, 63, 27, 5, 1, True),            # N <= 128: float masks; the thin back-propagation kernel still serves the heads
          (3, 160, 63, 0, 5, 0, False)]           # output_linear on cat[h, input_pts]; a width inside the mask-bit range that is not 256; the skip right after layer 0
BUILT = SHAPES[0]
TILE_ROWS = 257                                   # tiled() repeats a batch of this many rows
OPERAND_MAX, SUM_MAX = 256, 1 << 24               # bf16 holds integers up to 256; fp32 sums of integers below 2^24 are exact in any order


def shape_id(shape):
    d, w, in_ch, in_views, out_ch, skip, vd = shape
    return "d%d-w%d-v%d-skip%d-%s" % (d, w, in_views, skip, "views" if vd else "out%d" % out_ch)


def out_dims(shape):
    return 4 if shape[6] else shape[4]


def layers(shape):
    """-> [(name, out, in)] in blob order"""
    d, w, in_ch, in_views, out_ch, skip, vd = shape
    assert 0 <= skip < d - 1
    ls = [("pts_linears_%d" % l, w, in_ch if l == 0 else (w + in_ch if l - 1 == skip else w)) for l in range(d)]
    if vd:
        return ls + [("views_linears_0", w // 2, w + in_views), ("feature_linear", w, w), ("alpha_linear", 1, w), ("rgb_linear", 3, w // 2)]
    return ls + [("output_linear", out_ch, w + in_ch)]


def tensors(shape):
    """-> [(name, offset, shape)] of every parameter tensor in blob order: 'pts_linears_0.weight', 'pts_linears_0.bias', ..."""
    out, off = [], 0
    for name, o, i in layers(shape):
        out.append((name + ".weight", off, (o, i))); off += o * i
        out.append((name + ".bias", off, (o,))); off += o
    return out


def n_params(shape):
    return sum(o * i + o for _, o, i in layers(shape))


def oracle_kw(shape):
    """keyword arguments of oracle.capi.mlp_nerf / mlp_nerf_backward behind (params, x[, g_out])"""
    return dict(zip(("d", "w", "in_ch", "in_views", "out_ch", "skip", "use_viewdirs"), shape))


def matrices(blob, shape):
    """-> {layer name: (W [out][in], b [out])} in float64"""
    blob = np.asarray(blob).reshape(-1)
    assert blob.size == n_params(shape), (blob.size, n_params(shape))
    out, off = {}, 0
    for name, o, i in layers(shape):
        out[name] = (blob[off:off + o * i].astype(np.float64).reshape(o, i), blob[off + o * i:off + o * i + o].astype(np.float64))
        off += o * i + o
    return out


def pack(mats, shape):
    """{layer name: (W, b)} -> blob float32"""
    return np.concatenate([np.concatenate([np.asarray(mats[name][0]).reshape(-1), np.asarray(mats[name][1]).reshape(-1)]) for name, _, _ in layers(shape)]).astype(np.float32)


def _forward(mats, x, shape):
    d, w, in_ch, in_views, out_ch, skip, vd = shape
    x = np.asarray(x, np.float64)
    assert x.ndim == 2 and x.shape[1] == in_ch + in_views, x.shape
    pts, views = x[:, :in_ch], x[:, in_ch:]
    ins, pres = {}, {}

    def linear(name, a):
        ins[name] = a
        pres[name] = a @ mats[name][0].T + mats[name][1]
        return pres[name]
    h = pts
    for l in range(d):
        h = np.maximum(linear("pts_linears_%d" % l, h), 0.0)
        if l == skip:
            h = np.concatenate([pts, h], 1)                  # NeRF.cpp:103-104
    if vd:
        alpha = linear("alpha_linear", h)
        feat = linear("feature_linear", h)                   # no ReLU (:110); then views_linears_0 on its own, as the reference runs it -- not the merged layer
        hv = np.maximum(linear("views_linears_0", np.concatenate([feat, views], 1)), 0.0)
        return np.concatenate([linear("rgb_linear", hv), alpha], 1), ins, pres
    return linear("output_linear", np.concatenate([h, pts], 1)), ins, pres


def forward64(blob, x, shape):
    """NeRFImpl::forward in float64 -> (out [p, out dims], {layer: its input}, {layer: its pre-activation})"""
    return _forward(matrices(blob, shape), x, shape)


def _backward(mats, x, g_out, shape):
    """-> ({layer: (dW, db)}, g_x, every gradient array formed on the way, the (g, W) and (g, input) pairs of its products)"""
    d, w, in_ch, in_views, out_ch, skip, vd = shape
    _, ins, pres = _forward(mats, x, shape)
    g_out = np.asarray(g_out, np.float64)
    assert g_out.shape == (np.asarray(x).shape[0], out_dims(shape)), g_out.shape
    grads, stages, products = {}, [g_out], []

    def through(name, g):
        """the layer's parameter gradients; -> the gradient of its input"""
        grads[name] = (g.T @ ins[name], g.sum(0))
        products.append((name, g))
        stages.append(g @ mats[name][0])
        return stages[-1]
    g_x = np.zeros((g_out.shape[0], in_ch))
    if vd:
        g_hv = through("rgb_linear", g_out[:, :3]) * (pres["views_linears_0"] > 0)
        stages.append(g_hv)
        g_feat = through("views_linears_0", g_hv)[:, :w]
        g_h = through("feature_linear", g_feat) + through("alpha_linear", g_out[:, 3:4])
    else:
        g_c = through("output_linear", g_out)
        g_h, g_x = g_c[:, :w], g_x + g_c[:, w:]
    for l in range(d - 1, -1, -1):
        name = "pts_linears_%d" % l
        g = g_h * (pres[name] > 0)
        stages += [g_h, g]
        g_in = through(name, g)
        if l == 0:
            g_x = g_x + g_in
        elif l - 1 == skip:
            g_x, g_h = g_x + g_in[:, :in_ch], g_in[:, in_ch:]
        else:
            g_h = g_in
    stages.append(g_x)
    return grads, g_x, stages, products


def backward64(blob, x, g_out, shape):
    """Gradients of sum(out * g_out) in float64 -> (g_params as a blob, g_x [p, in_ch])"""
    grads, g_x, _, _ = _backward(matrices(blob, shape), x, g_out, shape)
    return np.concatenate([np.concatenate([grads[name][0].reshape(-1), grads[name][1]]) for name, _, _ in layers(shape)]), g_x


def tiled(a, p):
    """rows 0 .. 256 of a TILE_ROWS-row array repeated up to p rows: a large count costs one 257-row float64 evaluation"""
    a = np.asarray(a)
    assert a.shape[0] == TILE_ROWS
    return np.ascontiguousarray(a[np.arange(int(p)) % TILE_ROWS])


# ------------------------------------------------------------------ integer networks
def _whole(a, what):
    assert np.array_equal(a, np.rint(a)) and np.abs(a).max(initial=0.0) <= OPERAND_MAX, f"{what}: not an integer of magnitude <= {OPERAND_MAX} ({np.abs(a).max(initial=0.0)})"


def check_integer_network(blob, x, g_out, shape, batch=True):
    """The conditions the exact tests rest on, asserted in float64 (AssertionError otherwise) -> (out, (g_params blob, g_x)).
    Network: every weight and bias is -1 / 0 / +1; every layer has a non-zero bias; every row of the alpha and rgb (or output) layers is non-zero; every
    input_pts column of the skip layer meets a non-zero weight; every entry of the merged W_v[:, :w] . F and of its bias is an integer <= 256 in magnitude.
    Arithmetic: every operand of every product -- the inputs, every activation, feature_linear's output, the gradient at every stage -- is an integer <= 256 in
    magnitude; for every output element of every product (forward, merged forward, back-propagation, weight gradient, bias gradient) the sum of |terms| is below
    2^24; no pre-activation lies in (0, 1/2].
    Batch (batch=True; a truncated batch keeps the arithmetic conditions, not these): every output column varies; sigma and a colour are non-zero in row 0; the
    weight gradient of every input_pts column of the skip layer is non-zero somewhere (the column feeds a live neuron); one x row and one g_out row are all zero."""
    d, w, in_ch, in_views, out_ch, skip, vd = shape
    mats = matrices(blob, shape)
    x, g_out = np.asarray(x, np.float64), np.asarray(g_out, np.float64)
    for name, (W, b) in mats.items():
        assert np.isin(W, (-1.0, 0.0, 1.0)).all() and np.isin(b, (-1.0, 0.0, 1.0)).all(), name
        assert b.any(), f"{name}: no non-zero bias"
    for name in ("alpha_linear", "rgb_linear") if vd else ("output_linear",):
        assert mats[name][0].any(1).all(), f"{name}: a row is all zero"
    skip_name = "pts_linears_%d" % (skip + 1)
    assert mats[skip_name][0][:, :in_ch].any(0).all(), "an input_pts column of the skip layer is all zero"
    if vd:
        Wv, bv = mats["views_linears_0"]
        F, bf = mats["feature_linear"]
        merged, merged_b = Wv[:, :w] @ F, Wv[:, :w] @ bf + bv
        _whole(merged, "merged views layer"); _whole(merged_b, "merged views bias")
        assert (np.abs(Wv[:, :w]) @ np.abs(F)).max() < SUM_MAX
    out, ins, pres = _forward(mats, x, shape)
    for name, a in ins.items():
        _whole(a, "input of " + name)
        _whole(pres[name], "pre-activation of " + name)
        assert not ((pres[name] > 0) & (pres[name] <= 0.5)).any(), name
        assert (np.abs(a) @ np.abs(mats[name][0]).T + np.abs(mats[name][1])).max() < SUM_MAX, name
    if vd:
        h = ins["feature_linear"]
        assert (np.abs(h) @ np.abs(merged).T + np.abs(x[:, in_ch:]) @ np.abs(Wv[:, w:]).T + np.abs(merged_b)).max() < SUM_MAX
    grads, g_x, stages, products = _backward(mats, x, g_out, shape)
    for g in stages:
        _whole(g, "a back-propagated gradient")
    for name, g in products:
        assert (np.abs(g) @ np.abs(mats[name][0])).max() < SUM_MAX and (np.abs(g).T @ np.abs(ins[name])).max() < SUM_MAX and np.abs(g).sum(0).max() < SUM_MAX, name
    if batch:
        for c in range(out.shape[1]):
            assert np.ptp(out[:, c]) > 0, f"output column {c} is constant over the batch"
        assert out[0, 3] != 0 and out[0, :3].any(), "row 0 does not differ from a cleared buffer"          # (column 3 is sigma in both head forms)
        assert grads[skip_name][0][:, :in_ch].any(0).all(), "an input_pts column of the skip layer feeds no live neuron"
        assert (~x.any(1)).any() and (~g_out.any(1)).any(), "no all-zero x row / g_out row"
    g_blob = np.concatenate([np.concatenate([grads[name][0].reshape(-1), grads[name][1]]) for name, _, _ in layers(shape)])
    return out, (g_blob, g_x)


def _batch(shape, rng, rows):
    """positions in -2 .. 2, view features in -1 .. 1, g_out in {-1, 0, 1} with half of it zero; row 1 of x and row 2 of g_out all zero"""
    d, w, in_ch, in_views, out_ch, skip, vd = shape
    x = np.concatenate([rng.integers(-2, 3, (rows, in_ch)), rng.integers(-1, 2, (rows, in_views))], 1).astype(np.float32)
    g = (rng.integers(0, 2, (rows, out_dims(shape))) * rng.choice([-1.0, 1.0], size=(rows, out_dims(shape)))).astype(np.float32)
    if rows >= 3:
        x[1] = 0.0
        g[2] = 0.0
    return x, g


def _candidate(shape, rng):
    d, w, in_ch, in_views, out_ch, skip, vd = shape
    mats = {}
    for name, o, i in layers(shape):
        heads = name in ("alpha_linear", "rgb_linear", "output_linear")
        per_row = 8.0 if heads else (4.0 if name == "views_linears_0" else 3.0)
        W = np.zeros((o, i))
        nz = rng.random((o, i)) < per_row / i
        W[nz] = rng.choice([-1.0, 1.0], size=int(nz.sum()))
        for r in range(o):
            if heads and not W[r].any():
                W[r, rng.integers(0, i)] = rng.choice([-1.0, 1.0])
        b = np.where(rng.random(o) < 0.25, rng.choice([-1.0, 1.0], size=o), 0.0)
        if not b.any():
            b[rng.integers(0, o)] = rng.choice([-1.0, 1.0])
        mats[name] = (W, b)
    # the skip layer: every input_pts column is read by two neurons from which weights lead on to the output
    if vd:
        alive = mats["rgb_linear"][0].any(0)
        alive = (mats["views_linears_0"][0][alive][:, :w] != 0).any(0)
        alive = (mats["feature_linear"][0][alive] != 0).any(0) | (mats["alpha_linear"][0][0] != 0)
    else:
        alive = (mats["output_linear"][0][:, :w] != 0).any(0)
    for l in range(d - 1, skip + 1, -1):
        alive = (mats["pts_linears_%d" % l][0][alive][:, (in_ch if l - 1 == skip else 0):] != 0).any(0)
    alive = np.nonzero(alive)[0]
    W = mats["pts_linears_%d" % (skip + 1)][0]
    for c in range(in_ch):
        for r in rng.choice(alive, size=min(2, alive.size), replace=False):
            if not W[r, c]:
                W[r, c] = rng.choice([-1.0, 1.0])
    return mats


ATTEMPTS, PROBE_ROWS = 64, 1025


@functools.lru_cache(maxsize=None)
def _network(shape, seed):
    """the first candidate of (shape, seed) that meets every condition of check_integer_network on a 1025-row probe batch -> (blob, attempts used)"""
    last = None
    for attempt in range(ATTEMPTS):
        rng = np.random.default_rng([int(seed), attempt] + [int(q) for q in shape])
        try:
            blob = pack(_candidate(shape, rng), shape)
            x, g = _batch(shape, rng, PROBE_ROWS)
            out, _ = check_integer_network(blob, x, g, shape, batch=False)
            assert all(np.ptp(out[:, c]) > 0 for c in range(out.shape[1]))
        except (AssertionError, ValueError) as e:           # discarded: the next candidate is tried, no condition is relaxed
            last = e
            continue
        blob.setflags(write=False)
        return blob, attempt + 1
    raise AssertionError(f"no integer network for {shape_id(shape)} seed {seed} in {ATTEMPTS} attempts: {last}")


def attempts_used(shape, seed):
    return _network(tuple(shape), int(seed))[1]


@functools.lru_cache(maxsize=64)
def _integer_network(shape, seed, p):
    d, w, in_ch, in_views, out_ch, skip, vd = shape
    blob = _network(shape, seed)[0]
    rows = max(p, 64)
    rng = np.random.default_rng([seed, 977, rows] + [int(q) for q in shape])
    x, g = _batch(shape, rng, rows)
    out = _forward(matrices(blob, shape), x, shape)[0]
    good = np.nonzero((out[:, 3] != 0) & out[:, :3].any(1))[0]
    good = good[(good == 0) | (good >= 3)]                  # (rows 1 and 2 are the zero rows)
    assert good.size, "no row with a non-zero sigma and colour"
    x[[0, good[0]]] = x[[good[0], 0]]
    g[[0, good[0]]] = g[[good[0], 0]]
    check_integer_network(blob, x, g, shape, batch=True)
    x, g = np.ascontiguousarray(x[:p]), np.ascontiguousarray(g[:p])
    out, back = check_integer_network(blob, x, g, shape, batch=p >= 64)
    for a in (x, g, out) + back:
        a.setflags(write=False)
    return blob, x, g, out, back


def integer_network(shape, seed, p):
    """Sparse -1 / 0 / +1 weights and biases, positions in -2 .. 2, view features in -1 .. 1, g_out in {-1, 0, 1}
    -> (blob float32, x float32 [p, in_ch + in_views], g_out float32 [p, out dims], forward64's output [p, out dims], backward64 = (g_params blob, g_x [p, in_ch])).
    The network depends on (shape, seed) alone; the batch on p as well: it is drawn for max(p, 64) rows, ordered so that row 0 has a non-zero sigma and a non-zero
    colour, rows 1 and 2 carry the all-zero x row and the all-zero g_out row, checked whole and then cut to p rows and checked again.  Every array is read-only and
    shared between the callers."""
    return _integer_network(tuple(shape), int(seed), int(p))
