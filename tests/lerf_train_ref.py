"""float64 model, case tables and input builders for the stage-level tests of the LeRF head's training backward (nerfpp_amd/csrc/lerf_train.hip: nrf_lerf_head_backward,
nrf_huber_rows_nanmean): tests/test_lerf_train_shapes_host.py checks the model against the reference-autograd goldens and the cases themselves on the CPU,
tests/test_lerf_train_shapes_gpu.py runs them on the device.  No GPU in this file.

The model is torch float64 with autograd, general in dims = (in_ch, n_layers, hidden, geo, embed):
  LeRFImpl::forward (LeRF.cpp:86-108): bias-free sigma net in -> H.. -> [sigma | geo]; LE net cat[geo, x] -> H.. -> E; normalize eps 1e-8 (vector_norm + clamp_min,
  as LibTorch's normalize: backward 0 at a zero vector) -> sigma[~keep] = 0 (+ noise * std) -> RawToLEOutputs' weights (ray_reg_ref.ray_weights: log-space
  transmittance, TruncExp with its clamped backward, as k_lt_ray states them) -> RenderCLIPEmbedding (LeRFRenderer.h:45-54).

Inputs.  Every case draws its points from a POOL of feature rows per network (Net), and a drawn row is accepted only if every hidden pre-activation and the sigma
output lie OUTSIDE a margin of zero, |pre| > 8 u sum|w||x| in float64, with u = 2^-16, the coarsest operand precision of the arithmetics under test (U_MODE: the bits
gemm_bf16x3.hip's header states; the finer modes' margins are inside it): no ReLU is decided the other way by a rounding.  Row DEAD_ROW is all zero (the bias-free
network makes it exactly 0 in every precision).
sigma cannot be set directly, but noise is a free per-sample input added before the relu: with noise_std = 1 and noise = target - sigma_f64 a ray takes any of
per_ray_ref.COMPOSITE_KINDS (targets nearer to zero than NUDGE are moved to +-NUDGE: the relu of the density itself is never on its kink either); zero_sigma is a ray
with keep = 0 throughout and no noise.  What is left are the rays at the 1e-10 clamp of 1 - alpha (per_ray_ref.kink_rays): at most 2 % of a case's rays (SEED0), left
out of the value comparison only."""
import functools

import numpy as np
import torch

import per_ray_ref as PR
from ray_reg_ref import ray_weights, t64

U_MODE = {0: 2.0 ** -24, 1: 2.0 ** -16, 2: 2.0 ** -22}          # operand precision: fp32 products, bf16x3 (16 significant bits), f16x3 (22)
U_MARGIN = max(U_MODE.values())
NUDGE = 1e-3                                                     # smallest |sigma + noise| of a sample with noise (host test: > 8 u_margin sum|w||h| of the sigma row + 1e-6)
POOL_DRAWS = 384
DEAD_ROW = 0
MAX_KINK_SHARE = 0.02                                            # per_ray_ref's cap
DELTA = 1.25

SMALL, MAIN, TINY = (16, 2, 32, 8, 48), (128, 2, 256, 32, 768), (8, 2, 16, 4, 24)
KINDS = PR.COMPOSITE_KINDS


# ------------------------------------------------------------------------------------------------ the network
def layer_shapes(dims):
    """[(out, in)] of the 2 n_layers matrices in blob order: sigma net, then LE net."""
    in_ch, nl, hid, geo, emb = dims
    out, cd = [], in_ch
    for l in range(nl):
        od = 1 + geo if l == nl - 1 else hid
        out.append((od, cd)); cd = od
    cd = geo + in_ch
    for l in range(nl):
        od = emb if l == nl - 1 else hid
        out.append((od, cd)); cd = od
    return out


def param_slices(dims):
    """{name: (offset, (out, in))} in blob order."""
    nl, off, out = dims[1], 0, {}
    for i, (o, k) in enumerate(layer_shapes(dims)):
        out[("sigma_%d" % i) if i < nl else ("le_%d" % (i - nl))] = (off, (o, k)); off += o * k
    return out


def param_count(dims):
    return sum(o * k for o, k in layer_shapes(dims))


def make_blob(dims, seed):
    """uniform +-1 / sqrt(fan_in), as torch's Linear initialises"""
    rng = np.random.default_rng([11, seed, *dims])
    return np.concatenate([rng.uniform(-1.0, 1.0, o * k) / np.sqrt(k) for o, k in layer_shapes(dims)]).astype(np.float32)


def split_blob(blob, dims, grad=False):
    b, off, out = np.asarray(blob, np.float64), 0, []
    for o, k in layer_shapes(dims):
        out.append(t64(b[off:off + o * k].reshape(o, k), grad=grad)); off += o * k
    return out


def net_forward(ws, dims, x, census=None):
    """x [p, in] float64 -> (sigma [p], h [p, E]: the LE net's output before normalize).  census (a list): gets (pre, sum|w||x|) of every hidden layer and of sigma."""
    nl = dims[1]
    h = x
    for l in range(nl):
        pre = h @ ws[l].T
        if census is not None:
            census.append((pre if l != nl - 1 else pre[:, :1], (h.abs() @ ws[l].abs().T) if l != nl - 1 else (h.abs() @ ws[l].abs().T)[:, :1]))
        h = torch.relu(pre) if l != nl - 1 else pre
    sigma = h[:, 0]
    h = torch.cat([h[:, 1:], x], dim=1)
    for l in range(nl):
        pre = h @ ws[nl + l].T
        if census is not None and l != nl - 1:
            census.append((pre, h.abs() @ ws[nl + l].abs().T))
        h = torch.relu(pre) if l != nl - 1 else pre
    return sigma, h


def normalize(x, detach=False):
    nrm = torch.linalg.vector_norm(x, dim=-1, keepdim=True).clamp_min(1e-8)
    return x / (nrm.detach() if detach else nrm)


def model(blob, dims, emb, keep, z, d, g_rendered, noise=None, noise_std=0.0, detach_norms=False):
    """-> dict(weights [n, s], rendered [n, E], g_params [blob order], g_emb [n s, in], sigma [n, s]: the density that goes through the relu) in float64 numpy.
    detach_norms: both norms as constants -- the first term of each normalize backward alone.  At embed = 1 the two terms cancel EXACTLY (x / |x| is a sign: every
    gradient is zero), and what a finite precision leaves is a rounding of that first term: it is the scale the embed = 1 cases are measured on (scale_model)."""
    n, s = np.asarray(z).shape
    ws = split_blob(blob, dims, grad=True)
    x = t64(np.asarray(emb, np.float32), grad=True)
    sigma, h = net_forward(ws, dims, x)
    le = normalize(h, detach_norms)
    if keep is not None:
        sigma = torch.where(torch.as_tensor(np.asarray(keep).reshape(-1) != 0), sigma, torch.zeros_like(sigma))
    nz = None if noise is None else t64(np.asarray(noise, np.float32)).reshape(n, s)
    w, _ = ray_weights(sigma.reshape(n, s), t64(np.asarray(z, np.float32)), t64(np.asarray(d, np.float32)[:, :3]), nz, float(noise_std))
    rendered = normalize((w[..., None] * le.reshape(n, s, -1)).sum(1), detach_norms)
    grads = torch.autograd.grad((rendered * t64(np.asarray(g_rendered, np.float32))).sum(), ws + [x], allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, ws + [x])]
    sr = sigma.detach().reshape(n, s) if nz is None else sigma.detach().reshape(n, s) + nz * float(noise_std)
    return dict(weights=w.detach().numpy(), rendered=rendered.detach().numpy(), g_params=np.concatenate([g.reshape(-1).numpy() for g in grads[:-1]]),
                g_emb=grads[-1].numpy(), sigma=sr.numpy())


def huber_rows_nanmean(pred, target, delta=DELTA):
    """huber_loss(reduction none, delta).sum(-1).nanmean() on the fp32 inputs in float64 -> (loss, d loss / d pred)."""
    p = t64(np.asarray(pred, np.float32), grad=True)
    loss = torch.nn.functional.huber_loss(p, t64(np.asarray(target, np.float32)), reduction="none", delta=float(delta)).sum(-1).nanmean()
    (g,) = torch.autograd.grad(loss, p)
    return float(loss.detach()), g.numpy()


# ------------------------------------------------------------------------------------------------ networks and pools
class Net:
    """A blob of `dims` and its pool: POOL_DRAWS rows drawn uniform(-0.5, 0.5), the accepted ones kept (row DEAD_ROW: all zero, exempt)."""

    def __init__(self, dims, seed=0, blob=None):
        self.dims, self.seed = tuple(dims), seed
        self.blob = make_blob(dims, seed) if blob is None else np.ascontiguousarray(blob, np.float32)
        rng = np.random.default_rng([12, seed, *dims])
        x = rng.uniform(-0.5, 0.5, (POOL_DRAWS, dims[0])).astype(np.float32)
        census = []
        with torch.no_grad():
            sigma, _ = net_forward(split_blob(self.blob, dims), dims, t64(x), census)
        ok = np.ones(POOL_DRAWS, bool)
        for pre, bound in census:
            ok &= (pre.abs() > 8.0 * U_MARGIN * bound).all(1).numpy()
        self.accepted = float(ok.mean())
        self.pool = np.concatenate([np.zeros((1, dims[0]), np.float32), x[ok]])
        self.sigma = np.concatenate([[0.0], sigma.numpy()[ok]])                        # float64, unmasked
        self.sigma_bound = float(census[dims[1] - 1][1].max())                         # sum|w||h| of the sigma row, largest over the draws


@functools.lru_cache(maxsize=None)
def net(dims, seed=0):
    return Net(dims, seed)


# ------------------------------------------------------------------------------------------------ cases
def make_case(dims, n, s, kind, seed, keep_mode="mask", d_stride=3, one_hot=None, blob_seed=0, tag=""):
    """One batch of n rays x s samples on net(dims) -> dict(emb [n s, in], keep [n s] uint8 | None, z [n, s], d [n, d_stride], noise [n, s] | None, noise_std,
    g_rendered [n, E], idx, ...).  kind: one of KINDS, or "plain" (no noise: the network's own density, a fifth of the points masked).
    keep_mode: "mask" (a fifth of the points masked) | "null" (no mask).  From three rays on: ray 1 is FULLY MASKED with a non-positive density (every weight 0, the
    rendered sum v = 0: RenderCLIPEmbedding's clamp, g_v = g / 1e-8); a DEAD point (the pool's zero row) sits at the end of ray 0 and in the middle of the last ray,
    whose last sample stays live.  one_hot: g_rendered is zero except for that ray."""
    N = net(tuple(dims), blob_seed)
    pc = PR.composite_case(seed, n, s, 4, "ordinary" if kind == "plain" else kind, False)
    rng = np.random.default_rng([13, seed])
    idx = rng.integers(1, N.pool.shape[0], n * s)
    keep = (rng.random(n * s) >= 0.2).astype(np.uint8)
    target = pc["raw"][..., 3].astype(np.float64)
    target = np.where(np.abs(target) < NUDGE, np.where(target < 0, -NUDGE, NUDGE), target)
    masked_ray = 1 if n >= 3 and kind != "zero_sigma" else None
    if n >= 3:
        idx[s - 1] = DEAD_ROW
        idx[(n - 1) * s + (s - 1) // 2] = DEAD_ROW
        if s == 1:
            idx[(n - 1) * s] = 1 + seed % (N.pool.shape[0] - 1)
    keep[n * s - 1] = 1
    if masked_ray is not None:
        keep[s:2 * s] = 0
        target[1] = -np.abs(target[1])
    if kind == "zero_sigma":
        keep[:] = 0
    if keep_mode == "null" and kind not in ("zero_sigma",):
        keep = None
    sig = N.sigma[idx] if keep is None else np.where(keep != 0, N.sigma[idx], 0.0)
    if masked_ray is not None and keep is None and kind == "plain":
        masked_ray = None
    if kind in ("plain", "zero_sigma"):
        noise, noise_std = None, 0.0
    else:
        noise, noise_std = (target.reshape(-1) - sig).astype(np.float32).reshape(n, s), 1.0
    d = np.zeros((n, d_stride), np.float32)
    d[:, :3] = pc["d"]
    if d_stride > 3:
        d[:, 3:] = np.nan                                      # a read of the padding columns shows
    g = (rng.standard_normal((n, dims[4])) * 1e-2).astype(np.float32)
    if one_hot is not None:
        g[np.arange(n) != one_hot] = 0.0
    return dict(dims=tuple(dims), blob=N.blob, n=n, s=s, kind=kind, seed=seed, keep_mode=keep_mode, d_stride=d_stride, idx=idx, emb=N.pool[idx], keep=keep, z=pc["z"], d=d,
                noise=noise, noise_std=noise_std, g_rendered=g, masked_ray=masked_ray, one_hot=one_hot, blob_seed=blob_seed,
                tag=tag or f"dims {tuple(dims)} n {n} s {s} {kind} seed {seed} keep {keep_mode} d_stride {d_stride}")


def case_model(c, blob=None, detach_norms=False):
    return model(c["blob"] if blob is None else blob, c["dims"], c["emb"], c["keep"], c["z"], c["d"], c["g_rendered"], c["noise"], c["noise_std"], detach_norms)


def scale_model(c, ref, blob=None):
    """The model whose largest entries are the scales of a comparison: `ref` itself, but at embed = 1 (every gradient exactly zero) the first terms alone."""
    return ref if c["dims"][4] != 1 else case_model(c, blob, detach_norms=True)


def kink_census(c, ref):
    """per_ray_ref.kink_rays on the density that goes through the relu (ref["sigma"], float64): rays with |sigma| < 1e-6 or 1 - alpha within a factor two of the
    1e-10 clamp (the LeRF chain's `om > 1e-10f ? om : 1e-10f`, k_lt_ray)."""
    raw = np.zeros((c["n"], c["s"], 4))
    raw[..., 3] = np.where(ref["sigma"] == 0, -1.0, ref["sigma"])          # an EXACT zero (masked without noise, the dead row) is on the relu's off side in every precision
    return PR.kink_rays(raw, c["z"], c["d"][:, :3])


def compare(c, ref, weights, rendered, g_emb, g_params, scales=None):
    """Error figures of one result against the model `ref` -> dict:
      weights, rendered        largest |error| (weights absolute, rendered per component), kink rays left out; *_rel: of the tensor's largest reference entry
      g_emb                    ray by ray: the ray's largest |error| of the ray's largest reference entry, worst ray (kink rays left out): a wrong ray cannot hide
                               behind a large one; a ray whose reference gradient is exactly zero must be exactly zero
      <tensor>, <tensor>_norm  every parameter-gradient tensor max-wise (of its largest reference entry) and norm-wise
    None for an output that was not asked for.  scales: the model the scales are taken from (scale_model: `ref`, but the first terms alone at embed = 1)."""
    scales = scale_model(c, ref) if scales is None else scales
    n, s = c["n"], c["s"]
    ok = ~kink_census(c, ref)
    out = {}
    for name, got in (("weights", weights), ("rendered", rendered)):
        if got is None:
            continue
        err = np.abs(np.asarray(got, np.float64).reshape(ref[name].shape) - ref[name])[ok]
        assert not np.isnan(err).any(), f"{c['tag']}: NaN in {name}"
        mx = np.abs(ref[name][ok]).max(initial=0.0)
        out[name] = float(err.max(initial=0.0))
        out[name + "_rel"] = out[name] / mx if mx > 0 else out[name]
    if g_emb is not None:
        ge, re = np.asarray(g_emb, np.float64).reshape(n, -1), ref["g_emb"].reshape(n, -1)
        scale = np.abs(scales["g_emb"].reshape(n, -1)).max(1)
        err = np.abs(ge - re).max(1)
        assert not np.isnan(err).any(), f"{c['tag']}: NaN in g_emb"
        assert (err[scale == 0] == 0).all(), f"{c['tag']}: a ray whose reference feature gradient is exactly zero got {err[scale == 0].max():.3e}"
        live = ok & (scale > 0)
        out["g_emb"] = float((err[live] / scale[live]).max(initial=0.0))
    for name, (off, (o_, k_)) in param_slices(c["dims"]).items():
        a, b = np.asarray(g_params, np.float64)[off:off + o_ * k_], ref["g_params"][off:off + o_ * k_]
        sb = scales["g_params"][off:off + o_ * k_]
        mx, nr = np.abs(sb).max(), np.linalg.norm(sb)
        assert not np.isnan(a).any(), f"{c['tag']}: NaN in d {name}"
        if mx == 0:
            assert not a.any(), f"{c['tag']}: d {name} must be exactly zero"
            out[name], out[name + "_norm"] = 0.0, 0.0
        else:
            out[name], out[name + "_norm"] = float(np.abs(a - b).max() / mx), float(np.linalg.norm(a - b) / nr)
    return out


SEED0 = 33000          # a base at which no case below has more than 2 % of its rays on a kink (test_lerf_train_shapes_host asserts it)

SAMPLE_COUNTS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257)
THRESHOLDS = ((3, 24), (16, 16), (15, 17), (255, 16), (64, 64), (256, 16), (257, 17))
MODES = (0, 1, 2, -1)                                                                  # nrf_set_train_gemm; -1: the default (by family: f16x3 for the LeRF head)


def sample_count_specs():
    """(dims, n, s, kind, seed, keep_mode, d_stride) for every s x density kind on the small head; n, keep_mode and d_stride by a seeded draw."""
    rng = np.random.default_rng(4200)
    out = []
    for s in SAMPLE_COUNTS:
        for kind in KINDS:
            out.append((SMALL, int(rng.choice((3, 5))), s, kind, SEED0 + len(out), str(rng.choice(("mask", "null"))), int(rng.choice((3, 8)))))
    return out


def threshold_specs():
    kinds = ("ordinary", "opaque_at", "negative_sigma", "plain", "coincident", "zero_dir", "opaque_first")
    out = []
    for dims in (SMALL, MAIN):
        for i, (n, s) in enumerate(THRESHOLDS):
            out.append((dims, n, s, kinds[i], SEED0 + 500 + len(out), "mask", 3))
    return out


# head shapes: (dims, what it is there for); each at one threshold case below c = 4096 and one at or above
HEAD_SHAPES = (
    ((16, 2, 24, 8, 48), "hidden 24: L.out < 32"),
    ((16, 2, 30, 8, 48), "hidden 30: W % 4 != 0, yo = 0"),
    ((16, 2, 32, 5, 48), "geo 5: yo = 3, geo & 3 != 0"),
    ((16, 2, 32, 8, 48), "geo 8: yo = 3, geo & 3 == 0"),
    ((16, 2, 63, 8, 48), "hidden 63"), ((16, 2, 64, 8, 48), "hidden 64"), ((16, 2, 65, 8, 48), "hidden 65"), ((16, 2, 100, 8, 48), "hidden 100"),
    ((16, 2, 255, 8, 48), "hidden 255"), ((16, 2, 256, 8, 48), "hidden 256"),
    ((16, 2, 257, 8, 48), "hidden 257: Gram refused"),
    ((16, 1, 32, 8, 48), "one layer: Gram refused"),
    ((16, 3, 32, 8, 48), "three layers"),
    ((16, 2, 32, 8, 1), "embed 1"), ((16, 2, 32, 8, 40), "embed 40"), ((16, 2, 32, 8, 257), "embed 257"), ((16, 2, 32, 8, 768), "embed 768"),
    ((3, 2, 32, 8, 48), "in_ch 3"), ((13, 2, 32, 8, 48), "in_ch 13"), ((128, 2, 32, 8, 48), "in_ch 128"),
)
HEAD_SHAPE_SIZES = ((15, 17), (257, 17))
GEO0 = (16, 2, 32, 0, 48)


def head_shape_specs():
    out = []
    for dims, _ in HEAD_SHAPES:
        for n, s in HEAD_SHAPE_SIZES:
            out.append((dims, n, s, "ordinary", SEED0 + 700 + len(out), "mask", 3))
    return out


# LDS bounds
LDS_LIMIT = 60 * 1024
LDS_LAYERWISE = ((16, 2, 256, 8, 40), 3, 1500)                           # (9 s + 9 hd + 2) * 4 > 60 KiB: layer-wise, (7 s + 2 E) * 4 under it
GRAM_S_MAX = (LDS_LIMIT // 4 - 2 - 9 * 32) // 9                          # the largest s in the Gram form at hd = 32
LDS_GRAM = ((16, 2, 32, 8, 48), 3, GRAM_S_MAX)
UNSUPPORTED_S = (LDS_LIMIT // 4 - 2 * 48) // 7 + 1                       # one over (7 s + 2 E) * 4 > 60 KiB at E = 48
# several passes: (dims, n, s, gram form)
PASS_CASES = ((TINY, 2049, 64, 0), (TINY, 4097, 64, 0), (TINY, 4097, 256, 1))
ONE_HOT = (SMALL, 257, 17)                                               # c >= 4096, rays >= 256
UPLOAD = (MAIN, 64, 64)


# ------------------------------------------------------------------------------------------------ the dispatch of lerf_train.hip, restated from the shapes
def max_width(dims):
    return max(max(o, k) for o, k in layer_shapes(dims))


def gram_form(dims, s, gram_on=1):
    """lerf_train_gram(): the library GEMMs are there and the head is bias-free on every build"""
    return bool(gram_on) and dims[1] >= 2 and dims[2] <= 256 and (9 * s + 9 * dims[2] + 2) * 4 <= LDS_LIMIT


def unsupported(dims, s):
    return (7 * s + 2 * dims[4]) * 4 > LDS_LIMIT


def dispatch(dims, n, s, mode=-1, gram_on=1):
    """The paths head_backward_chunk takes for n rays x s samples -> dict."""
    in_ch, nl, hid, geo, emb = dims
    gram = gram_form(dims, s, gram_on)
    shapes = layer_shapes(dims)
    W = max([8] + [v for o, k in shapes[:-1] for v in (o, k)] + [shapes[-1][1]]) if gram else max_width(dims)
    cap = max(1, ((1 << 20) if gram else (1 << 17)) // s)
    passes = 1 if n <= cap else -(-n // cap)
    rays = max(1, n) if n <= cap else -(-n // passes)
    c = rays * s
    m = 2 if mode < 0 else mode
    yo = 3 if (W >= 4 + geo and W % 4 == 0) else 0
    arith = m if (gram and c >= 4096) else 0
    le0_out = shapes[nl][0]
    cat2 = c >= 4096 and m != 0 and le0_out >= 32 and W >= ((yo + 1 + geo + 3) & ~3)
    return dict(gram=gram, W=W, passes=passes, rays=rays, c=c, yo=yo, split_fwd=c >= 256 and m != 0, arith=arith, arith_r=arith if rays >= 256 else 0,
                cat2=("aligned" if (yo == 3 and geo % 4 == 0) else "offset") if cat2 else None, gram_from_packer=gram and hid == 256 and dims == MAIN,
                tail_rays=n - (passes - 1) * rays)


# ------------------------------------------------------------------------------------------------ the language loss
LOSS_N, LOSS_E = (1, 3, 4, 5, 257, 1025), (1, 63, 64, 65, 768)
NAN_ROWS = (3, 4, 255, 256)


def loss_case(n, e, nan="one"):
    """pred, target [n, e] fp32.  Differences of every size either side of delta; row 0 (where e allows) holds |d| exactly at delta, the fp32 number just under and
    just over it, with both signs, on targets of zero (the fp32 difference is exact).  nan: "none" | "one" (a NaN in the target of the middle row) | "edges" (rows 3, 4,
    255, 256 where they exist) | "all" (every row)."""
    rng = np.random.default_rng([14, n, e])
    pred = rng.standard_normal((n, e)).astype(np.float32)
    target = (pred + rng.standard_normal((n, e)) * 1.2).astype(np.float32)
    at = np.float32(DELTA)
    edge = np.array([at, np.nextafter(at, np.float32(0)), np.nextafter(at, np.float32(2)), -at, -np.nextafter(at, np.float32(0)), -np.nextafter(at, np.float32(2))], np.float32)
    k = min(e, edge.size)
    pred[0, :k], target[0, :k] = edge[:k], 0.0
    rows = dict(none=[], one=[n // 2], edges=[r for r in NAN_ROWS if r < n], all=list(range(n)))[nan]
    for r in rows:
        target[r, (r * 7) % e] = np.nan
    return pred, target, rows
