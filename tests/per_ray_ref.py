"""Float64 restatements of the one-wave-per-ray stages (nerfpp_amd/csrc/composite.hip, k_raw2outputs_bwd of train.hip, k_z_vals of rays.hip) and the seeded cases their
tests share: z_vals (NeRFRenderer.h:393-402), RawToOutputs (:199-282 with TruncExp, CustomOps.cpp:5-15; the weight chain is ray_reg_ref's), its gradient by autograd,
SamplePDF (Sampler.h:6-43) as the plain definition in double and as the reference's own op chain in torch CPU fp32, sort(cat(z, samples)) (NeRFRenderer.h:431).
tests/test_per_ray_host.py pins the C oracle against these on the CPU; tests/test_per_ray_gpu.py holds the kernels to the oracle bit for bit.  No GPU in this file."""
import numpy as np
import torch

from ray_reg_ref import TruncExp, ray_weights, rgb_map, t64, dists_of          # noqa: F401  (TruncExp: the chain's exp, re-exported for the tests)

SINGLE_S = (1, 2, 3, 5, 63, 64, 65, 127, 128, 129, 191, 193, 255, 256)          # one pass: both sides of every 64-lane block edge
MERGED_S = (257, 320, 511, 512)                                                # coarse + importance samples of one ray
RAY_COUNTS = (1, 3, 5, 66)                                                     # four waves per block: 1 and 3 leave waves idle, 5 and 66 end in a partial block
BIG_N = 4097
PDF_NB = (2, 3, 4, 5, 6, 8, 9, 10, 16, 17, 18, 33, 63, 64, 65, 66, 100, 127, 129, 200, 255, 256)      # nb - 1 <, ==, > each of 4, 8, 16
PDF_NS = (1, 5, 64, 65, 128, 256, 512)
SUM_VECS = (0, 4, 8, 16)
FINE_S = (2, 3, 4, 63, 64, 65, 128, 256)
FINE_NS = (1, 5, 64, 128, 256)


# ------------------------------------------------------------------ restatements
def z_vals(near, far, t, lindisp=False):
    """NeRFRenderer.h:397 (near (1 - t) + far t) / :400-401 (safe_inv, eps 1e-8) in float64 -> [n, s]."""
    near, far, t = (np.asarray(a, np.float64) for a in (near, far, t))
    near, far = near[:, None], far[:, None]
    if not lindisp:
        return near * (1.0 - t) + far * t
    inv = lambda x: np.where(np.abs(x) < 1e-8, 1.0 / 1e-8, 1.0 / np.where(x == 0, 1.0, x))
    return inv(inv(near) * (1.0 - t) + inv(far) * t)


def raw2outputs(raw, z, d, white=False, noise=None, noise_std=0.0, sigma_ch=3, grad=False):
    """RawToOutputs in torch float64 -> dict(rgb [n,3], disp, acc, depth [n], weights [n,s]) of tensors (grad: raw is a leaf, returned as out["raw"])."""
    raw, z, d = t64(raw, grad=grad), t64(z), t64(d)
    nz = None if noise is None else t64(noise)
    w, _ = ray_weights(raw[..., sigma_ch], z, d, nz, noise_std)                                   # :234-267
    if sigma_ch != 3:
        rgb = None                                                                                 # RawToLEOutputs' weights part: no colour
    elif nz is None:
        rgb = rgb_map(raw, z, d, white)                                                            # :271, :276-277
    else:
        rgb = (w[..., None] * torch.sigmoid(raw[..., :3])).sum(-2)
        if white:
            rgb = rgb + (1.0 - w.sum(-1, keepdim=True))
    acc = w.sum(-1)                                                                                # :274
    depth = (w * z).sum(-1) / torch.clamp_min(acc, 1e-10)                                          # :272
    disp = 1.0 / torch.clamp_min(depth, 1e-10)                                                     # :273
    return dict(rgb=rgb, disp=disp, acc=acc, depth=depth, weights=w, raw=raw)


def raw2outputs_grad(raw, z, d, g_rgb, white=False, noise=None, noise_std=0.0):
    """d sum(g_rgb * RGBMap) / d raw by autograd through the restatement -> [n, s, c] float64 (columns 4.. carry no gradient: zero)."""
    out = raw2outputs(raw, z, d, white, noise, noise_std, grad=True)
    (g,) = torch.autograd.grad((out["rgb"] * t64(g_rgb)).sum(), out["raw"])
    return g.numpy()


def kink_rays(raw, z, d, noise=None, noise_std=0.0):
    """Rays with a sample at a kink of the chain, where fp32 and fp64 may take different branches (the census of ray_reg_ref.kinks, with the wider clamp band this
    comparison needs): |sigma + noise * std| < 1e-6 (the relu), or 1 - alpha within a factor of two of the 1e-10 clamp."""
    with torch.no_grad():
        sr = t64(np.asarray(raw)[..., 3]) if noise is None else t64(np.asarray(raw)[..., 3]) + t64(noise) * noise_std
        om = torch.exp(-torch.relu(sr) * dists_of(t64(z), t64(d))).numpy()
    return ((sr.abs().numpy() < 1e-6) | ((om > 0.5e-10) & (om < 2e-10))).any(-1)


def sample_pdf_f64(bins, weights, u):
    """SamplePDF as defined, everything in double: -> (samples [n,ns], inds [n,ns] int64, cdf [n,nb]).  u: [ns] shared or [n,ns]."""
    bins, w = np.asarray(bins, np.float64), np.asarray(weights, np.float64) + 1e-8                 # Sampler.h:10
    n, nb = bins.shape
    u = np.broadcast_to(np.asarray(u, np.float64), (n, np.asarray(u).shape[-1]))
    cdf = np.concatenate([np.zeros((n, 1)), np.cumsum(w / w.sum(-1, keepdims=True), -1)], -1)      # :11-13
    inds = np.stack([np.searchsorted(cdf[i], u[i], side="right") for i in range(n)])              # :28
    below, above = np.maximum(inds - 1, 0), np.minimum(inds, nb - 1)                               # :29-30
    cb, ca = np.take_along_axis(cdf, below, 1), np.take_along_axis(cdf, above, 1)
    denom = ca - cb
    denom = np.where(denom < 1e-5, 1.0, denom)                                                     # :37-38
    t = (u - cb) / denom
    bb, ba = np.take_along_axis(bins, below, 1), np.take_along_axis(bins, above, 1)
    return bb + t * (ba - bb), inds.astype(np.int64), cdf


def sample_pdf_aten(bins, weights, u):
    """Sampler.h:10-40 op for op in torch CPU fp32, in the reference's order -> (samples [n,ns] float32, inds [n,ns] int64): the bit-exact anchor of the indices."""
    bins, weights = torch.from_numpy(np.ascontiguousarray(bins, np.float32)), torch.from_numpy(np.ascontiguousarray(weights, np.float32))
    u = torch.from_numpy(np.ascontiguousarray(u, np.float32))
    weights = weights + 1e-8
    pdf = weights / torch.sum(weights, -1, True)
    cdf = torch.cumsum(pdf, -1)
    cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1)
    u = u.expand(cdf.shape[0], u.shape[-1]).contiguous()
    inds = torch.searchsorted(cdf, u, right=True)
    below = torch.max(torch.zeros_like(inds - 1), inds - 1)
    above = torch.min((cdf.shape[-1] - 1) * torch.ones_like(inds), inds)
    inds_g = torch.stack([below, above], -1)
    shape = (inds_g.shape[0], inds_g.shape[1], cdf.shape[-1])
    cdf_g = torch.gather(cdf.unsqueeze(1).expand(shape), 2, inds_g)
    bins_g = torch.gather(bins.unsqueeze(1).expand(shape), 2, inds_g)
    denom = cdf_g[..., 1] - cdf_g[..., 0]
    denom = torch.where(denom < 1e-5, torch.ones_like(denom), denom)
    t = (u - cdf_g[..., 0]) / denom
    return (bins_g[..., 0] + t * (bins_g[..., 1] - bins_g[..., 0])).numpy(), inds.numpy()


def merge_sorted(z, samples):
    """sort(cat(z, samples), -1), stable -> (values [n, s+ns] float32, order [n, s+ns]: the column of cat(z, samples) each value came from)."""
    both = np.concatenate([np.asarray(z, np.float32), np.asarray(samples, np.float32)], -1)
    order = np.argsort(both, axis=-1, kind="stable")
    return np.take_along_axis(both, order, -1), order


def linspace(ns):
    return torch.linspace(0.0, 1.0, ns, dtype=torch.float32).numpy()


# ------------------------------------------------------------------ seeded cases
def _depths(rng, n, s):
    """ascending in [2, 6]: jittered strata"""
    edges = np.linspace(2.0, 6.0, s + 1)
    return (edges[:-1] + rng.uniform(0.0, 1.0, (n, s)) * (edges[1:] - edges[:-1])).astype(np.float32)


def _dirs(rng, n):
    d = rng.standard_normal((n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)


def _dist(z, d):
    """fp32 sigma -> alpha distances (last sample: 1e10), for the cases that set sigma * dist"""
    dz = np.concatenate([np.diff(z, axis=1), np.full((z.shape[0], 1), 1e10, np.float32)], 1)
    return dz * np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)


COMPOSITE_KINDS = ("ordinary", "zero_sigma", "negative_sigma", "opaque_first", "opaque_at", "coincident", "zero_dir")
OPAQUE = 64.0          # sigma * dist of an opaque sample: exp(-64) = 1.6e-28, 1 - alpha = 0 in fp32 and far below the 1e-10 clamp in fp64.  sigma is at least 8 (the last sample's
                       # dist is 1e10), so noise of std 0.5 moves it by a few per cent at most


def composite_case(seed, n, s, c, kind, white, d_stride=3, misalign=False):
    """One compositing batch -> dict(raw [n,s,c], z [n,s], d [n,3], noise [n,s] | None, noise_std, white, g_rgb [n,3], + the arguments).  Every case is composited
    twice, without the sigma noise and with it (the draws are part of every case but zero_sigma, whose point is the exact zero).  Densities as in
    ray_reg_ref.seeded_inputs (N(0.3, 1) times a per-ray gain 10^U(-1, 1.3)), then by kind:
      zero_sigma      raw[..., 3] = 0, no noise (every weight 0; both precisions agree on every branch)
      negative_sigma  raw[..., 3] < 0 (the relu's off side; with noise a few samples cross)
      opaque_first    sample 0 of every ray has sigma * dist = 64 (1 - alpha at the clamp); in every second ray EVERY sample has, so the log-transmittance falls by
                      log(1e-10) = -23.03 per sample through all the 64-sample blocks
      opaque_at       thin fog (gain 0.05) with one opaque sample: at index 63, 64 or s - 1 by ray % 3 (min(.., s - 1))
      coincident      depths in equal pairs (dist = 0 at every even sample); every fourth ray has all depths equal
      zero_dir        every second ray (ray 0 included) has direction 0: every dist is 0"""
    rng = np.random.default_rng(seed)
    z, d = _depths(rng, n, s), _dirs(rng, n)
    raw = rng.standard_normal((n, s, c)).astype(np.float32)
    gain = 10.0 ** rng.uniform(-1.0, 1.3, (n, 1))
    sig = (rng.standard_normal((n, s)) + 0.3) * gain
    noise = rng.standard_normal((n, s)).astype(np.float32)
    g_rgb = (rng.standard_normal((n, 3)) * 1e-2).astype(np.float32)
    if kind == "coincident":
        z[:, 1::2] = z[:, 0:2 * (s // 2):2]
        z[::4] = z[::4, :1]
    if kind == "zero_dir":
        d[::2] = 0.0
    if kind == "zero_sigma":
        sig[:], noise = 0.0, None
    elif kind == "negative_sigma":
        sig = -np.abs(sig) - 0.01
    elif kind == "opaque_first":
        dist = _dist(z, d)
        sig[:, 0] = np.maximum(OPAQUE / dist[:, 0], 8.0)
        sig[1::2] = np.maximum(OPAQUE / dist[1::2], 8.0)
    elif kind == "opaque_at":
        dist = _dist(z, d)
        sig = np.abs(rng.standard_normal((n, s))) * 0.05
        at = np.minimum(np.array([63, 64, s - 1])[np.arange(n) % 3], s - 1)
        sig[np.arange(n), at] = np.maximum(OPAQUE / dist[np.arange(n), at], 8.0)
    raw[..., 3] = sig.astype(np.float32)
    return dict(raw=raw, z=z, d=d, noise=noise, noise_std=0.5, white=white, g_rgb=g_rgb, seed=seed, n=n, s=s, c=c, kind=kind,
                d_stride=d_stride, misalign=misalign, tag=f"seed {seed} {kind} n {n} s {s} c {c} white {int(white)} d_stride {d_stride} misalign {int(misalign)}")


def noise_modes(c):
    """The two compositions of a case -> [(noise | None, noise_std)]: without the draws (nrf_raw2outputs) and, where the case has them, with (nrf_raw2outputs_noise)"""
    return [(None, 0.0)] + ([(c["noise"], c["noise_std"])] if c["noise"] is not None else [])


COMPOSITE_SEED0 = 24200          # a base at which no case has more than 2 % of its rays on a kink (kink_rays, a property of the inputs alone; test_per_ray_host asserts it): with 5
                                 # rays or fewer one ray with sigma * dist in [22.3, 23.7] is already over, and at 2 to 5 samples the distances are long enough for that


def composite_specs():
    """The argument tuples of composite_case for every compositing case: every kind at every sample count, the other layout choices drawn by a seeded generator
    (test_per_ray_host.test_cases_cover asserts that every value and the pairs that select a code path occur), + the one n = 4097 batch."""
    rng = np.random.default_rng(4100)
    out = []
    for s in SINGLE_S + MERGED_S:
        for kind in COMPOSITE_KINDS:
            n = int(rng.choice(RAY_COUNTS[1:] if kind == "opaque_at" else RAY_COUNTS))
            out.append((COMPOSITE_SEED0 + len(out), n, s, int(rng.choice((4, 5, 7))), kind, bool(rng.integers(2)), int(rng.choice((3, 11))), bool(rng.integers(2))))
    out.append((COMPOSITE_SEED0 + len(out), BIG_N, 193, 4, "ordinary", True, 11, False))
    return out


def pdf_case(seed, n, nb, ns):
    """One SamplePDF batch -> dict(bins [n,nb] ascending, weights [n,nb-1] >= 0, u [ns] = linspace(0, 1, ns) (u = 0 and u = 1 both drawn), u_rand [n,ns] in [0, 1)).
    Weights: U(0,1)^3 (peaked).  Batches of at least 66 rays, at every draw count but 5: row 0 all zero (uniform CDF), rows 1, 2, 3 a single spike in the first, the last and
    the 64th bin (min(63, nb - 2)): CDF plateaus, the denom < 1e-5 branch (with one draw, u = 0, the last-bin spike row takes it).  (Not with 5 draws: the draw u = 1 lies
    on the last CDF entry of every row, so test_per_ray_host's share of draws near a CDF entry allows 5-draw batches of a few rays only -- see pdf_specs.)"""
    rng = np.random.default_rng(seed)
    bins = np.sort(rng.uniform(2.0, 6.0, (n, nb)).astype(np.float32), axis=1)
    w = (rng.uniform(0.0, 1.0, (n, nb - 1)) ** 3).astype(np.float32)
    if n >= 66 and ns != 5:
        w[:4] = 0.0
        w[1, 0] = w[2, nb - 2] = w[3, min(63, nb - 2)] = 1.0
    return dict(bins=bins, weights=w, u=linspace(ns), u_rand=rng.uniform(0.0, 1.0, (n, ns)).astype(np.float32), n=n, nb=nb, ns=ns, seed=seed, tag=f"seed {seed} n {n} nb {nb} ns {ns}")


# Seeds replaced so that the ORACLE itself stays under test_per_ray_host's cap on draws left out next to a CDF entry (0.5 % of a case's draws).  The deterministic draws
# hold u = 1, which lies on the last CDF entry of every row: the fp32 CDF ends at 1 - ulp, 1 or 1 + ulp, the index there is nb or nb - 1 (the sample is bins[nb - 1] either
# way), and in a batch of a few rays one such draw is already above the cap; the all-zero row's uniform CDF k / (nb - 1) meets linspace draws j / (ns - 1) the same way.
# Whether a seed passes depends on + and / in IEEE fp32 (the oracle's C loops) and on numpy's float64 sum and cumsum alone -- no libm call, no vector-width-dependent order --
# so a seed that is under the cap here is under it on every host; test_sample_pdf_oracle_vs_float64 asserts the cap for each.
PDF_SEEDS = {5030: 15030, 5043: 15043, 5059: 25059, 5072: 15072, 5099: 135099, 5101: 35101, 5106: 15106, 5107: 15107, 5108: 55108, 5113: 15113, 5120: 15120, 5121: 1295121,
             5135: 15135, 5136: 35136, 5141: 55141, 5142: 15142, 5143: 15143, 5148: 35148, 5149: 35149, 5150: 15150}


def pdf_specs():
    out = []
    for i, nb in enumerate(PDF_NB):
        for j, ns in enumerate(PDF_NS):
            n = RAY_COUNTS[(i + j) % 4]
            if ns == 5 and n == 66:          # see PDF_SEEDS: 66 rows x 5 draws hold 66 draws u = 1, more than the share that may sit on a CDF entry
                n = RAY_COUNTS[i % 3]
            seed = 5000 + len(out)
            out.append((PDF_SEEDS.get(seed, seed), n, nb, ns))
    out.append((5000 + len(out), BIG_N, 129, 128))
    return out


def fine_case(seed, n, s, ns):
    """One fine-depth batch -> dict(z [n,s] ascending, weights [n,s] >= 0, u [ns], u_rand [n,ns]).  s = 2, 3: all-zero weights, and every second ray has all depths equal, so
    the bin edges equal the depths and z and samples tie; batches of at least 3 rays with s >= 4: row 1 has one swapped pair of depths (the exhaustive-rank path)."""
    rng = np.random.default_rng(seed)
    z = _depths(rng, n, s)
    w = (rng.uniform(0.0, 1.0, (n, s)) ** 3).astype(np.float32)
    if s <= 3:
        w[:] = 0.0
        z[::2] = z[::2, :1]
    elif n >= 3:
        a = s // 2
        z[1, [a, a + 1]] = z[1, [a + 1, a]]
    return dict(z=z, weights=w, u=linspace(ns), u_rand=rng.uniform(0.0, 1.0, (n, ns)).astype(np.float32), n=n, s=s, ns=ns, seed=seed, tag=f"seed {seed} n {n} s {s} ns {ns}")


def fine_specs():
    out = []
    for i, s in enumerate(FINE_S):
        for j, ns in enumerate(FINE_NS):
            out.append((6000 + len(out), RAY_COUNTS[(i + j) % 4], s, ns))
    out.append((6000 + len(out), BIG_N, 65, 64))
    return out


def z_vals_case(seed, n, s, stride, lindisp):
    """-> dict(rays [n, stride] with near / far in columns 6, 7 (the rest random), t = linspace(0, 1, s)); lindisp: ray 0 has near = 0 (safe_inv's eps branch)."""
    rng = np.random.default_rng(seed)
    rays = rng.standard_normal((n, stride)).astype(np.float32)
    rays[:, 6] = rng.uniform(0.5, 3.0, n)
    rays[:, 7] = rays[:, 6] + rng.uniform(0.5, 4.0, n).astype(np.float32)
    if lindisp:
        rays[0, 6] = 0.0
    return dict(rays=rays, t=linspace(s), n=n, s=s, stride=stride, lindisp=lindisp, tag=f"seed {seed} n {n} s {s} stride {stride} lindisp {int(lindisp)}")


def z_vals_specs():
    out = []
    for i, s in enumerate(SINGLE_S + MERGED_S):
        out.append((7000 + len(out), RAY_COUNTS[i % 4], s, (8, 11)[i % 2], bool((i // 2) % 2)))
    out.append((7000 + len(out), BIG_N, 193, 11, False))
    return out


def cases(which):
    """The shared generator: which in {"composite", "pdf", "fine", "z_vals"} -> the case dicts, made on the CPU from their seeds."""
    make, specs = dict(composite=(composite_case, composite_specs), pdf=(pdf_case, pdf_specs), fine=(fine_case, fine_specs), z_vals=(z_vals_case, z_vals_specs))[which]
    for spec in specs():
        yield make(*spec)
