"""Plain numpy models of the kernels that close a training step (nerfpp_amd/csrc/train.hip: k_huber + k_finish_loss, k_mask_grad, k_tv_loss<F>, k_adam) and the case
lists that tests/test_train_tail_host.py (against the C oracle and the reference's goldens, on the CPU) and tests/test_train_tail_gpu.py (against the kernels) share.

Every model is elementwise float32 arithmetic with one rounding per operation -- numpy's float32 +, -, *, /, sqrt are correctly rounded IEEE operations, as the device's
are in a library built with -ffp-contract=off and no fast-math flag -- and sums in float64.  No library call."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


def ulp32(x):
    """spacing of float32 at |x| (x a float64 number)"""
    return float(np.spacing(np.float32(abs(x))))


# ------------------------------------------------------------------ huber
def huber(pred, target):
    """nrf_huber_loss -> (loss64, mse64, grad32): d and z = |d| in float32; the per-element terms 0.5 z^2 | z - 0.5 and d^2 in float64 from the float32 d (both exact:
    a 24-bit number squared fits 48 bits), summed with math.fsum, divided by count; the gradient in float32 only."""
    pred = np.ascontiguousarray(pred, f32).reshape(-1); target = np.ascontiguousarray(target, f32).reshape(-1)
    count = pred.size
    with np.errstate(all="ignore"):
        d = pred - target
        z = np.abs(d)
        z64, d64 = z.astype(f64), d.astype(f64)
        h = np.where(z < f32(1), 0.5 * z64 * z64, z64 - 0.5)
        q = d64 * d64
        loss64 = math.fsum(h.tolist()) / count
        mse64 = math.fsum(q.tolist()) / count
        norm = f32(1) / f32(count)
        grad = np.where(d < f32(-1), -norm, np.where(d > f32(1), norm, norm * d)).astype(f32)
    return loss64, mse64, grad


HUBER_COUNTS = (1, 63, 64, 65, 255, 256, 257, 131071, 131072, 131073, 393221)      # wave edge, block edge, the 512 x 256 grid cap (a second grid-stride trip), a ragged fourth trip
_ONE = f32(1)
HUBER_PLANTS = (_ONE, -_ONE, np.nextafter(_ONE, f32(0)), np.nextafter(-_ONE, f32(0)), np.nextafter(_ONE, f32(np.inf)), np.nextafter(-_ONE, f32(-np.inf)), f32(0.0), f32(-0.0))


def huber_case(count, seed=0):
    """target in [0, 1), pred = target + U[-3, 3]; the eight branch-boundary differences planted (target 0, so d = pred exactly) at the last min(8, count) elements -- which
    of them lands on the very last element rotates with the count, so all eight do over HUBER_COUNTS -- and once more spread over the array."""
    rng = np.random.default_rng(1000 + seed + count)
    target = rng.random(count, dtype=f32)
    pred = (target + rng.uniform(-3.0, 3.0, count).astype(f32)).astype(f32)
    rot = HUBER_COUNTS.index(count) if count in HUBER_COUNTS else count
    for j in range(min(8, count)):
        target[count - 1 - j] = 0.0; pred[count - 1 - j] = HUBER_PLANTS[(rot + j) % 8]
    if count >= 64:
        for j in range(8):
            i = (j * count) // 8 + j
            target[i] = 0.0; pred[i] = HUBER_PLANTS[j]
    return pred, target


# ------------------------------------------------------------------ sigma mask
def mask_sigma(g_raw, keep, c, src=None):
    """nrf_mask_sigma_grad(_src): column c - 1 of row i becomes +0.0 where keep[i] (keep[src[i]] in the _src form) is zero; nothing else changes (bits included)."""
    g = np.array(g_raw, f32).reshape(-1, c)
    k = np.asarray(keep, np.uint8)
    rows = k[np.asarray(src, np.int64)] if src is not None else k[:g.shape[0]]
    g[rows == 0, c - 1] = f32(0.0)
    return g


MASK_P, MASK_C = (1, 255, 256, 257, 1000), (1, 4, 7)
MASK_KEEPS = ("zeros", "ones", "alternating", "last_false", "true_as_2_and_255")


def mask_grad_buffer(p, c):
    """[p, c] float32 words with distinct bit patterns; NaN (with a payload) and -0.0 in the sigma column and in its neighbours."""
    g = (np.uint32(0x3F000000) + np.arange(p * c, dtype=np.uint32) * np.uint32(37)).view(f32).reshape(p, c).copy()
    gb = g.view(np.uint32)
    for i in range(p):
        kind = i % 5
        if kind == 0: gb[i, c - 1] = 0x7FC00123          # NaN in the sigma column
        elif kind == 1: gb[i, c - 1] = 0x80000000        # -0.0 in the sigma column
        elif kind == 2 and c > 1: gb[i, c - 2] = 0xFFC00456   # NaN left of it
        elif kind == 3 and c > 1: gb[i, 0] = 0x80000000   # -0.0 in the row's first word (right of the previous row's sigma)
    return g


def mask_keep(name, n):
    k = np.zeros(n, np.uint8)
    if name == "ones": k[:] = 1
    elif name == "alternating": k[::2] = 1
    elif name == "last_false": k[:] = 1; k[-1] = 0
    elif name == "true_as_2_and_255": k[:] = np.array([0, 2, 255], np.uint8)[np.arange(n) % 3]
    else: assert name == "zeros", name
    return k


def mask_src_lengths(p):
    """lengths of the keep-by-column array: shorter than p (a single point has no shorter one) and longer"""
    return (p // 2 + 1 if p > 1 else 2, 2 * p + 3)


def mask_src_case(p, m, seed=0):
    """keep by column [m] (values 0, 1, 2, 255) and src [p] int32 into it: repeats, column 0 and column m - 1"""
    rng = np.random.default_rng(77 + 13 * p + m + seed)
    keep_cols = np.array([0, 1, 0, 2, 255, 0], np.uint8)[rng.integers(0, 6, m)]
    src = rng.integers(0, m, p).astype(np.int32)
    src[0] = m - 1
    if p > 1: src[-1] = 0
    if p > 4: src[2] = src[3] = src[1]
    return keep_cols, src


# ------------------------------------------------------------------ TV
def tv(table_level, log2_t, min_vertex, cube, weight):
    """TotalVariationLoss of one level as the reference's tensor formulation (NeRF.h:276-295): hash the (cube + 1)^3 lattice (integers that do not wrap), gather the
    [n, n, n, F] block, three slice differences and their squares in float32, summed in float64, / cube  -> the UNWEIGHTED loss64 (what the reference returns; the library
    adds weight * loss).  grad64 [2^T, F] = the float32 addends g = weight * (2 d) / cube (each operation rounded to float32), +g at u and -g at v, scattered in float64;
    k [2^T, F] = addends per entry, A = sum of |addend| per entry, W = 64-thread waves of a thread-per-vertex launch."""
    t = np.ascontiguousarray(table_level, f32)
    F = t.shape[-1]; n = cube + 1
    ax = [int(min_vertex[a]) + np.arange(n, dtype=np.int64) for a in range(3)]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    rows = (X ^ (Y * 2654435761) ^ (Z * 805459861)) & ((1 << log2_t) - 1)
    E = t.reshape(1 << log2_t, F)[rows]                                    # [n, n, n, F]
    grad = np.zeros((1 << log2_t, F), f64); A = np.zeros_like(grad); k = np.zeros(grad.shape, np.int64)
    cols = np.arange(F)
    total = 0.0
    for a in range(3):
        hi = tuple(slice(1, None) if b == a else slice(None) for b in range(3)); lo = tuple(slice(None, -1) if b == a else slice(None) for b in range(3))
        d = E[hi] - E[lo]                                                  # float32
        total += float((d * d).astype(f64).sum())
        g = ((f32(weight) * (f32(2) * d)) / f32(cube)).astype(f64)
        u, v = rows[hi][..., None], rows[lo][..., None]
        np.add.at(grad, (u, cols), g); np.add.at(grad, (v, cols), -g)
        np.add.at(A, (u, cols), np.abs(g)); np.add.at(A, (v, cols), np.abs(g))
        np.add.at(k, (u, cols), 1); np.add.at(k, (v, cols), 1)
    return dict(loss=total / cube, grad=grad, k=k, A=A, W=-(-n ** 3 // 64))


def tv_loss_budget(W, loss):
    """all terms non-negative; each wave's partial is rounded to float32 once and added by a float atomic (one more rounding, of a running sum <= the total)"""
    return (W + 2) * 2.0 ** -24 * loss


def tv_grad_budget(k, A):
    """k float32 addends accumulated by float atomics in any order: every partial sum is <= A in magnitude"""
    return (k + 1) * 2.0 ** -23 * A


TV_LEVELS, TV_F, TV_T, TV_CUBES = 3, (1, 2, 4, 8), (4, 10, 14), (1, 5, 6, 7, 16)          # cube + 1 cubed: 8, 216, 343 (crosses one block edge), 512 (two blocks), 4913 vertices
TV_BIG = ((1 << 20) + 7, (1 << 21) + 1, (1 << 19) + 5)          # y * 2654435761 and z * 805459861 pass 2^32: the kernel's uint32 products wrap, the model's integers do not
TV_LOSS_PREFILL = 2.5


def _tv_case(F, T, cube, mv=(3, 1, 2), weight=1.0, level=1, table="normal", g_prefill="zero", loss_prefill=0.0):
    return dict(F=F, T=T, cube=cube, mv=tuple(mv), weight=weight, level=level, table=table, g_prefill=g_prefill, loss_prefill=loss_prefill)


# F x log2_t x cube complete at one min_vertex, weight and level; d_loss prefilled with 0 and 2.5 in turn
TV_CASES = [_tv_case(F, T, cube, loss_prefill=TV_LOSS_PREFILL * ((i + j + k) % 2)) for i, F in enumerate(TV_F) for j, T in enumerate(TV_T) for k, cube in enumerate(TV_CUBES)]
TV_CASES += [
    _tv_case(2, 14, 16, mv=(0, 0, 0), level=0),
    _tv_case(2, 14, 7, mv=TV_BIG, weight=0.37, level=2),
    _tv_case(1, 10, 16, mv=TV_BIG, weight=1e-6, level=0),
    _tv_case(4, 4, 5, mv=TV_BIG, weight=0.37, level=2),
    _tv_case(8, 10, 6, mv=(0, 0, 0), weight=1e-6, level=2),
    _tv_case(2, 10, 16, table="repeated"),
    _tv_case(4, 14, 7, table="repeated", weight=0.37, level=0),
    # the level's own slice of d_g_table prefilled with random values: the call accumulates
    _tv_case(1, 4, 5, weight=0.37, g_prefill="random"),
    _tv_case(2, 10, 6, weight=0.37, g_prefill="random"),
    _tv_case(4, 14, 7, weight=0.37, g_prefill="random", mv=TV_BIG),
    _tv_case(8, 4, 16, weight=0.37, g_prefill="random"),
]


def tv_case_id(c):
    mv = "big" if c["mv"] == TV_BIG else "".join(map(str, c["mv"]))
    return f"F{c['F']}-T{c['T']}-cube{c['cube']}-mv{mv}-w{c['weight']:g}-l{c['level']}-{c['table']}-g{c['g_prefill']}-loss{c['loss_prefill']:g}"


def tv_table(c):
    """[3, 2^T, F] float32: random normal, or rows repeated in runs (every row one of five distinct rows: most differences are zero)"""
    rng = np.random.default_rng(500 + 7 * c["F"] + 31 * c["T"] + c["cube"])
    rows = 1 << c["T"]
    if c["table"] == "repeated":
        five = rng.standard_normal((TV_LEVELS, 5, c["F"])).astype(f32)
        return np.ascontiguousarray(five[:, rng.integers(0, 5, rows) * (rng.random(rows) < 0.3), :])
    return rng.standard_normal((TV_LEVELS, rows, c["F"])).astype(f32)


def tv_g_prefill(c):
    """the level's own slice of d_g_table before the call"""
    if c["g_prefill"] == "random":
        return np.random.default_rng(900 + c["F"]).standard_normal((1 << c["T"], c["F"])).astype(f32)
    return np.zeros((1 << c["T"], c["F"]), f32)


def tv_expect(c, table=None):
    """What one nrf_hash_tv_loss call of case c leaves behind, with its budgets: the level slice of d_g_table = prefill + grad (the prefill counts as one more addend),
    d_loss = loss_prefill + weight * loss within the loss budget plus -- where the running sum starts at the prefill -- one float32 ulp of the sum."""
    table = tv_table(c) if table is None else table
    m = tv(table[c["level"]], c["T"], c["mv"], c["cube"], c["weight"])
    pre = tv_g_prefill(c).astype(f64)
    wl = float(f32(c["weight"])) * m["loss"]
    want_loss = c["loss_prefill"] + wl
    return dict(model=m, weighted_loss=wl, want_loss=want_loss, loss_budget=tv_loss_budget(m["W"], wl) + (ulp32(want_loss) if c["loss_prefill"] else 0.0),
                want_grad=pre + m["grad"], grad_budget=tv_grad_budget(m["k"] + (pre != 0), m["A"] + np.abs(pre)), prefill=pre.astype(f32))


# ------------------------------------------------------------------ Adam
def adam(p, g, m, v, lr, b1, b2, eps, t, flags=None, trace=None):
    """nrf_adam_step(_guarded) -> (p, m, v), float32 arrays, each operation rounded once, in the kernel's order; the bias corrections in float64 from the float32 betas.
    Any non-zero flag word: the inputs come back untouched.  trace (a list) receives every intermediate array, for the no-subnormal check of the case lists."""
    p, g, m, v = (np.ascontiguousarray(a, f32) for a in (p, g, m, v))
    if flags is not None and np.any(np.asarray(flags, np.uint32) != 0):
        return p.copy(), m.copy(), v.copy()
    lr, b1, b2, eps = f32(lr), f32(b1), f32(b2), f32(eps)
    bc1 = 1.0 - math.pow(float(b1), float(t)); bc2 = 1.0 - math.pow(float(b2), float(t))
    step, bc2s = f32(float(lr) / bc1), f32(math.sqrt(bc2))
    a1 = m * b1; a2 = g * (f32(1) - b1); m1 = a1 + a2
    c1 = v * b2; gg = g * g; c2 = gg * (f32(1) - b2); v1 = c1 + c2
    s = np.sqrt(v1); sd = s / bc2s; denom = sd + eps
    r = m1 / denom; u = step * r
    p1 = p - u
    if trace is not None:
        trace += [a1, a2, m1, c1, gg, c2, v1, s, sd, denom, r, u, p1]
    return p1.astype(f32), m1.astype(f32), v1.astype(f32)


ADAM_N, ADAM_T = (1, 255, 256, 257, 65537), (1, 2, 10, 1000, 200000)
ADAM_BETAS, ADAM_EPS, ADAM_LR = ((0.9, 0.99), (0.9, 0.999)), (1e-15, 1e-8), (5e-4, 1e-2)
ADAM_CASES = [dict(n=n, t=t, b1=b[0], b2=b[1], eps=e, lr=lr) for n in ADAM_N for t in ADAM_T for b in ADAM_BETAS for e in ADAM_EPS for lr in ADAM_LR]


def adam_state(case, seed=0):
    """p random; m random with |m| >= 1e-6; v random in [1e-12, 1]; g log-uniform in magnitude over 1e-12 .. 1e3 with random sign.  Planted rows: g = m = v = 0 (p must not
    move), g = 0 with non-zero moments, v = 0 with non-zero g -- at both ends of the array; a single-element array takes one of them (or none) in turn.  Every value is
    exactly zero or far from the subnormals: with |g| >= 1e-12 the smallest product, g^2 (1 - beta2), is 1e-27."""
    n = case["n"]
    idx = ADAM_CASES.index(case) if case in ADAM_CASES else 0
    rng = np.random.default_rng(4000 + 17 * idx + seed)
    p = rng.standard_normal(n).astype(f32)
    m = (rng.standard_normal(n) * 0.1).astype(f32)
    m = np.where(np.abs(m) < 1e-6, f32(1e-6), m).astype(f32)
    v = np.maximum(rng.random(n) ** 4, 1e-12).astype(f32)
    g = (np.exp(rng.uniform(math.log(1e-12), math.log(1e3), n)) * rng.choice([-1.0, 1.0], n)).astype(f32)
    def plant(i, kind):
        if kind == 0: g[i] = m[i] = v[i] = 0.0
        elif kind == 1: g[i] = 0.0
        elif kind == 2: v[i] = 0.0
    if n >= 6:
        for kind in range(3):
            plant(kind, kind); plant(n - 1 - kind, kind)
    else:
        plant(0, idx % 4)
    return p, g, m, v


def is_subnormal(a):
    a = np.abs(np.asarray(a, f32))
    return (a > 0) & (a < np.finfo(f32).tiny)
