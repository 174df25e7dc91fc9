"""Cases, inputs and the expected host dispatch of the level-major hash-grid encoders (tests/test_hash_shapes_host.py checks this module on the CPU,
tests/test_hash_shapes_gpu.py runs the kernels on the same cases).  Plain numpy; nothing here touches the GPU or the library.

dispatch() restates, from a grid's shape alone, what the host code decides: hash_fast_prepare's bake (nerfpp_amd/csrc/hash_fast.hip: a byte budget, 4 x 4 tiles of
floor(level_scale) + 2 vertices), launch_hash_lm's instance choice (coarse / fine split, levels per thread, the straight-line baked instances, 32- or 64-bit
addressing per baked level, 32- or 64-bit stores), launch_hash_ngp_lm's 4 + 1 split and encode.hip's routing of F != 2 and L < 8 grids to k_hash_cu_lmf.  The
level scales are the oracle's (O.hash_cu_scales, O.hash_ngp_resolutions) or the case's injected ones, never the library's.

ref_hash_cu() / ref_hash_ngp() are numpy float32 restatements of the two encoders, one rounding per operation in the reference's own order
(CuHashEmbedder.cu:40-100 behind CuHashEmbedder.cpp:92-94; NeRF.cpp:208-318), written independently of oracle/nerf_oracle.c: the host tests hold the C oracle to
them bit for bit on every case, so a bias, a non-cubic box or an injected scale has a second statement besides the oracle's."""
import functools
from collections import namedtuple

import numpy as np

from nerfpp_amd import synth
from nerfpp_amd.scene import CU_PRIMES, LEGO_BBOX
from oracle import capi as O

ALL = 1 << 40                     # a budget no grid here reaches: every level is baked unless the 2^30-entry stop or a bias forbids it
NONCUBIC = np.array([-0.7, 0.2, -3.0, 1.9, 0.9, 1.1], np.float32)          # off-centre, three different extents, the origin outside
MAX_LEVELS = 32                   # NRF_MAX_LEVELS

Case = namedtuple("Case", "name mode L F T base finest bbox biases scales budget why")


def _biases(seed, L, lo, span):
    """[L, 3] float32 in [lo, lo + span)"""
    return (np.float32(lo) + np.float32(span) * synth.synth_u01(seed, L * 3)).astype(np.float32).reshape(L, 3)


def smallest_scale_on_64bit_path():
    """the smallest integer level scale whose image leaves the 32-bit form: nby * nby * dz >= 2^24 with dz = scale + 2, nby = ceil(dz / 4)"""
    s = 1
    while ((s + 2 + 3) // 4) ** 2 * (s + 2) < (1 << 24):
        s += 1
    return s


SCALE_64 = smallest_scale_on_64bit_path()          # 643: dim 645, nby 162; 642 -> dim 644, nby 161, 161 * 161 * 644 < 2^24
SCALES_INTEGERS = np.array([1.0, 1.5, 2.0, 3.0, 3.999, 5.0, 7.25, 8.0, 11.5, 16.0, 17.0, 23.75, 32.0, 40.5, 63.0, 64.0], np.float32)
SCALES_64BIT = np.array([2.0, 2.5, 3.25, 4.0, 5.5, 6.0, 7.75, 9.0, 10.5, 12.0, 13.25, 15.0, 16.5, 18.0, 20.0, SCALE_64], np.float32)


def _cu(name, L, T, base, finest, why, F=2, bbox=LEGO_BBOX, biases=None, scales=None, budget=ALL):
    return Case(name, "cu", L, F, T, base, finest, np.asarray(bbox, np.float32), biases, scales, budget, why)


def _ngp(name, base, finest, T, why, bbox=LEGO_BBOX, budget=ALL):
    return Case(name, "ngp", 16, 2, T, base, finest, np.asarray(bbox, np.float32), None, None, budget, why)


L16 = dict(L=16, T=10, base=4, finest=64)          # the cheap twin of the default scene (16 levels, 16..512, T 19)


def _through(k, minus):
    """the budget that ends exactly with level k of the L16 grid (every level baked up to and including k), minus `minus` bytes"""
    d = dispatch(_cu("tmp", why="", **L16), ALL)
    return int(np.cumsum(d["entries"])[k]) * 16 - minus


def _cases():
    c = [
        _cu("cu-L16", why="12 + 2, both straight-line instances", **L16),
        _cu("cu-L8", 8, 8, 4, 32, "lc 4: coarse 4 per thread generic, fine straight-line 2 per thread"),
        _cu("cu-L9", 9, 9, 3, 48, "fine count 5: fine 1 per thread"),
        _cu("cu-L12", 12, 8, 4, 64, "lc 8"),
        _cu("cu-L20", 20, 10, 2, 64, "lc 12 with 8 fine levels"),
        _cu("cu-L24", 24, 7, 2, 64, "lc 16: falls back to 4 per thread"),
        _cu("cu-L32", 32, 6, 2, 64, "lc 24: two groups of 12 on grid.y; NRF_MAX_LEVELS"),
        _cu("cu-L16-budget-through-5", why="budget == bytes through level 5 (coarse range): level 5 baked; 4 + 1 generic, baked and hashed levels in one launch", budget=_through(5, 0), **L16),
        _cu("cu-L16-budget-through-5-less-1", why="one byte less: level 5 hashed", budget=_through(5, 1), **L16),
        _cu("cu-L16-budget-through-13", why="budget == bytes through level 13 (fine range): 12 + 2 generic, the fine launch mixed", budget=_through(13, 0), **L16),
        _cu("cu-L16-budget-through-13-less-1", why="one byte less: level 13 hashed", budget=_through(13, 1), **L16),
        _cu("cu-L16-budget-0", why="nothing baked: 4 + 1 generic, every level hashed", budget=0, **L16),
        _cu("cu-L16-bias", why="non-zero biases in [0, 1): no dense image, every level hashed with q + bias", biases=_biases(901, 16, 0.0, 1.0), **L16),
        _cu("cu-L16-box", why="off-centre, non-cubic box", bbox=NONCUBIC, **L16),
        _cu("cu-L16-T4", 16, 4, 4, 64, "local_size 16: the level-offset quirk at its smallest"),
        _cu("cu-L16-T5", 16, 5, 4, 64, "local_size 32"),
        _cu("cu-L16-scales-integers", why="injected level scales with exact integers and the minimum 1.0 (dim 3, one tile)", scales=SCALES_INTEGERS, **L16),
        _cu("cu-L16-scales-64bit", why="injected level scales whose last level is the smallest on the 64-bit addressing path: straight false, one level through pointer loads",
            scales=SCALES_64BIT, **L16),
        _cu("lmf-L2-F1", 2, 4, 2, 8, "k_hash_cu_lmf<1, 1>", F=1),
        _cu("lmf-L5-F1-bias-box", 5, 6, 3, 24, "k_hash_cu_lmf<1, 1> with biases in the reference's own range (rand * 1000 + 100, CuHashEmbedder.cpp:56) and the non-cubic box", F=1,
            bbox=NONCUBIC, biases=_biases(902, 5, 100.0, 1000.0)),
        _cu("lmf-L3-F4", 3, 8, 2, 20, "k_hash_cu_lmf<4, 1>", F=4),
        _cu("lmf-L7-F2", 7, 10, 4, 48, "k_hash_cu_lmf<2, 1>: F = 2 below the fast path's L >= 8 (an image is baked and not read)"),
        _cu("lmf-L16-F8", 16, 12, 4, 64, "k_hash_cu_lmf<8, 1>", F=8),
        _ngp("ngp-4-64", 4, 64, 12, "k_hash_ngp_lm 4 + 1, every level baked"),
        _ngp("ngp-2-30", 2, 30, 10, "floor()ed resolutions repeat"),
        _ngp("ngp-16-2048", 16, 2048, 14, "the entries >= 2^30 stop leaves the finest levels hashed"),
        _ngp("ngp-box", 4, 64, 12, "non-cubic box", bbox=NONCUBIC),
        _ngp("ngp-budget-0", 4, 64, 12, "nothing baked: every level hashed", budget=0),
    ]
    return c


# ------------------------------------------------------------------ the host's decisions
def level_scales(cfg):
    if cfg.scales is not None:
        return np.asarray(cfg.scales, np.float32)
    return O.hash_cu_scales(cfg.L, cfg.base, cfg.finest) if cfg.mode == "cu" else O.hash_ngp_resolutions(cfg.L, cfg.base, cfg.finest)


def dispatch(cfg, budget=None, pstride=None):
    """-> dict: scales, dim / nby / entries per level, n_baked, baked_bytes, lookup per level ('straight', 'baked32', 'baked64', 'hashed'), path ('lm', 'lmf', 'ngp'),
    lc, coarse_lpt, fine_lpt, straight, coarse / fine (the kernel instances), coarse_kind / fine_kind ('baked', 'hashed', 'mixed'), store32 (for `pstride`)"""
    budget = cfg.budget if budget is None else budget
    L, ngp = cfg.L, cfg.mode == "ngp"
    scales = level_scales(cfg)
    dim = np.floor(scales).astype(np.int64) + 2
    nby = (dim + 3) // 4
    entries = nby * nby * dim * 16
    entry_bytes = 32 if ngp else 16
    zero_bias = cfg.biases is None or not np.any(np.asarray(cfg.biases) != 0)
    nb, total = 0, 0
    if cfg.F == 2 and (ngp or zero_bias):
        for l in range(L):
            if (total + int(entries[l])) * entry_bytes > budget or int(entries[l]) >= (1 << 30):
                break
            total += int(entries[l]); nb = l + 1
    a32 = [int(nby[l]) ** 2 * int(dim[l]) < (1 << 24) for l in range(L)]
    out = dict(scales=scales, dim=dim, nby=nby, entries=entries, n_baked=nb, baked_bytes=total * entry_bytes, a32=a32, store32=None)
    lookup = [("baked32" if a32[l] else "baked64") if l < nb else "hashed" for l in range(L)]
    lc = (L * 3 // 4) & ~3
    if ngp:
        out.update(path="ngp", lc=lc, coarse_lpt=4, fine_lpt=1, straight=False, coarse="k_hash_ngp_lm<4>", fine="k_hash_ngp_lm<1>", lookup=["baked" if l < nb else "hashed" for l in range(L)])
    elif cfg.F == 2 and L >= 8:
        baked = nb >= lc
        clpt = 12 if baked and lc % 12 == 0 else 4
        flpt = 2 if baked and (L - lc) % 2 == 0 else 1
        straight = baked and nb == L and all(a32) and zero_bias
        coarse = "k_hash_cu_lm<1, 0, 4>" if clpt == 4 else ("k_hash_cu_lm<1, 0, 12, 3>" if straight else "k_hash_cu_lm<1, 0, 12>")
        fine = "k_hash_cu_lm<1, 0, 2, 2>" if straight and flpt == 2 else ("k_hash_cu_lm<1, 0, 1>" if flpt == 1 else "k_hash_cu_lm<1, 0, 2>")
        for l in range(L):          # the levels served by a straight-line instance (the fourth template argument, DENSE > 0)
            if straight and (clpt == 12 if l < lc else flpt == 2):
                lookup[l] = "straight"
        out.update(path="lm", lc=lc, coarse_lpt=clpt, fine_lpt=flpt, straight=straight, coarse=coarse, fine=fine, lookup=lookup)
        if pstride is not None:
            out["store32"] = L * pstride * 4 < (1 << 32)
    else:
        out.update(path="lmf", lc=0, coarse_lpt=None, fine_lpt=1, straight=False, coarse=None, fine="k_hash_cu_lmf<%d, 1>" % cfg.F, lookup=["hashed"] * L)
    kind = lambda ls: None if not ls else ("hashed" if all(v == "hashed" for v in ls) else ("mixed" if any(v == "hashed" for v in ls) else "baked"))
    out.update(coarse_kind=kind(out["lookup"][:out["lc"]]), fine_kind=kind(out["lookup"][out["lc"]:]))
    return out


def held_bytes(held, need):
    """hash_fast_prepare keeps an image that is large enough and not more than twice too large: nrf_hash_memory_bytes reports the ALLOCATION, which equals
    dispatch()'s baked_bytes on a handle's first bake and follows this rule afterwards"""
    if need == 0:
        return 0
    return need if held < need or held // 2 > need else held


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
CU_CASES = [c for c in CASES if c.mode == "cu"]
NGP_CASES = [c for c in CASES if c.mode == "ngp"]
case_id = lambda c: c.name


# ------------------------------------------------------------------ inputs
KINDS = ("inside", "outside", "on a face", "corners and centre", "negative zero", "coarsest lattice", "finest lattice")


def points(cfg, n=6000, seed=1):
    """-> (x [n', 3] float32, {kind: slice}); n' is within a few points of n.  Every kind is one contiguous slice, so a failing index names its kind."""
    f = np.float32
    mn, mx = cfg.bbox[:3].astype(f), cfg.bbox[3:].astype(f)
    ext, ctr = (mx - mn).astype(f), ((mx + mn) * f(0.5)).astype(f)
    u = lambda k, m: synth.synth_u01(seed * 100 + k, m * 3).reshape(m, 3)
    inside = lambda k, m: (mn + ext * u(k, m)).astype(f)
    sc = level_scales(cfg)
    parts = []
    parts.append(("inside", inside(1, int(n * 0.4))))
    parts.append(("outside", (ctr + (inside(2, int(n * 0.2)) - ctr) * f(1.3)).astype(f)))
    m = int(n * 0.15)
    face = inside(3, m)
    pick = synth.synth_u32(seed * 100 + 4, m)
    ax, hi = (pick % np.uint32(3)).astype(np.int64), ((pick >> np.uint32(8)) & np.uint32(1)).astype(bool)
    face[np.arange(m), ax] = np.where(hi, mx[ax], mn[ax])
    parts.append(("on a face", face))
    parts.append(("corners and centre", np.stack([mn, mx, ctr]).astype(f)))
    m = int(n * 0.03)
    nz = inside(5, m)
    pick = synth.synth_u32(seed * 100 + 6, m) % np.uint32(7) + np.uint32(1)          # which coordinates become -0.0: never none
    for a in range(3):
        nz[((pick >> np.uint32(a)) & np.uint32(1)).astype(bool), a] = f(-0.0)
    parts.append(("negative zero", nz))
    for name, mul, k in (("coarsest lattice", sc[0], 7), ("finest lattice", sc[-1], 8)):
        m = int(n * 0.11)
        cells = f(np.floor(mul))
        kk = np.floor(u(k, m) * (cells + f(1.0))).astype(f)          # 0 .. floor(mul), the far face included
        parts.append((name, (mn + kk * ext / cells).astype(f)))
    x = np.ascontiguousarray(np.concatenate([p for _, p in parts]), f)
    kinds, at = {}, 0
    for name, p in parts:
        kinds[name] = slice(at, at + p.shape[0]); at += p.shape[0]
    return x, kinds


def kind_of(kinds, i):
    return next(k for k, s in kinds.items() if s.start <= i < s.stop)


def table_of(cfg, seed=77):
    """fp32 master table in the mode's parameter layout: cu [L * 2^T, F], ngp [L][2^T][F]"""
    return synth.synth_sym(seed + cfg.L, (cfg.L * (1 << cfg.T) * cfg.F,), np.float32(0.5))


def primes_of(cfg):
    return np.array(CU_PRIMES[:3 * cfg.L], np.int32)


def local_size_of(cfg):
    return ((1 << cfg.T) >> 4) << 4


def oracle_cu(cfg, x, table=None, scales=None):
    """O.hash_cu on the case's grid -> (features [p, L * F] float32 holding fp16 values, keep [p] bool)"""
    table = table_of(cfg) if table is None else table
    ls = local_size_of(cfg)
    bias = np.zeros((cfg.L, 3), np.float32) if cfg.biases is None else cfg.biases
    return O.hash_cu(x, O.f32_to_f16(table), primes_of(cfg), np.arange(cfg.L, dtype=np.int32) * ls, np.full(cfg.L, ls, np.int32), bias, cfg.bbox,
                     level_scales(cfg) if scales is None else scales, cfg.L, cfg.F)


def oracle_ngp(cfg, x, table=None):
    return O.hash_ngp(x, table_of(cfg) if table is None else table, cfg.bbox, cfg.L, cfg.F, cfg.T, cfg.base, cfg.finest)


@functools.lru_cache(maxsize=None)
def expected(name):
    """the case's points and the oracle's answer on them, computed once and shared: (x, kinds, features [p, L * F] float32, keep [p] bool) -- treat as read-only"""
    cfg = BY_NAME[name]
    x, kinds = points(cfg)
    emb, keep = oracle_cu(cfg, x) if cfg.mode == "cu" else oracle_ngp(cfg, x)
    for a in (x, emb, keep):
        a.setflags(write=False)
    return x, kinds, emb, keep


def f16_bits(emb):
    """fp32 array holding fp16 values -> their fp16 bit patterns (uint16)"""
    h = np.asarray(emb, np.float32).astype(np.float16)
    assert np.array_equal(h.astype(np.float32).view(np.uint32), np.asarray(emb, np.float32).view(np.uint32)), "not fp16 values"
    return h.view(np.uint16)


def level_major(emb, L, F):
    """[p, L * F] -> [L, p, F]"""
    return np.ascontiguousarray(emb.reshape(-1, L, F).transpose(1, 0, 2))


# ------------------------------------------------------------------ independent restatements (numpy float32, one rounding per operation)
def ref_hash_cu(cfg, x, table=None, scales=None):
    """CuHashEmbedder.cpp:92-94 (keep mask, clamp) and CuHashEmbedder.cu:40-100, statement by statement -> (features [p, L * F] float32 holding fp16 values, keep)"""
    f, u32 = np.float32, np.uint32
    x = np.asarray(x, f).reshape(-1, 3)
    mn, mx = cfg.bbox[:3].astype(f), cfg.bbox[3:].astype(f)
    table = np.asarray(table_of(cfg) if table is None else table, f).astype(np.float16)          # the fp32 master cast once (.cu:257)
    scales = level_scales(cfg) if scales is None else np.asarray(scales, f)
    primes = primes_of(cfg).astype(np.int64).astype(u32).reshape(cfg.L, 3)
    ls = u32(local_size_of(cfg))
    xc = np.maximum(np.minimum(x, mx), mn)
    keep = (x == xc).all(1)
    out = np.empty((x.shape[0], cfg.L, cfg.F), f)
    one = f(1.0)
    for l in range(cfg.L):
        pt = (xc - mn) / (mx - mn) * scales[l]                                                    # .cu:44-46: subtract, divide, multiply
        if cfg.biases is not None:
            pt = pt + cfg.biases[l].astype(f)                                                       # .cu:61-63
        else:
            pt = pt + f(0.0)
        fl = np.floor(pt)
        pos = fl.astype(np.int64).astype(u32)                                                       # .cu:66-68
        a, b, c = (pt - fl).T                                                                       # .cu:79-81
        pool = table[l * int(ls):]                                                                  # .cu:54: an ELEMENT offset, rows F wide from there
        acc = None
        for dx, dy, dz in ((0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)):          # .cu:70-77, :83-90, :96-99 in their order
            h = (((pos[:, 0] + u32(dx)) * primes[l, 0]) ^ ((pos[:, 1] + u32(dy)) * primes[l, 1]) ^ ((pos[:, 2] + u32(dz)) * primes[l, 2])) % ls
            w = ((a if dx else one - a) * (b if dy else one - b)) * (c if dz else one - c)
            rows = h.astype(np.int64)[:, None] * cfg.F + np.arange(cfg.F)[None, :]
            term = w[:, None] * pool[rows].astype(f)
            acc = term if acc is None else acc + term
        out[:, l, :] = acc.astype(np.float16).astype(f)                                             # (T) of .cu:95, returned as fp32 (.cu:274)
    return out.reshape(x.shape[0], cfg.L * cfg.F), keep


def ngp_resolutions(L, base, finest):
    """NeRF.cpp:251, :309: b = float(exp((ln finest - ln base) / (L - 1))); res_l = floor(float(base * pow(b, l)))"""
    b = np.float32(np.exp((np.log(np.float64(finest)) - np.log(np.float64(base))) / np.float64(L - 1)))
    return np.array([np.floor(np.float32(np.float64(base) * np.power(np.float64(b), np.float64(l)))) for l in range(L)], np.float32)


def ref_hash_ngp(x, table, bbox, L, F, T, base, finest):
    """HashEmbedderImpl::forward, NeRF.cpp:208-318 -> (features [p, L * F] float32, keep)"""
    f = np.float32
    x = np.asarray(x, f).reshape(-1, 3)
    bbox = np.asarray(bbox, f)
    mn, mx = bbox[:3], bbox[3:]
    table = np.asarray(table, f).reshape(L, 1 << T, F)
    res = ngp_resolutions(L, base, finest)
    xc = np.maximum(np.minimum(x, mx), mn)
    keep = (x == xc).all(1)
    out = np.empty((x.shape[0], L, F), f)
    one = f(1.0)
    for l in range(L):
        grid = (mx - mn) / res[l]
        idx = np.floor((xc - mn) / grid).astype(np.int64)
        vmin = idx.astype(f) * grid + mn
        vmax = vmin + grid
        w = (x - vmin) / (vmax - vmin)                                                              # the UNCLAMPED point (NeRF.cpp:311)
        e = []
        for c in range(8):                                                                          # corner c = 4 dx + 2 dy + dz
            cx, cy, cz = idx[:, 0] + ((c >> 2) & 1), idx[:, 1] + ((c >> 1) & 1), idx[:, 2] + (c & 1)
            h = (cx ^ (cy * np.int64(2654435761)) ^ (cz * np.int64(805459861))) & np.int64((1 << T) - 1)
            e.append(table[l][h])
        wx, wy, wz = w[:, 0:1], w[:, 1:2], w[:, 2:3]
        c00 = e[0] * (one - wx) + e[4] * wx
        c01 = e[1] * (one - wx) + e[5] * wx
        c10 = e[2] * (one - wx) + e[6] * wx
        c11 = e[3] * (one - wx) + e[7] * wx
        c0 = c00 * (one - wy) + c10 * wy
        c1 = c01 * (one - wy) + c11 * wy
        out[:, l, :] = c0 * (one - wz) + c1 * wz
    return out.reshape(x.shape[0], L * F), keep
