"""Float64 restatement of sigma(x) of a hash grid + NeRFSmall scene (scene.make_hash_scene), for the density-gradient tests.

The cell of every level is chosen in fp32 exactly as the encoders choose it (CuHashEmbedder: clamp, ((c - min) / (max - min)) * mul + bias, floor;
HashEmbedder: NeRF.cpp:208-318 with grid = (max - min) / res, vmin = floor(...) * grid + min).  Inside that cell the interpolation weight is a float64 affine
function of x with the derivative the contract names (mul / (max - min), 0 on a clamped axis; 1 / (vmax - vmin)), the corner blend and the sigma net are float64,
and torch autograd gives the gradient.  exact=True (the comparison with the kernel) takes the weights' VALUES from the fp32 arithmetic of the encoders (at the
finest CuHash level the fp32 scaled position carries an absolute error of ~3e-5 in the fraction, which the kernel's derivative sees) and gives the CuHash features
their fp16 value, rounded from the fp32 blend in the kernel's order, with the gradient of the unrounded blend -- so the ReLU masks are the fp32 network's.
exact=False keeps everything a smooth float64 function of x inside the cells (the finite-difference self-check).
"""
import numpy as np
import torch

PRIME_Y, PRIME_Z = 2654435761, 805459861


def _u32(t):
    return t & 0xFFFFFFFF


def _f32(a):
    return np.asarray(a, np.float32)


def level_scales(sc):
    """The embedder's per-level scale as the library holds it (CU: mul_l; NGP: floored resolution)."""
    import ctypes as C
    from nerfpp_amd import _lib as L
    n = sc["cfg"]["n_levels"]
    out = (C.c_float * n)()
    L.check(L.lib().nrf_hash_get_level_scales(sc["embedder"]._h, out))
    return np.array(out[:], np.float32)


class SigmaRef:
    def __init__(self, sc, scales=None, biases=None, num_layers=3, hidden=64, out_dims=4):
        cfg = sc["cfg"]
        self.mode = sc["mode"]
        self.L, self.F, self.T = cfg["n_levels"], cfg["n_feat"], cfg["log2_t"]
        self.bbox = _f32(sc["bbox"]).reshape(6)
        self.scales = _f32(level_scales(sc) if scales is None else scales)
        self.biases = np.zeros((self.L, 3), np.float32) if biases is None else _f32(biases).reshape(self.L, 3)
        tab = np.asarray(sc["table"], np.float32)
        self.table = torch.from_numpy((tab.astype(np.float16) if self.mode == "cu" else tab).astype(np.float64))
        self.primes = None if sc["primes"] is None else np.asarray(sc["primes"], np.int64).reshape(self.L, 3)
        blob = np.asarray(sc["mlp_blob"], np.float64)
        in_ch = self.L * self.F
        self.W, off = [], 0
        for l in range(num_layers):
            o, i = (16 if l == num_layers - 1 else hidden), (in_ch if l == 0 else hidden)
            self.W.append(torch.from_numpy(blob[off:off + o * i].reshape(o, i).copy())); off += o * i
        self.mask_keep = out_dims == 4

    def _cell(self, x32, l):
        """fp32 cell choice of level l: (integer corner [N,3] int64, weight offset [N,3] f64 such that w = a * x + b, slope a [N,3] f64)."""
        mn, mx = self.bbox[:3], self.bbox[3:]
        c = np.maximum(np.minimum(x32, mx), mn)
        inside = x32 == c
        if self.mode == "cu":
            mul = self.scales[l]
            ext = (mx - mn).astype(np.float32)
            q = ((c - mn).astype(np.float32) / ext).astype(np.float32) * mul
            q = (q.astype(np.float32) + self.biases[l]).astype(np.float32)
            fl = np.floor(q)
            slope = np.where(inside, np.float64(mul) / ext.astype(np.float64), 0.0)
            # w = ((clamp(x) - mn) / ext * mul + bias) - fl in float64; on a clamped axis the constant fp32 value
            wconst = (q - fl).astype(np.float64)
            return fl.astype(np.int64), slope, wconst, c, inside
        res = self.scales[l]
        grid = ((mx - mn).astype(np.float32) / res).astype(np.float32)
        fl = np.floor(((c - mn).astype(np.float32) / grid).astype(np.float32))
        vmin = (fl * grid).astype(np.float32) + mn
        vmin = vmin.astype(np.float32)
        vmax = (vmin + grid).astype(np.float32)
        return fl.astype(np.int64), vmin.astype(np.float64), (vmax - vmin).astype(np.float32).astype(np.float64), c, inside

    def features(self, x, exact=True):
        """x [N,3] float64 tensor (requires_grad allowed) -> features [N, L*F] float64, keep [N] bool."""
        x32 = x.detach().numpy().astype(np.float32)
        feats = []
        keep = None
        mn = torch.from_numpy(self.bbox[:3].astype(np.float64))
        for l in range(self.L):
            if self.mode == "cu":
                fl, slope, wconst, c, inside = self._cell(x32, l)
                if exact:
                    w = torch.from_numpy(wconst) + torch.from_numpy(slope) * (x - x.detach())
                else:
                    aff = (x - mn) * torch.from_numpy(slope) + torch.from_numpy(self.biases[l].astype(np.float64)) - torch.from_numpy(fl.astype(np.float64))
                    w = torch.where(torch.from_numpy(inside), aff, torch.from_numpy(wconst) + 0 * x)
            else:
                fl, vmin, span, c, inside = self._cell(x32, l)
                w = (x - torch.from_numpy(vmin)) / torch.from_numpy(span)
            keep = torch.from_numpy(inside.all(axis=1)) if keep is None else keep
            corners = []
            for k in range(8):
                b = np.array([(k >> 2) & 1, (k >> 1) & 1, k & 1], np.int64)
                p = fl + b
                if self.mode == "cu":
                    pr = self.primes[l]
                    hv = _u32(_u32(p[:, 0] * pr[0]) ^ _u32(p[:, 1] * pr[1]) ^ _u32(p[:, 2] * pr[2]))
                    e = hv & ((1 << self.T) - 1)
                    idx = l * (1 << self.T) + e[:, None] * self.F + np.arange(self.F)[None, :]
                else:
                    hv = _u32(_u32(p[:, 0]) ^ _u32(p[:, 1] * PRIME_Y) ^ _u32(p[:, 2] * PRIME_Z)) & ((1 << self.T) - 1)
                    idx = (l * (1 << self.T) + hv)[:, None] * self.F + np.arange(self.F)[None, :]
                corners.append(self.table[torch.from_numpy(idx)])
            f = 0
            for k in range(8):
                wx = w[:, 0] if (k & 4) else 1 - w[:, 0]
                wy = w[:, 1] if (k & 2) else 1 - w[:, 1]
                wz = w[:, 2] if (k & 1) else 1 - w[:, 2]
                f = f + (wx * wy * wz)[:, None] * corners[k]
            if self.mode == "cu" and exact:
                # cu_blend in fp32: three-factor weights, products summed in corner order, one fp16 rounding
                wc = wconst.astype(np.float32)
                s32 = None
                for k in range(8):
                    wx = wc[:, 0] if (k & 4) else np.float32(1) - wc[:, 0]
                    wy = wc[:, 1] if (k & 2) else np.float32(1) - wc[:, 1]
                    wz = wc[:, 2] if (k & 1) else np.float32(1) - wc[:, 2]
                    term = ((wx * wy) * wz)[:, None] * corners[k].numpy().astype(np.float32)
                    s32 = term if s32 is None else (s32 + term).astype(np.float32)
                f = f + (torch.from_numpy(s32.astype(np.float16).astype(np.float64)) - f.detach())
            feats.append(f)
        return torch.cat(feats, 1), keep

    def sigma(self, x, exact=True):
        """-> sigma [N] float64, keep [N], min over layers of |z| / sum |w h| (the closeness of a pre-activation to its ReLU kink)."""
        h, keep = self.features(x, exact)
        kink = torch.full((x.shape[0],), float("inf"), dtype=torch.float64)
        for l, W in enumerate(self.W):
            z = h @ W.T
            if l == len(self.W) - 1:
                sig = z[:, 0]
                break
            mag = h.detach().abs() @ W.abs().T
            kink = torch.minimum(kink, (z.detach().abs() / mag.clamp_min(1e-300)).min(1).values)
            h = torch.relu(z)
        if self.mask_keep:
            sig = torch.where(keep, sig, torch.zeros_like(sig))
        return sig, keep, kink

    def grad(self, pts, exact=True):
        """pts [N,3] (any float array) -> (sigma [N], grad [N,3], kink [N]) as numpy float64."""
        x = torch.tensor(np.asarray(pts, np.float32).astype(np.float64), requires_grad=True)
        sig, keep, kink = self.sigma(x, exact)
        (g,) = torch.autograd.grad(sig.sum(), x)
        return sig.detach().numpy(), g.numpy(), kink.numpy()
