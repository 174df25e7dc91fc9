"""Float64 torch restatement of what the predicted-normals training step differentiates: NeRFSmallImpl::forward with the head (NeRF.cpp:372-408) and the two losses of
NeRF.h:309-326, in this file's own words.  Gradients come from torch autograd on the CPU.  It is the yardstick of tests/test_normal_train_gpu.py and is itself pinned by
tests/test_normal_train_host.py (the compiled reference's golden mlp_small_pn; a case worked out by hand).
"""
import numpy as np
import torch

F64 = torch.float64


def t64(a, grad=False):
    t = torch.tensor(np.asarray(a, np.float64), dtype=F64)
    return t.requires_grad_(True) if grad else t


class SmallPNRef:
    """The three bias-free stacks of a NeRFSmall with use_pred_normal, weights cut from the blob in checkpoint order (sigma_net, color_net, normals_net; W [out][in])."""

    def __init__(self, blob, in_ch=32, in_views=16, n_layers=3, hidden=64, geo=15, n_layers_c=4, hidden_c=64, n_layers_n=3, hidden_n=64):
        self.in_ch, self.in_views, self.geo = in_ch, in_views, geo
        shapes = [((1 + geo) if l == n_layers - 1 else hidden, in_ch if l == 0 else hidden) for l in range(n_layers)]
        shapes += [(3 if l == n_layers_c - 1 else hidden_c, (in_views + geo) if l == 0 else hidden_c) for l in range(n_layers_c)]
        shapes += [(3 if l == n_layers_n - 1 else hidden_n, (1 + geo + in_ch) if l == 0 else hidden_n) for l in range(n_layers_n)]
        blob = np.asarray(blob, np.float64).reshape(-1)
        self.W, self.where, off = [], [], 0
        for o, i in shapes:
            self.W.append(t64(blob[off:off + o * i].reshape(o, i), grad=True))
            self.where.append((off, o * i)); off += o * i
        assert off == blob.size, (off, blob.size)
        self.n_sigma, self.n_color, self.n_normals = n_layers, n_layers_c, n_layers_n
        self.head_offset = self.where[n_layers + n_layers_c][0]

    @staticmethod
    def _stack(h, Ws):
        """-> (output of the last layer (no activation), smallest |pre-activation| of the hidden layers per row)"""
        near = torch.full((h.shape[0],), float("inf"), dtype=F64)
        for k, W in enumerate(Ws):
            z = h @ W.T
            if k == len(Ws) - 1:
                return z, near
            near = torch.minimum(near, z.detach().abs().min(1).values)
            h = torch.relu(z)

    def forward(self, x):
        """x [p, in_ch + in_views] float64 -> (out [p, 7] = [rgb, sigma, normal xyz], kink [p]: the smallest hidden |pre-activation| of the row, over the three nets)"""
        pts, views = x[:, :self.in_ch], x[:, self.in_ch:self.in_ch + self.in_views]
        ns, nc = self.n_sigma, self.n_sigma + self.n_color
        h, k0 = self._stack(pts, self.W[:ns])                                   # column 0 sigma, 1.. geo features
        rgb, k1 = self._stack(torch.cat([views, h[:, 1:]], 1), self.W[ns:nc])
        nrm, k2 = self._stack(torch.cat([h, pts], 1), self.W[nc:])              # the head reads sigma, the geo features and the input points
        return torch.cat([rgb, h[:, :1], nrm], 1), torch.minimum(torch.minimum(k0, k1), k2)

    def grad_blob(self):
        """The weights' .grad in blob order, float64 numpy."""
        return np.concatenate([(w.grad if w.grad is not None else torch.zeros_like(w)).reshape(-1).numpy() for w in self.W])


def density_normals(g):
    """-g / max(|g|, 1e-8): the density normal of a sample from the density gradient g [..., 3]."""
    return -g / g.norm(dim=-1, keepdim=True).clamp_min(1e-8)


def pred_normal_loss(w, nrm, pred):
    """Mean squared difference of the weighted predicted and weighted density normals over every element.  w [n, s], nrm / pred [n, s, 3]."""
    a, b = w[..., None] * pred, w[..., None] * nrm
    return ((a - b) ** 2).mean()


def orientation_loss(w, normals, rays_d):
    """Per ray: sum_i w_i * min(0, normal_i . (-rays_d))^2 -- normals that face away from the camera are penalised.  -> [n]"""
    d = (normals * (-rays_d)[:, None, :]).sum(-1)
    return (w * torch.minimum(torch.zeros_like(d), d) ** 2).sum(-1)


def normal_losses(w, g, pred, rays_d):
    """(L_pn, L_or) of a batch: w [n, s] and g [n, s, 3] are constants (detached), pred [n, s, 3] may require grad, rays_d [n, 3]."""
    w, g = w.detach(), g.detach()
    return pred_normal_loss(w, density_normals(g), pred), orientation_loss(w, pred, rays_d).mean()
