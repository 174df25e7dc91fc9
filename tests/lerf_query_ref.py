"""float64 torch restatement of the LeRF relevancy query (include/nerfpp_hip.h, lerf_query.hip): LeRFImpl::forward (LeRF.cpp:75-110), normalize and the
relevancy of nrf_lerf_relevancy, in two forms --
  direct:      the 768-wide embedding e = W a, normalised, dotted with the prompts;
  projection:  ||W a||^2 = a^T (W^T W) a and q . W a = (W^T q) . a, as the fused kernel computes them, without the 768-wide value."""
import numpy as np
import torch

IN, HID, GEO, EMB = 128, 256, 32, 768


def split_blob(blob, in_ch=IN, hidden=HID, geo=GEO, embed=EMB):
    """blob (checkpoint order) -> (W_s0 [hid, in], W_s1 [1 + geo, hid], W_l0 [hid, geo + in], W_l1 [embed, hid]) as float64 tensors."""
    b = torch.as_tensor(np.asarray(blob, np.float32)).to(torch.float64)
    shapes = [(hidden, in_ch), (1 + geo, hidden), (hidden, geo + in_ch), (embed, hidden)]
    out, o = [], 0
    for r, c in shapes:
        out.append(b[o:o + r * c].reshape(r, c))
        o += r * c
    assert o == b.numel(), (o, b.numel())
    return out


def head(blob, x):
    """(sigma_le [p], a [p, hid] (LE0 output, ReLU), W_l1) of LeRFImpl::forward in float64."""
    w0, w1, l0, l1 = split_blob(blob)
    x = torch.as_tensor(np.asarray(x, np.float32)).to(torch.float64)
    h = torch.relu(x @ w0.T)
    s = h @ w1.T
    a = torch.relu(torch.cat([s[:, 1:], x], dim=1) @ l0.T)
    return s[:, 0], a, l1


def relevancy_from_logits(lp, ln):
    """lp [p], ln [p, q] cosine logits -> [p, 2]: temperature 10, pairwise softmax, the negative the positive does worst against (first on ties); q = 0: zeros."""
    p = lp.shape[0]
    if ln.shape[1] == 0:
        return torch.zeros((p, 2), dtype=torch.float64)
    s0 = torch.sigmoid(10.0 * (lp[:, None] - ln))            # the pair softmax's positive share
    j = torch.argmin(s0, dim=1)                              # torch.argmin: the first minimum
    b0 = s0.gather(1, j[:, None])[:, 0]
    return torch.stack([b0, 1.0 - b0], dim=1)


def _prompts(pos, neg, positive_id):
    q = torch.as_tensor(np.asarray(pos, np.float32)).to(torch.float64).reshape(-1, EMB)[positive_id]
    n = torch.as_tensor(np.asarray(neg, np.float32)).to(torch.float64).reshape(-1, EMB)
    return q, n


def relevancy_direct(blob, x, pos, neg, positive_id=0):
    _, a, l1 = head(blob, x)
    e = a @ l1.T
    e = e / torch.linalg.vector_norm(e, dim=1, keepdim=True).clamp_min(1e-8)
    e = e / torch.linalg.vector_norm(e, dim=1, keepdim=True).clamp_min(1e-8)          # normalize(le(x)): le is LeRFImpl::forward's output, itself normalised
    q, n = _prompts(pos, neg, positive_id)
    return relevancy_from_logits(e @ q, e @ n.T)


def relevancy_projection(blob, x, pos, neg, positive_id=0):
    _, a, l1 = head(blob, x)
    q, n = _prompts(pos, neg, positive_id)
    g = l1.T @ l1                                            # W^T W [hid, hid]
    u = l1.T @ torch.cat([q[None], n], dim=0).T              # U = W^T [q; negs] [hid, 1 + q]
    nrm = torch.sqrt(torch.clamp_min(((a @ g) * a).sum(dim=1), 0.0)).clamp_min(1e-8)
    d = (a @ u) / nrm[:, None]
    return relevancy_from_logits(d[:, 0], d[:, 1:])


def unit_prompts(n, seed):
    """n seeded unit-norm prompt embeddings [n, 768] fp32."""
    r = np.random.default_rng(seed).standard_normal((n, EMB))
    return (r / np.linalg.norm(r, axis=1, keepdims=True)).astype(np.float32)


def locate(rel, sigma, threshold, top_k):
    """LocateQuery's selection on a grid: flat indices of the top_k rel[..., 0] among sigma >= threshold, ties to the lower index."""
    r = np.asarray(rel, np.float64).reshape(-1, 2)[:, 0]
    idx = np.nonzero(np.asarray(sigma).reshape(-1) >= threshold)[0]
    order = sorted(idx.tolist(), key=lambda i: (-r[i], i))
    return np.asarray(order[:top_k], np.int64)
