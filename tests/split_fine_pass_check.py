"""check_default_split_fine_pass: the check of the default HashNeRF split render against its stage-wise evaluation, shared by tests/test_gpu_parity.py (the default
scenes) and tests/test_hash_shapes_gpu.py (the HashEmbedder grids of tests/hash_shapes_ref.py).  Needs a GPU; imported by GPU tests only."""
import numpy as np
import torch


def host(t):
    return t.detach().cpu().numpy()


def assert_exact(a, b, what=""):
    a = np.asarray(a).reshape(-1); b = np.asarray(b).reshape(-1)
    assert a.size == b.size, (what, a.size, b.size)
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} differ, first at {bad[:5]}: {a[bad[:3]]} vs {b[bad[:3]]}"


def assert_close(a, b, rtol, atol, what=""):
    np.testing.assert_allclose(np.asarray(a).reshape(-1), np.asarray(b).reshape(-1), rtol=rtol, atol=atol, err_msg=what)


def check_default_split_fine_pass(api, sc, res, rays, what):
    """The default HashNeRF split render: sigma-only exact coarse pass that hands the sigma net's output (sigma, geo_feat) to the fine pass; the fine pass runs the
    whole network on the N_importance NEW samples and the colour net alone on its S coarse depths.  Against the stage-wise evaluation (encoder, SH, MLP on explicit
    points) of all S + N_importance depths:
      new samples     == the split-precision MLP, bit for bit (same kernel arithmetic on the same operands);
      coarse depths   sigma == the NRF_PREC_F32 MLP's, bit for bit (the exact fp32 matrix-core chain); rgb within split-precision distance of it."""
    zf = res.Extras["z_fine"]; zc = res.Extras["z_coarse"]
    n, s = zf.shape
    pts = (rays[:, None, 0:3] + rays[:, None, 3:6] * zf[..., None]).reshape(-1, 3)
    emb, keep = sc["embedder"].forward(pts)
    if sc["embedder"].mode == api.L.NRF_HASH_NGP:
        emb[~keep] = 0                  # HashEmbedder fast path: a point outside the box is encoded as zeros (k_hash_ngp_lm); CuHashEmbedder clamps the point instead
    dirs, _ = sc["embeddirs"].forward(rays[:, 8:11].contiguous())
    x = torch.cat([emb, dirs[:, None, :].expand(n, s, dirs.shape[1]).reshape(n * s, -1)], 1).contiguous()
    ref = sc["mlp"].forward(x, api.L.NRF_PREC_F16_SPLIT)
    ref32 = sc["mlp"].forward(x, api.L.NRF_PREC_F32)
    ref[~keep, 3] = 0; ref32[~keep, 3] = 0
    got = host(res.Raw).reshape(-1, 4); ref = host(ref); ref32 = host(ref32)
    coarse = host((zf[:, :, None] == zc[:, None, :]).any(-1))
    # a new sample that lands exactly on a coarse depth cannot be told from it by its depth: leave such pairs out (a handful per tile at most)
    tie = np.zeros_like(coarse)
    eq = host(zf[:, 1:] == zf[:, :-1])
    tie[:, 1:] |= eq; tie[:, :-1] |= eq
    assert tie.sum() <= 1e-4 * tie.size
    assert (coarse & ~tie).sum() + tie.sum() // 2 == n * zc.shape[1], "every coarse depth is among the fine depths"
    tie = tie.reshape(-1); new = ~coarse.reshape(-1) & ~tie; coarse = coarse.reshape(-1) & ~tie
    assert_exact(got[new], ref[new], what + ": new samples == stage-wise split-precision MLP")
    assert_exact(got[coarse, 3], ref32[coarse, 3], what + ": sigma at the coarse depths == NRF_PREC_F32")
    scale = np.abs(ref32[:, :3]).max()
    assert_close(got[coarse, :3], ref32[coarse, :3], rtol=0, atol=2e-5 * scale, what=what + ": rgb at the coarse depths vs the fp32 MLP")
    # ... and not further from fp32 than the full split-precision network is
    assert np.abs(got[coarse, :3] - ref32[coarse, :3]).max() <= 1.5 * np.abs(ref[coarse, :3] - ref32[coarse, :3]).max() + 1e-7 * scale
