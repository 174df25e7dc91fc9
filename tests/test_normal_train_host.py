"""CPU tests of the predicted-normals training feature: the float64 yardstick (tests/normal_loss_ref.py) is pinned against the compiled reference's golden and a case
worked out by hand, and the library exports and the Trainer's checkpoint layout know the new pieces."""
import ctypes as C

import numpy as np
import torch

from conftest import load_golden
from nerfpp_amd import synth
from normal_loss_ref import SmallPNRef, density_normals, normal_losses, orientation_loss, pred_normal_loss, t64


def test_restated_forward_reproduces_the_compiled_reference(manifest):
    """NeRFSmallImpl::forward with the head, restated in float64, against tests/golden/mlp_small_pn.npz (written by the compiled reference): the bar of the GPU test of
    the same golden (rtol 1e-4, atol 1e-5); seen: max |difference| 1.6e-6 on values up to 6.7, the reference's own fp32 rounding."""
    g = load_golden("mlp_small_pn")
    ref = SmallPNRef(synth.blob_from_manifest(manifest["mlp_small_pn"]), n_layers_c=3)
    with torch.no_grad():
        y, _ = ref.forward(t64(g["x"]))
    y = y.numpy()
    assert y.shape == g["y"].shape == (g["x"].shape[0], 7)
    print("max |restatement - golden| =", np.abs(y - g["y"]).max(), "max |golden| =", np.abs(g["y"]).max())
    np.testing.assert_allclose(y, g["y"], rtol=1e-4, atol=1e-5)


def test_restated_losses_equal_values_worked_out_by_hand():
    """2 rays x 3 samples; a zero weight on each ray, a normal facing away from the camera and one facing it, one zero density gradient."""
    rays_d = t64([[0, 0, -1], [0, 0, -2]])                      # -rays_d = (0,0,1) and (0,0,2)
    w = t64([[0.5, 0.0, 0.25], [1.0, 0.5, 0.0]])
    pred = t64([[[0, 0, 1], [5, 5, -5], [0, 0, -2]], [[1, 0, -0.5], [0, 1, 0.5], [7, 7, 7]]], grad=True)
    g = t64([[[0, 0, -2], [1, 1, 1], [0, 3, 0]], [[0, 0, 0], [-4, 0, 0], [1, 2, 3]]])
    nrm = density_normals(g)
    assert np.array_equal(nrm[0, 0].numpy(), [0, 0, 1]) and np.array_equal(nrm[0, 2].numpy(), [0, -1, 0]) and np.array_equal(nrm[1, 1].numpy(), [1, 0, 0])
    assert np.array_equal(nrm[1, 0].numpy(), [0, 0, 0])        # |g| = 0: -0 / 1e-8
    # orientation: ray 0: sample 0 faces the camera (dot 1 -> 0), sample 1 has w = 0, sample 2 faces away (dot -2 -> 0.25 * 4 = 1); ray 1: dot -1 -> 1 * 1, dot 1 -> 0, w = 0
    assert np.array_equal(orientation_loss(w, pred, rays_d).detach().numpy(), [1.0, 1.0])
    # pred-normal: (0,0): 0.5 * ((0,0,1) - (0,0,1)) = 0;  (0,2): 0.25 * ((0,0,-2) - (0,-1,0)) = (0, .25, -.5) -> .3125;  (1,0): 1 * (1,0,-.5) -> 1.25;
    # (1,1): 0.5 * ((0,1,.5) - (1,0,0)) = (-.5,.5,.25) -> .5625;  the two w = 0 samples: 0.  Mean over 2 * 3 * 3 elements
    assert abs(float(pred_normal_loss(w, nrm, pred).detach()) - (0.3125 + 1.25 + 0.5625) / 18.0) < 1e-15
    l_pn, l_or = normal_losses(w, g, pred, rays_d)
    assert abs(float(l_pn.detach()) - 2.125 / 18.0) < 1e-15 and float(l_or.detach()) == 1.0
    (l_pn + l_or).backward()
    gp = pred.grad.numpy()
    assert np.array_equal(gp[0, 1], [0, 0, 0]) and np.array_equal(gp[1, 2], [0, 0, 0])          # w = 0: no gradient
    # (0,2): d L_pn = 2 * w * diff / 18 = 2 * .25 * (0,.25,-.5) / 18;  d L_or = (1/2) * w * 2 * dot * (-rays_d) = .5 * .25 * 2 * (-2) * (0,0,1)
    np.testing.assert_allclose(gp[0, 2], np.array([0, 0.125, -0.25]) / 18.0 + np.array([0, 0, -0.5]), rtol=0, atol=1e-15)
    np.testing.assert_allclose(gp[0, 0], [0, 0, 0], rtol=0, atol=0)


def test_new_entries_are_declared_and_the_checkpoint_layout_names_the_head():
    from nerfpp_amd import _lib as L
    for name in ("nrf_normal_losses", "nrf_normal_losses_workspace_bytes", "nrf_mlp_backward_pn", "nrf_mlp_backward_pn_workspace_bytes"):
        assert name in L.SYMBOLS
        assert hasattr(C.CDLL(L.LIB_PATH), name), name
    assert L.lib().nrf_normal_losses_workspace_bytes(C.c_int64(257), 64) == ((257 * 64 + 255) // 256) * 16
    # Trainer._param_layout (what SaveCheckpoint / LoadCheckpoint and the Adam moments are cut by) covers the head's three matrices, in the reference's registration order
    from nerfpp_amd.train import Trainer

    class _T:
        has_table = True
    d = L.MlpSmallDesc(32, 16, 3, 64, 15, 4, 64, 1, 3, 64)
    n = int(L.lib().nrf_mlp_small_param_count(C.byref(d)))
    t = _T()
    t.embedder = type("E", (), dict(Log2HashmapSize=4, NFeaturesPerLevel=2, mode=L.NRF_HASH_NGP, NLevels=2, name="embedder"))()
    t.mlp = type("M", (), dict(desc=d))()
    t.blob = torch.zeros(n)
    _, mlp = Trainer._param_layout(t)
    assert [m[0] for m in mlp][-3:] == [f"model_normals_net_{l}.weight" for l in range(3)] and [m[2] for m in mlp][-3:] == [(64, 48), (64, 64), (3, 64)]
    assert mlp[-1][1] + 3 * 64 == n
