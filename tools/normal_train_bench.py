"""Time the training step of a CuHash scene + NeRFSmall with the predicted-normals head on one MI355X: 16 384 rays x 64 samples, coarse only, NRF_PREC_F32, once with both
normal-loss weights 0 (the head is carried but not trained) and once with both non-zero (density gradient + nrf_normal_losses + nrf_mlp_backward_pn), and
nrf_density_grad alone on the same 2^20 points.

Warm-up first, then hipEvent timing of each step and the median of the repeats (one JSON line on stdout; --out also writes it to a file).
    python tools/normal_train_bench.py [--rays 16384] [--steps 20] [--warmup 5] [--only a|b] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), ms


def head_scene(L, M, S, synth):
    sc = S.make_hash_scene(mode="cu")
    d = L.MlpSmallDesc(32, 16, 3, 64, 15, 4, 64, 1, 3, 64)
    n = int(L.lib().nrf_mlp_small_param_count(C.byref(d)))
    blob = np.concatenate([sc["mlp_blob"], synth.synth_sym(91, (n - sc["mlp_blob"].size,), np.float32(0.1))]).astype(np.float32)
    return sc, M.NeRFSmall(3, 64, 15, 4, 64, True, 3, 64, 32, 16, "model", params=blob), blob


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["a", "b"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from nerfpp_amd import _lib as L, mesh, modules as M, renderer as R, scene as S, synth
    from nerfpp_amd.train import Trainer
    torch.cuda.set_device(0)
    K = S.lego_K(800, 800)
    o, d, _ = R.GetRays(800, 800, K, S.pose_spherical(30.0, -30.0, 4.0))
    idx = (torch.arange(0, a.rays, device="cuda") * (640000 // a.rays + 1)) % 640000
    o, d = o.reshape(-1, 3)[idx].contiguous(), d.reshape(-1, 3)[idx].contiguous()
    tgt = torch.rand((a.rays, 3), generator=torch.Generator().manual_seed(3)).cuda()
    rp = R.NeRFRenderParams(NSamples=64, NImportance=0, Chunk=a.rays, Perturb=0.0, WhiteBkgr=False, Ndc=False, UseViewdirs=True, ThinRay=True, BoundingBox=S.LEGO_BBOX,
                            Precision=L.NRF_PREC_F32)
    out = dict(rays=a.rays, samples=64, steps=a.steps, warmup=a.warmup)
    for tag, wpn, wor in (("a", 0.0, 0.0), ("b", 1.0, 1.0)):
        if a.only and a.only != tag:
            continue
        sc, m, blob = head_scene(L, M, S, synth)
        with Trainer(sc["embedder"], sc["embeddirs"], m, sc["table"], blob, learning_rate=1e-3, pred_normal_loss_weight=wpn, orientation_loss_weight=wor) as tr:
            out[f"step_{tag}_ms"], out[f"step_{tag}_all_ms"] = timed(lambda: tr.step(o, d, tgt, rp), a.warmup, a.steps)
            if tag == "b":
                out["normal_losses"] = [float(v) for v in tr.normal_losses.cpu()]
                pts = tr.last["pts"]
                out["density_grad_ms"], _ = timed(lambda: mesh.DensityGradient(tr.renderer, pts), 2, a.steps)
                out["points"] = int(pts.shape[0])
    if "step_a_ms" in out and "step_b_ms" in out:
        out["b_minus_a_ms"] = out["step_b_ms"] - out["step_a_ms"]
        out["new_kernels_and_head_backward_ms"] = out["b_minus_a_ms"] - out["density_grad_ms"]
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
