"""Time the training step of the bench configuration (CuHash scene, 16 384 rays, 64 + 128 samples, NRF_PREC_F16_SPLIT render, mlp_backward="f16", hash_backward="binned",
render features reused) on one MI355X, once with both ray-regulariser weights 0 and once with both on (nrf_ray_regularizers between the RawToOutputs backward and the
keep mask).

Warm-up first, then hipEvent timing of each step and the median of the repeats (one JSON line on stdout; --out also writes it to a file).  For the kernel's own time run
this script under `rocprofv3 --kernel-trace --stats` (no counters in that run) with --only b and read k_ray_reg beside k_raw2outputs_bwd: same batch, same bytes.
    python tools/ray_reg_bench.py [--rays 16384] [--steps 20] [--warmup 5] [--only a|b] [--out FILE]
"""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["a", "b"], default=None)
    ap.add_argument("--distortion", type=float, default=1e-2)
    ap.add_argument("--sparsity", type=float, default=1e-4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from nerfpp_amd import _lib as L, renderer as R, scene as S
    from nerfpp_amd.train import Trainer
    torch.cuda.set_device(0)
    K = S.lego_K(800, 800)
    o, d, _ = R.GetRays(800, 800, K, S.pose_spherical(30.0, -30.0, 4.0))
    idx = torch.arange(0, a.rays, device="cuda") * (640000 // a.rays)
    o, d = o.reshape(-1, 3)[idx].contiguous(), d.reshape(-1, 3)[idx].contiguous()
    tgt = torch.rand((a.rays, 3), generator=torch.Generator().manual_seed(3)).cuda()
    rp = R.NeRFRenderParams(NSamples=64, NImportance=128, Chunk=a.rays, Perturb=0.0, WhiteBkgr=False, Ndc=False, UseViewdirs=True, ThinRay=True, BoundingBox=S.LEGO_BBOX,
                            Precision=L.NRF_PREC_F16_SPLIT)
    out = dict(rays=a.rays, samples=192, steps=a.steps, warmup=a.warmup, distortion_loss_weight=a.distortion, sparsity_loss_weight=a.sparsity)
    for tag, wd, ws in (("a", 0.0, 0.0), ("b", a.distortion, a.sparsity)):
        if a.only and a.only != tag:
            continue
        sc = S.make_hash_scene(mode="cu", table_amp=1e-2, sigma_scale=4.0)
        with Trainer(sc["embedder"], sc["embeddirs"], sc["mlp"], sc["table"], sc["mlp_blob"], learning_rate=5e-4, mlp_backward="f16", hash_backward="binned",
                     distortion_loss_weight=wd, sparsity_loss_weight=ws) as tr:
            out[f"step_{tag}_ms"], out[f"step_{tag}_all_ms"] = timed(lambda: tr.step(o, d, tgt, rp), a.warmup, a.steps)
            out[f"reused_render_features_{tag}"] = bool(tr.reused_render_features)
            out[f"skipped_steps_{tag}"] = int(tr.skipped_steps)
            if tag == "b":
                out["ray_losses"] = [float(v) for v in tr.ray_losses.cpu()]
        del sc
    if "step_a_ms" in out and "step_b_ms" in out:
        out["b_minus_a_ms"] = out["step_b_ms"] - out["step_a_ms"]
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
