"""Measure the SSIM training loss (nrf_ssim_loss, Trainer(ssim_loss_weight, patch_size)) on one MI355X.

  step     the training step of the bench configuration (CuHash scene, 16 384 rays, 64 + 128 samples, NRF_PREC_F16_SPLIT render, mlp_backward="f16",
           hash_backward="binned", render features reused) on patch-shaped batches of an 800 x 800 camera (nrf_rand_patches): weight 0 and weight 0.2, as 64 patches of
           16 x 16 and as 16 of 32 x 32.  Warm-up first, then hipEvent timing of each step and the median of the repeats.  For the kernel's own time run
           `--mode step --only b16` under `rocprofv3 --kernel-trace --stats` (no counters in that run) and read k_ssim_loss beside k_raw2outputs_bwd: same batch.
  torch    the yardstick: the same loss and gradient composed from torch float64 ops with autograd on the same GPU (two valid grouped conv2d per plane with the
           library's window), timed against the kernel on the same pairs, with the largest difference of the two gradients.
  heldout  whether the term helps: a student trained for --train-steps steps on patches of the teacher scene's training views, with and without the term, scored on
           held-out views with metrics.EvaluateViews (PSNR, SSIM).
One JSON line on stdout; --out also writes it to a file.
    python tools/ssim_loss_bench.py [--mode step|torch|heldout] [--rays 16384] [--steps 20] [--warmup 5] [--weight 0.2] [--only a16|b16|a32|b32] [--out FILE]
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


def patch_batch(view, rays, patch, seed=3, it=0):
    from nerfpp_amd.dataset import NeRFDataset
    ds = NeRFDataset([view], batch_size=rays, seed=seed, patch_size=patch)
    ds.SetCurrentIter(it)
    return ds.get_batch()


def mode_step(a, out):
    from nerfpp_amd import _lib as L, renderer as R, scene as S
    from nerfpp_amd.dataset import View
    from nerfpp_amd.train import Trainer
    view = View(H=800, W=800, K=S.lego_K(800, 800), Pose=S.pose_spherical(30.0, -30.0, 4.0), Near=2.0, Far=6.0)
    tgt = torch.rand((a.rays, 3), generator=torch.Generator().manual_seed(3)).cuda()
    rp = R.NeRFRenderParams(NSamples=64, NImportance=128, Chunk=a.rays, Perturb=0.0, WhiteBkgr=False, Ndc=False, UseViewdirs=True, ThinRay=True, BoundingBox=S.LEGO_BBOX,
                            Precision=L.NRF_PREC_F16_SPLIT)
    for patch in (16, 32):
        b = patch_batch(view, a.rays, patch)
        o, d = b["rays_o"].contiguous(), b["rays_d"].contiguous()
        for tag, w in ((f"a{patch}", 0.0), (f"b{patch}", a.weight)):
            if a.only and a.only != tag:
                continue
            sc = S.make_hash_scene(mode="cu", table_amp=1e-2, sigma_scale=4.0)
            with Trainer(sc["embedder"], sc["embeddirs"], sc["mlp"], sc["table"], sc["mlp_blob"], learning_rate=5e-4, mlp_backward="f16", hash_backward="binned",
                         ssim_loss_weight=w, patch_size=patch) as tr:
                out[f"step_{tag}_ms"], out[f"step_{tag}_all_ms"] = timed(lambda: tr.step(o, d, tgt, rp), a.warmup, a.steps)
                out[f"reused_render_features_{tag}"] = bool(tr.reused_render_features)
                out[f"skipped_steps_{tag}"] = int(tr.skipped_steps)
                if w > 0:
                    out[f"ssim_loss_{tag}"] = [float(v) for v in tr.ssim_loss.cpu()]
            del sc
        if f"step_a{patch}_ms" in out and f"step_b{patch}_ms" in out:
            out[f"b{patch}_minus_a{patch}_ms"] = out[f"step_b{patch}_ms"] - out[f"step_a{patch}_ms"]


def torch_ssim_loss(x, y, g):
    """x, y [b, h, w, c] fp32 on the device -> (1 - mean SSIM, d / dx) in float64 torch ops with autograd."""
    xt = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    yt = y.double().permute(0, 3, 1, 2).contiguous()
    c = xt.shape[1]
    kr, kc = g.reshape(1, 1, 1, -1).repeat(c, 1, 1, 1), g.reshape(1, 1, -1, 1).repeat(c, 1, 1, 1)          # row pass then column pass, as tools/metrics_bench.py
    f = lambda t: torch.nn.functional.conv2d(torch.nn.functional.conv2d(t, kr, groups=c), kc, groups=c)
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    mx, my = f(xt), f(yt)
    vx, vy, cxy = f(xt * xt) - mx * mx, f(yt * yt) - my * my, f(xt * yt) - mx * my
    loss = 1.0 - (((2 * mx * my + c1) * (2 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))).mean()
    loss.backward()
    return loss.detach(), xt.grad.permute(0, 2, 3, 1)


def mode_torch(a, out):
    from nerfpp_amd import metrics as M
    g = M.SsimWindow().cuda()
    gen = torch.Generator().manual_seed(5)
    for b, p in ((a.rays // 256, 16), (a.rays // 1024, 32), (1, 800)):
        x = torch.rand((b, p, p, 3), generator=gen).cuda()
        y = (x + 0.1 * (torch.rand((b, p, p, 3), generator=gen).cuda() - 0.5)).clamp(0.0, 1.0)
        grad = torch.zeros_like(x)
        tag = f"{b}x{p}x{p}"
        out[f"kernel_{tag}_ms"], _ = timed(lambda: M.SSIMLoss(x, y, weight=1.0, grad=grad), a.warmup, a.steps)
        out[f"torch_f64_{tag}_ms"], _ = timed(lambda: torch_ssim_loss(x, y, g), a.warmup, a.steps)
        loss, _, g64 = M.SSIMLoss(x, y, return_grad64=True)
        tl, tg = torch_ssim_loss(x, y, g)
        out[f"grad_dev_rel_{tag}"] = float((g64 - tg).abs().max() / tg.abs().max())
        out[f"loss_dev_{tag}"] = float((loss[0] - tl).abs())


def mode_heldout(a, out):
    from nerfpp_amd import _lib as L, metrics as M, renderer as R, scene as S
    from nerfpp_amd.dataset import View
    from nerfpp_amd.train import Trainer
    H = W = a.view_size
    K = S.lego_K(H, W)
    rp = R.NeRFRenderParams(NSamples=64, NImportance=128, Chunk=a.train_rays, Perturb=0.0, WhiteBkgr=False, Ndc=False, UseViewdirs=True, ThinRay=True, BoundingBox=S.LEGO_BBOX,
                            Precision=L.NRF_PREC_F16_SPLIT)
    teacher = S.make_hash_scene(mode="cu", log2_t=16, table_amp=1e-2, sigma_scale=4.0, seed=5000)
    shot = lambda th, ph: View(H=H, W=W, K=K, Pose=S.pose_spherical(th, ph, 4.0), Near=2.0, Far=6.0,
                               Image=R.RenderView(teacher["renderer"], S.pose_spherical(th, ph, 4.0), W, H, K, rp).Outputs.RGBMap.clone())
    train_views = [shot(th, -30.0) for th in range(-180, 180, 30)]
    held = [shot(th, -25.0) for th in (-165.0, -45.0, 75.0, 135.0)]
    out.update(view_size=H, train_views=len(train_views), heldout_views=len(held), train_steps=a.train_steps, train_rays=a.train_rays, patch=a.patch)
    for tag, w in (("plain", 0.0), ("ssim", a.weight)):
        sc = S.make_hash_scene(mode="cu", log2_t=16, table_amp=1e-2, sigma_scale=4.0, seed=6000)
        with Trainer(sc["embedder"], sc["embeddirs"], sc["mlp"], sc["table"], sc["mlp_blob"], learning_rate=5e-3, mlp_backward="f16", hash_backward="binned",
                     ssim_loss_weight=w, patch_size=a.patch) as tr:
            for it in range(a.train_steps):
                b = patch_batch(train_views[it % len(train_views)], a.train_rays, a.patch, seed=9, it=it)
                tr.step(b["rays_o"], b["rays_d"], b["target_s"], rp)
            out[f"skipped_steps_{tag}"] = int(tr.skipped_steps)
        res = M.EvaluateViews(sc["renderer"], held, rp)
        out[f"heldout_psnr_{tag}"], out[f"heldout_ssim_{tag}"] = float(res["mean_psnr"]), float(res["mean_ssim"])
        del sc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["step", "torch", "heldout"], default="step")
    ap.add_argument("--rays", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--weight", type=float, default=0.2)
    ap.add_argument("--only", choices=["a16", "b16", "a32", "b32"], default=None)
    ap.add_argument("--train-steps", type=int, default=400)
    ap.add_argument("--train-rays", type=int, default=4096)
    ap.add_argument("--patch", type=int, default=16)
    ap.add_argument("--view-size", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    out = dict(mode=a.mode, rays=a.rays, samples=192, steps=a.steps, warmup=a.warmup, ssim_loss_weight=a.weight)
    dict(step=mode_step, torch=mode_torch, heldout=mode_heldout)[a.mode](a, out)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
