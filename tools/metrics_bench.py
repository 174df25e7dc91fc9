"""Time the image metrics on one MI355X: metrics.SSIM, metrics.MSSSIM and metrics.PSNR on one 800x800x3 pair and on a batch of 8, against the same definition
composed from torch ops on the same GPU -- valid grouped conv2d with the library's window, row pass then column pass, 2x2 avg_pool2d between scales -- in float64 and
in float32.  Beside each library time the bytes the two input images occupy (2 * b * h * w * c * 4) divided by it.

Warm-up first, then hipEvent timing of each call and the median of the repeats; the three paths of a metric are timed alternately inside one repeat loop.  The composed
float64 result is also compared with the library's (max |difference|), and the float32 one shows what fp32 costs in accuracy.  One JSON line on stdout; --out also writes it.
    python tools/metrics_bench.py [--size 800] [--batches 1 8] [--repeats 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def composed_ssim(x, y, g, data_range=1.0):
    """x, y [b, c, h, w] in the dtype to compute in -> (mean ssim, mean cs), each [b, c]."""
    c = x.shape[1]
    kr = g.to(x.dtype).reshape(1, 1, 1, 11).repeat(c, 1, 1, 1)
    kc = g.to(x.dtype).reshape(1, 1, 11, 1).repeat(c, 1, 1, 1)
    f = lambda a: torch.nn.functional.conv2d(torch.nn.functional.conv2d(a, kr, groups=c), kc, groups=c)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mx, my = f(x), f(y)
    mxx, myy, mxy = mx * mx, my * my, mx * my
    sxx, syy, sxy = f(x * x) - mxx, f(y * y) - myy, f(x * y) - mxy
    cs = (2 * sxy + c2) / (sxx + syy + c2)
    ssim = (2 * mxy + c1) / (mxx + myy + c1) * cs
    return ssim.mean(dim=(2, 3)), cs.mean(dim=(2, 3))


def composed_ms_ssim(x, y, g, weights=WEIGHTS):
    terms = []
    for i in range(len(weights)):
        if i:
            x, y = torch.nn.functional.avg_pool2d(x, 2), torch.nn.functional.avg_pool2d(y, 2)
        ssim, cs = composed_ssim(x, y, g)
        terms.append(ssim if i == len(weights) - 1 else cs)
    w = torch.tensor(weights, dtype=x.dtype, device=x.device)
    return torch.prod(torch.stack(terms).clamp_min(0) ** w[:, None, None], dim=0).mean(dim=1)


def composed_psnr(x, y):
    d = x - y
    return 10.0 * torch.log10(1.0 / (d * d).mean(dim=(1, 2, 3)))


def timed_together(fns, warmup, repeats):
    """{name: median ms}: every repeat runs each fn once, in turn, each between its own pair of events."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: float(np.median(v)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    from nerfpp_amd import metrics as M
    from nerfpp_amd.synth import synth_u01
    torch.cuda.set_device(0)
    g = M.SsimWindow().cuda()
    s = a.size
    out = dict(size=s, channels=3, repeats=a.repeats, warmup=a.warmup, device=torch.cuda.get_device_name(0))
    for b in a.batches:
        n = b * s * s * 3
        yy, xx = np.meshgrid(np.arange(s, dtype=np.float32), np.arange(s, dtype=np.float32), indexing="ij")
        smooth = (0.5 + 0.2 * np.sin(0.021 * xx + 0.013 * yy)).astype(np.float32)[None, :, :, None]
        x = torch.from_numpy((smooth + 0.2 * (synth_u01(11, n).reshape(b, s, s, 3) - 0.5)).astype(np.float32)).cuda()
        y = (x + 0.1 * (torch.from_numpy(synth_u01(12, n).reshape(b, s, s, 3)).cuda() - 0.5)).contiguous()
        # the composed paths get their layout and dtype for free: [b, c, h, w], converted outside the timed window
        x64, y64 = x.permute(0, 3, 1, 2).double().contiguous(), y.permute(0, 3, 1, 2).double().contiguous()
        x32, y32 = x64.float(), y64.float()
        row = dict(input_bytes=2 * n * 4)
        groups = dict(
            ssim=dict(lib=lambda: M.SSIM(x, y), torch_f64=lambda: composed_ssim(x64, y64, g)[0].mean(dim=1), torch_f32=lambda: composed_ssim(x32, y32, g)[0].mean(dim=1)),
            ms_ssim=dict(lib=lambda: M.MSSSIM(x, y), torch_f64=lambda: composed_ms_ssim(x64, y64, g), torch_f32=lambda: composed_ms_ssim(x32, y32, g)),
            psnr=dict(lib=lambda: M.PSNR(x, y), torch_f64=lambda: composed_psnr(x64, y64), torch_f32=lambda: composed_psnr(x32, y32)))
        for name, fns in groups.items():
            ms = timed_together(fns, a.warmup, a.repeats)
            lib, f64, f32 = (fns[k]().double() for k in ("lib", "torch_f64", "torch_f32"))
            row[name] = dict(lib_ms=ms["lib"], torch_f64_ms=ms["torch_f64"], torch_f32_ms=ms["torch_f32"], lib_input_gb_per_s=row["input_bytes"] / ms["lib"] * 1e-6,
                             value=float(lib[0]), max_abs_lib_minus_torch_f64=float((lib - f64).abs().max()), max_abs_lib_minus_torch_f32=float((lib - f32).abs().max()))
        out[f"batch_{b}"] = row
        del x, y, x64, y64, x32, y32
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
