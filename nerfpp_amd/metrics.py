"""Image metrics on the device: MSE, PSNR, SSIM, MSSSIM, SSIMLoss and EvaluateViews over the C ABI (include/nerfpp_hip.h, image_metrics.hip).

The reference measures a frame only inside its training loop (-10 log10(mse), NeRFExecutor.h:893; scene.psnr restates it on the host).  Here a render is scored
where it lies: the kernels compute in fp64 in a stated operation order (the header gives it), so a numpy float64 restatement equals the SSIM map bit for bit, the
sums are ordered (two runs, and any batching, give the same bits), and nothing here synchronises: every result is a float64 tensor on the device.

Images are [H, W], [H, W, C] or [B, H, W, C] with C in 1..4; a result has one entry per image ([B]; a scalar tensor for an unbatched image).
"""
import ctypes as C

import torch

from . import _lib as L
from .modules import _ptr, _stream, _dev_f32

MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)          # Wang et al. 2003


def _pair(x, y, who):
    """-> (x, y) as [b, h, w, c] fp32 contiguous, batched (whether the caller's images had a batch axis)."""
    x, y = _dev_f32(x), _dev_f32(y)
    if x.shape != y.shape:
        raise L.NrfError(f"{who}: the images differ in shape: {tuple(x.shape)} and {tuple(y.shape)}")
    if x.dim() not in (2, 3, 4):
        raise L.NrfError(f"{who}: images are [H, W], [H, W, C] or [B, H, W, C], got {tuple(x.shape)}")
    batched = x.dim() == 4
    if x.dim() == 2:
        x, y = x[..., None], y[..., None]
    if x.dim() == 3:
        x, y = x[None], y[None]
    return x.contiguous(), y.contiguous(), batched


def _workspace(nbytes, dev):
    return torch.empty((max(1, int(nbytes)),), device=dev, dtype=torch.uint8)


def SsimWindow():
    """nrf_ssim_window: the library's 11 Gaussian weights (sigma 1.5) as a float64 CPU tensor."""
    out = (C.c_double * 11)()
    L.check(L.lib().nrf_ssim_window(out))
    return torch.tensor(list(out), dtype=torch.float64)


def MSE(x, y):
    """nrf_image_mse: the mean of ((double)x - (double)y)^2 per image."""
    x, y, batched = _pair(x, y, "MSE")
    b = x.shape[0]
    n = x.numel() // b
    lib = L.lib()
    out = torch.empty((b,), device=x.device, dtype=torch.float64)
    ws = _workspace(lib.nrf_image_mse_workspace_bytes(b, n), x.device)
    L.check(lib.nrf_image_mse(_ptr(x), _ptr(y), b, n, _ptr(out), _ptr(ws), ws.numel(), _stream()))
    return out if batched else out[0]


def PSNR(x, y, data_range=1.0):
    """10 log10(L^2 / mse); inf where the images are equal."""
    mse = MSE(x, y)
    return 10.0 * torch.log10(float(data_range) ** 2 / mse)


def SSIM(x, y, data_range=1.0, per_channel=False, return_map=False):
    """nrf_ssim: the mean SSIM over the valid region (H-10) x (W-10), averaged over the channels ([B]) or, with per_channel, for each ([B, C]).  With return_map,
    (means, map [B, H-10, W-10, C]): the per-pixel SSIM."""
    x, y, batched = _pair(x, y, "SSIM")
    b, h, w, c = (int(v) for v in x.shape)
    lib = L.lib()
    means = torch.empty((b, c, 2), device=x.device, dtype=torch.float64)
    smap = torch.empty((b, max(h - 10, 0), max(w - 10, 0), c), device=x.device, dtype=torch.float64) if return_map else None
    ws = _workspace(lib.nrf_ssim_workspace_bytes(b, h, w, c), x.device)
    L.check(lib.nrf_ssim(_ptr(x), _ptr(y), b, h, w, c, float(data_range), _ptr(means), _ptr(smap), _ptr(ws), ws.numel(), _stream()))
    out = means[..., 0] if per_channel else means[..., 0].mean(dim=1)
    if not batched:
        out = out[0]
        smap = smap[0] if return_map else None
    return (out, smap) if return_map else out


def SSIMLoss(x, y, data_range=1.0, weight=1.0, grad=None, return_grad64=False):
    """nrf_ssim_loss: 1 - the mean SSIM over every valid value of the batch, as a training loss of x against y -> (loss [2] float64 on the device: {1 - mean, mean},
    grad).  `grad` (fp32, x's shape) is accumulated into, grad += float32(weight * d(1 - mean)/dx); None starts from zeros.  With return_grad64 the result is
    (loss, grad, grad64): the unweighted float64 gradient."""
    x, y, _ = _pair(x, y, "SSIMLoss")
    b, h, w, c = (int(v) for v in x.shape)
    if grad is None:
        grad = torch.zeros_like(x)
    elif grad.dtype != torch.float32 or not grad.is_cuda or not grad.is_contiguous() or grad.numel() != x.numel():
        raise L.NrfError(f"SSIMLoss: grad must be a contiguous fp32 device tensor of {x.numel()} elements")
    lib = L.lib()
    loss = torch.empty((2,), device=x.device, dtype=torch.float64)
    g64 = torch.empty(x.shape, device=x.device, dtype=torch.float64) if return_grad64 else None
    ws = _workspace(lib.nrf_ssim_loss_workspace_bytes(b, h, w, c), x.device)
    L.check(lib.nrf_ssim_loss(_ptr(x), _ptr(y), b, h, w, c, float(data_range), float(weight), _ptr(loss), _ptr(grad), _ptr(g64), _ptr(ws), ws.numel(), _stream()))
    return (loss, grad, g64) if return_grad64 else (loss, grad)


def MsSsimScaleMeans(x, y, data_range=1.0, scales=5):
    """nrf_ms_ssim: [scales, B, C, 2] -- the mean ssim and the mean cs of every scale (scale i: the images pooled 2 x 2 i times, in double)."""
    x, y, _ = _pair(x, y, "MSSSIM")
    b, h, w, c = (int(v) for v in x.shape)
    lib = L.lib()
    means = torch.empty((int(scales), b, c, 2), device=x.device, dtype=torch.float64)
    ws = _workspace(lib.nrf_ms_ssim_workspace_bytes(b, h, w, c, int(scales)), x.device)
    L.check(lib.nrf_ms_ssim(_ptr(x), _ptr(y), b, h, w, c, float(data_range), int(scales), _ptr(means), _ptr(ws), ws.numel(), _stream()))
    return means


def CombineMsSsim(scale_means, weights=MS_SSIM_WEIGHTS):
    """Per channel prod_i max(cs_i, 0)^w_i over every scale but the last, times max(ssim_last, 0)^w_last; then the mean over channels.  scale_means [scales, B, C, 2]
    (ssim, cs) on any device -> [B] float64."""
    m = torch.as_tensor(scale_means, dtype=torch.float64)
    wt = torch.tensor([float(v) for v in weights], dtype=torch.float64, device=m.device)
    if m.dim() != 4 or m.shape[0] != wt.numel() or m.shape[-1] != 2:
        raise L.NrfError(f"CombineMsSsim: scale means {tuple(m.shape)} for {wt.numel()} weights")
    terms = torch.cat([m[:-1, ..., 1], m[-1:, ..., 0]], dim=0).clamp_min(0.0)          # [scales, B, C]
    return torch.prod(terms ** wt[:, None, None], dim=0).mean(dim=1)


def MSSSIM(x, y, data_range=1.0, weights=MS_SSIM_WEIGHTS):
    """Multi-scale SSIM (Wang et al. 2003); len(weights) sets the number of scales (1..5), and min(H, W) >> (scales - 1) must be >= 11."""
    batched = _dev_f32(x).dim() == 4
    out = CombineMsSsim(MsSsimScaleMeans(x, y, data_range, len(weights)), weights)
    return out if batched else out[0]


_METRICS = {"mse": lambda a, b: MSE(a, b), "psnr": lambda a, b: PSNR(a, b), "ssim": lambda a, b: SSIM(a, b), "ms_ssim": lambda a, b: MSSSIM(a, b)}


def EvaluateViews(renderer, views, rparams, metrics=("psnr", "ssim"), quantize=False):
    """Score a renderer on held-out views: each dataset.View is rendered with RenderView at (v.W, v.H, v.K, v.Pose) and its RGBMap scored against v.Image
    (data_range 1).  Returns {name: float64 device tensor [n_views], "mean_" + name: its mean} for the names in `metrics` ("mse", "psnr", "ssim", "ms_ssim").
    quantize=True scores TorchTensorToCVMat(rgb) / 255: what the written 8-bit image would score.  Adds no host synchronisation of its own between views."""
    from .renderer import RenderView, TorchTensorToCVMat
    names = tuple(metrics)
    for n in names:
        if n not in _METRICS:
            raise L.NrfError(f"EvaluateViews: unknown metric {n!r} (one of {sorted(_METRICS)})")
    views = list(views)
    for i, v in enumerate(views):
        if v.Image is None:
            raise L.NrfError(f"EvaluateViews: view {i} has no image to score against")
    scores = {n: [] for n in names}
    for v in views:
        rgb = RenderView(renderer, v.Pose, v.W, v.H, v.K, rparams).Outputs.RGBMap
        if quantize:
            rgb = TorchTensorToCVMat(rgb).to(torch.float32) / 255.0
        img = _dev_f32(v.Image)
        if rgb.shape != img.shape:
            raise L.NrfError(f"EvaluateViews: the render is {tuple(rgb.shape)}, the view's image {tuple(img.shape)}")
        for n in names:
            scores[n].append(_METRICS[n](rgb, img))
    out = {}
    for n in names:
        dev = torch.device("cuda", torch.cuda.current_device())
        out[n] = torch.stack(scores[n]) if scores[n] else torch.empty((0,), device=dev, dtype=torch.float64)
        out["mean_" + n] = out[n].mean()
    return out
