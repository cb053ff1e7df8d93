"""Image metrics of rendered frames: MSE, PSNR and SSIM per view.

The arithmetic is ``nerf_hip_image_metrics`` (csrc/metrics.hip, fp64 on the device; the definition is written out in
include/nerf_hip.h): SSIM as mip-NeRF's ``compute_ssim`` reports it -- 11-tap Gaussian window, sigma 1.5, valid filtering,
C1 = 0.01^2, C2 = 0.03^2 -- and PSNR = -10 log10(MSE), data range 1, no clipping.  There is no host fallback.
"""
from __future__ import annotations

import numpy as np
import torch

WINDOW = 11  # SSIM's window: H and W must be at least this


def psnr_from_mse(mse):
    """-10 log10(mse) for a float or an array of them: +inf where mse is 0, NaN where it is NaN."""
    with np.errstate(divide="ignore", invalid="ignore"):
        out = -10.0 * np.log10(np.asarray(mse, dtype=np.float64))
    return float(out) if out.ndim == 0 else out


def _as_views(x, name: str):
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    if not torch.is_tensor(t):
        raise TypeError(f"{name}: a torch tensor or a numpy array, not {type(x).__name__}")
    if t.dim() == 3:
        t = t.unsqueeze(0)
    if t.dim() != 4 or t.shape[-1] != 3:
        raise ValueError(f"{name} {tuple(t.shape)}: [H, W, 3] or [n, H, W, 3]")
    return t


def image_metrics(pred, gt):
    """Per-view {"mse", "psnr", "ssim"} of pred against gt: [H, W, 3] or [n, H, W, 3] torch tensors or numpy arrays of the same shape,
    values in [0, 1] (data range 1, nothing is clipped).  H, W >= 11.  Inputs off the device are copied to the device the other one is
    on, or to the current ROCm device.  Returns numpy float64 arrays of length n, or floats for an [H, W, 3] input.
    NaN or inf in a view's inputs shows in that view's results."""
    single = getattr(pred, "ndim", None) == 3
    p, g = _as_views(pred, "pred"), _as_views(gt, "gt")
    if tuple(p.shape) != tuple(g.shape):
        raise ValueError(f"pred {tuple(p.shape)} and gt {tuple(g.shape)} differ")
    if p.shape[1] < WINDOW or p.shape[2] < WINDOW:
        raise ValueError(f"{p.shape[1]} x {p.shape[2]} images: SSIM's {WINDOW} x {WINDOW} window needs H, W >= {WINDOW}")
    from . import ops

    device = g.device if g.device.type == "cuda" else (p.device if p.device.type == "cuda" else None)
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("image_metrics runs on a ROCm device (MI355X): there is no CPU path")
        device = torch.device("cuda", torch.cuda.current_device())
    mse, ssim = ops.image_metrics(p.to(device, torch.float32), g.to(device, torch.float32))
    mse, ssim = mse.cpu().numpy(), ssim.cpu().numpy()
    out = {"mse": mse, "psnr": psnr_from_mse(mse), "ssim": ssim}
    if single:
        out = {k: float(v[0]) for k, v in out.items()}
    return out
