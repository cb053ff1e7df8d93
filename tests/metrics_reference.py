"""numpy fp64 restatement of nerf_hip_image_metrics (include/nerf_hip.h): per view the MSE over H * W * 3 values
and SSIM as mip-NeRF's compute_ssim reports it -- 11-tap Gaussian window (sigma 1.5, sum 1), separable, horizontal pass first, VALID
filtering, C1 = 0.01^2, C2 = 0.03^2, variances clamped at 0 and the covariance to sign(t) min(sqrt(s_xx s_yy), |t|)."""
import numpy as np

C1 = 0.01 ** 2
C2 = 0.03 ** 2


def window(size=11, sigma=1.5):
    f = ((np.arange(size, dtype=np.float64) - size // 2) / sigma) ** 2
    g = np.exp(-0.5 * f)
    return g / g.sum()


def filt(z, g=None):
    """Valid separable filter over the last two axes but one of z [..., H, W, C]: [..., H - 10, W - 10, C]."""
    g = window() if g is None else g
    k = g.shape[0]
    H, W = z.shape[-3], z.shape[-2]
    h = sum(g[b] * z[..., :, b:b + W - k + 1, :] for b in range(k))
    return sum(g[a] * h[..., a:a + H - k + 1, :, :] for a in range(k))


def ssim_map(x, y):
    """x, y [..., H, W, 3] -> the SSIM map [..., H - 10, W - 10, 3] (fp64)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    mx, my = filt(x), filt(y)
    mxx, myy, mxy = mx * mx, my * my, mx * my
    with np.errstate(invalid="ignore"):
        sxx = np.maximum(0.0, filt(x * x) - mxx)
        syy = np.maximum(0.0, filt(y * y) - myy)
        t = filt(x * y) - mxy
        sxy = np.sign(t) * np.minimum(np.sqrt(sxx * syy), np.abs(t))
        return (2 * mxy + C1) * (2 * sxy + C2) / ((mxx + myy + C1) * (sxx + syy + C2))


def metrics(pred, gt):
    """pred, gt [n, H, W, 3] -> (mse [n], ssim [n]) fp64."""
    x, y = np.asarray(pred, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    mse = ((x - y) ** 2).reshape(x.shape[0], -1).mean(axis=1)
    ssim = ssim_map(x, y).reshape(x.shape[0], -1).mean(axis=1)
    return mse, ssim
