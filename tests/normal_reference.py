"""Rule NM of include/nerf_hip.h (the per-ray normal composite) restated in numpy: the field normal of every sample in fp32 with each
operation rounded, then the weighted sum in fp64.  The summation order is not part of the rule; `bound` is what a reordering and the one
fp32 rounding of the result may move."""
import numpy as np

F32 = np.float32


def field_normals(g):
    """g [..., 3] fp32 sigma gradients -> n [..., 3] fp32 = -g / sqrt((g0 g0 + g1 g1) + g2 g2), (0, 0, 0) where the length is 0 or not
    finite (nerf.field_normals, the marching-cubes kernel's rule)"""
    g = np.asarray(g, F32)
    with np.errstate(all="ignore"):
        g0, g1, g2 = g[..., 0], g[..., 1], g[..., 2]
        length = np.sqrt(((g0 * g0).astype(F32) + (g1 * g1).astype(F32)).astype(F32) + (g2 * g2).astype(F32)).astype(F32)
        ok = np.isfinite(length) & (length > 0)
        n = (-g / np.where(ok, length, F32(1.0))[..., None]).astype(F32)
    return np.where(ok[..., None], n, F32(0.0)).astype(F32)


def composite64(w, g):
    """w [B, N], g [B, N, 3] fp32 -> S64 [B, 3] fp64 = sum_i double(w_i) * double(n_i); a weight that is 0 or NaN adds nothing"""
    w = np.asarray(w, F32)
    n = field_normals(g).astype(np.float64)
    with np.errstate(invalid="ignore"):
        live = (w > 0) | (w < 0)
    wd = np.where(live, w, F32(0.0)).astype(np.float64)
    with np.errstate(invalid="ignore"):
        terms = np.where(live[..., None], wd[..., None] * n, 0.0)
    S = np.zeros((w.shape[0], 3), np.float64)
    for i in range(w.shape[1]):  # index order, sample by sample
        S += terms[:, i]
    return S


def composite(w, g):
    """rule NM's N [B, 3] fp32"""
    return composite64(w, g).astype(F32)


def ulp32(x):
    """the spacing of fp32 at |x| (fp64 in, fp64 out); the smallest subnormal at 0"""
    a = np.abs(np.asarray(x, np.float64)).astype(F32)
    return (np.nextafter(a, F32(np.inf)) - a).astype(np.float64)


def bound(w, S64):
    """per component: one fp32 rounding plus a possible tie, and the reordering of at most 2,048 fp64 terms of magnitude <= |w_i|
    (below 2048 * 2^-53 * sum |w_i| = 2.3e-13 sum |w_i|, taken with a 4x margin)"""
    w = np.asarray(w, F32)
    with np.errstate(invalid="ignore"):
        live = (w > 0) | (w < 0)
    sw = np.where(live, np.abs(w), F32(0.0)).astype(np.float64).sum(axis=1)
    return ulp32(S64) + 1e-12 * sw[:, None]


def sequential(w_row, g_row):
    """rule NM for one ray with Python floats, sample by sample in index order (the definition the restatement is held to)"""
    acc = [0.0, 0.0, 0.0]
    for wi, gi in zip(w_row, g_row):
        n = field_normals(np.asarray(gi, F32))
        wi = float(wi)
        if wi > 0 or wi < 0:
            for c in range(3):
                acc[c] += wi * float(n[c])
    return np.array(acc, np.float64)
