"""Rule QD of include/nerf_hip.h in numpy: the quantile depths of one pass of a ray, including the order in which the kernels form the
fp64 prefix sums (per chunk of 64 samples the Hillis-Steele steps 1, 2, 4 .. 32 of wave_incl_scan, then + the carried total).

  prefix_sums(w)        W_i exactly as k_coarse_x / k_merge_x (quantile forms) form them  [..., N] fp32 -> [..., N] fp64
  quantile_depths(...)  Q(q_j) per ray                                                    w, t [B, N] fp32, q [nq] -> [B, nq] fp32
  definition(...)       the rule once more, one ray, plain sequential Python floats (tests: exact weights make the scan order irrelevant)
  depth_image(...)      fuse_depth's depth-image rule over arrays (median, spread rejection -> NaN, background -> inf)
"""
import numpy as np

CHUNK = 64


def prefix_sums(w):
    """fp64 inclusive prefix sums of the fp32 weights w [..., N] in the kernels' order."""
    w = np.asarray(w, dtype=np.float32)
    N = w.shape[-1]
    out = np.empty(w.shape, dtype=np.float64)
    carry = np.zeros(w.shape[:-1], dtype=np.float64)
    for base in range(0, N, CHUNK):
        n = min(CHUNK, N - base)
        v = np.zeros(w.shape[:-1] + (CHUNK,), dtype=np.float64)
        v[..., :n] = w[..., base:base + n].astype(np.float64)  # lanes behind the ray hold 0
        d = 1
        while d < CHUNK:
            nxt = v.copy()
            nxt[..., d:] = v[..., d:] + v[..., :-d]  # every lane l >= d at once: v_l += v_{l-d}
            v = nxt
            d *= 2
        v = v + carry[..., None]
        carry = v[..., CHUNK - 1]
        out[..., base:base + n] = v[..., :n]
    return out


def quantile_depths(w, t, q):
    """w, t [B, N] fp32, q: nq floats (taken as fp32) -> Q [B, nq] fp32 by rule QD."""
    w = np.asarray(w, dtype=np.float32)
    t = np.asarray(t, dtype=np.float32)
    q = np.asarray(q, dtype=np.float32).reshape(-1)
    B, N = w.shape
    Wi = prefix_sums(w)
    out = np.empty((B, q.shape[0]), dtype=np.float32)
    with np.errstate(all="ignore"):
        for b in range(B):
            W = Wi[b, N - 1]
            for j in range(q.shape[0]):
                theta = np.float64(q[j]) * W
                hit = np.nonzero(Wi[b] >= theta)[0]  # (a comparison with NaN is false)
                res = t[b, N - 1]
                if hit.size:
                    k = int(hit[0])
                    if w[b, k] > 0:
                        E = Wi[b, k - 1] if k > 0 else np.float64(0.0)
                        f = (theta - E) / np.float64(w[b, k])
                        f = f if f > 0.0 else np.float64(0.0)
                        f = f if f < 1.0 else np.float64(1.0)
                        tk = np.float64(t[b, k])
                        tn = np.float64(t[b, k + 1]) if k + 1 < N else tk
                        res = np.float32(tk + f * (tn - tk))
                out[b, j] = res
    return out


def definition(w, t, q):
    """One ray, one quantile, sequential Python floats (fp64): the rule with the prefix sums taken left to right."""
    w = [float(np.float32(x)) for x in w]
    t = [float(np.float32(x)) for x in t]
    N = len(w)
    acc, Wi = 0.0, []
    for x in w:
        acc = acc + x
        Wi.append(acc)
    theta = float(np.float32(q)) * Wi[-1]
    for k in range(N):
        if Wi[k] >= theta:
            if not w[k] > 0:
                break
            E = Wi[k - 1] if k else 0.0
            f = (theta - E) / w[k]
            f = f if f > 0.0 else 0.0
            f = f if f < 1.0 else 1.0
            tn = t[k + 1] if k + 1 < N else t[k]
            return np.float32(t[k] + f * (tn - t[k]))
    return np.float32(t[-1])


def depth_image(mean, a, Q3, depth_stat, min_opacity, max_spread):
    """fuse_depth's rule, written out pixel by pixel: mean = D / A, a = A, Q3 [n, 3] = (Q(0.25), Q(0.5), Q(0.75)) -> (depth, rejected)."""
    mean, a, Q3 = (np.asarray(x, dtype=np.float32) for x in (mean, a, Q3))
    d = np.empty(a.shape, dtype=np.float32)
    rej = np.zeros(a.shape, dtype=bool)
    for i in range(a.shape[0]):
        if not a[i] >= min_opacity:
            d[i] = np.inf
        elif max_spread is not None and Q3[i, 2] - Q3[i, 0] > np.float32(max_spread):
            d[i], rej[i] = np.nan, True
        else:
            d[i] = Q3[i, 1] if depth_stat == "median" else mean[i]
    return d, rej


def two_layer_s(a):
    """(s_a, s_b): the optical depths sigma * delta of a two-layer ray whose front layer takes the share a of the ray's hit distribution.
    The composite's transmittance is INCLUSIVE (T_i = exp(-sum_{j <= i} s_j), as the reference's), so one sample's weight is
    T_{i-1} x (1 - x) with x = exp(-s) -- at most a quarter of what reaches it, at s = ln 2, which is the back layer here: w_b = x_a / 4,
    w_a = x_a (1 - x_a), and w_a / (w_a + w_b) = a gives 1 - x_a = a / (4 (1 - a)) (a < 0.8)."""
    return float(-np.log(1.0 - a / (4.0 * (1.0 - a)))), float(np.log(2.0))


def weights_inclusive(s):
    """fp64: w_i = exp(-sum_{j <= i} s_j) (1 - exp(-s_i)), the composite's definition"""
    s = np.asarray(s, dtype=np.float64)
    return np.exp(-np.cumsum(s, axis=-1)) * (1.0 - np.exp(-s))
