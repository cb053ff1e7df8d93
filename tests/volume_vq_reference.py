"""numpy restatements of rules VI, VQ-A, VQ-U and VQ-D of include/nerf_hip.h (per-row importance, the k-means codebook and the decode
of vector-quantised compact volumes), of volume.vq_classes and of volume.kmeans' initial codebook, each in a vectorised and in a
scalar-loops form, and the word-by-word budget rule VI's sums have to meet against the fp64 restatement.  Shared by
tests/test_volume_vq_cpu.py and tests/test_gpu_volume_vq.py.  Built on volume_grad_reference (geometry, lookup32, pad, forward,
_corner_terms) and volume_compact_reference (slots, rows).

THE BUDGET OF RULE VI (derived, never fitted).  u = 2^-24.  The device adds llrint((tw_c (double)w_i) 2^40) with ITS fp32 w_i; the
reference adds tw_c w_i with w_i from the fp64 recurrence over the same fp32 sigma_s.  tw_c is formed in fp64 from the same fp32
fractions on both sides (the cell and the fractions are rule VL's fp32 values, restated bit for bit).  So the only inexact inputs are
the fp32 alpha_i, w_i and T_i, for which volume_reference's THE BOUND gives, i being the 1-based ordinal of the contributing sample,
      |dw_i| <= e_(i-1) alpha_i + 6 u <= 7 u (i - 1) alpha_i + 6 u.
A contribution therefore errs by at most tw_c |dw_i|, plus 2^-41 (half a unit of the fixed point) for its llrint; a row's budget is the
sum of that over what the row received, times (1 + 2^-10) for the second-order terms and the fp64 roundings of the products.  A row
that received nothing has budget 0 and must hold exactly 0.  It inherits volume_reference's ASSUMPTION that expm1f is good to 2 ulp.
"""
from fractions import Fraction

import numpy as np

import volume_compact_reference as X
import volume_grad_reference as GR
import volume_reference as R

F = np.float32
H = np.float16
U = R.U
SHIFT = 40                # rule VI's fixed point: rule VG's
QUANT = 2.0 ** -(SHIFT + 1)
VQ_SHIFT = 20             # rule VQ-U's fixed point
MAX_WORD = 1024.0
INF = F(np.inf)


def fix(x, shift):
    """llrint(clamp(x 2^shift, +-2^62)); a NaN gives 0 -- np.rint rounds half to even, as llrint does in the default mode"""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        y = np.clip(x * 2.0 ** shift, -2.0 ** 62, 2.0 ** 62)
    return np.where(np.isnan(x), 0.0, np.rint(y)).astype(np.int64)


# ---- rule VI ----

def corner_rows(G, idx, slot, n):
    """per padded sample and corner: tw [N, Mx, 8] fp64, and the corner's row [N, Mx, 8] (-1 where its slot lies outside [0, n))"""
    tw, lin = GR._corner_terms(G, idx)
    s = np.asarray(slot).reshape(-1)[lin].astype(np.int64)
    return tw, np.where((s >= 0) & (s < n), s, -1)


def importance_fixed(G, idx, valid, w, slot, n, mutate=None, T_before=None, w_after=None):
    """Rule VI's int64 sums for the given per-sample weights w [N, Mx] (fp32: the device's own values) -> imp [n] int64.
    mutate: None, or one of the wrong versions the budget has to reject -- "T" (T before the sample in place of w; T_before given),
    "no_wz" (the corner term without its z factor), "w_after" (the weight formed with T after its update; w_after given)."""
    tw, row = corner_rows(G, idx, slot, n)
    if mutate == "no_wz":
        f = G.f[np.maximum(idx, 0)].astype(np.float64)
        tw = np.stack([(f[..., 0] if (c >> 2) & 1 else 1.0 - f[..., 0]) * (f[..., 1] if (c >> 1) & 1 else 1.0 - f[..., 1]) for c in range(8)], -1)
    wt = {None: w, "no_wz": w, "T": T_before, "w_after": w_after}[mutate]
    q = fix(tw * np.asarray(wt, np.float64)[..., None], SHIFT)
    ok = valid[..., None] & (row >= 0)
    imp = np.zeros(n, np.int64)
    np.add.at(imp, row[ok], q[ok])
    return imp


def importance_reference(G, sig, slot, n, limit=None, t_stop=0.0):
    """The fp64 restatement of rule VI with its budget -> dict(imp [n] fp64 in weight units, budget [n], idx, valid, alpha, w, Tn);
    limit [N]: every ray truncated at that many contributing samples (the device's own steps[:, 0])."""
    idx = GR.pad(G, sig, limit=limit)
    alpha, w, Tn, valid = GR.forward(G, sig, idx, np.float64, t_stop)
    tw, row = corner_rows(G, idx, slot, n)
    ok = valid[..., None] & (row >= 0)
    imp, bud = np.zeros(n), np.zeros(n)
    np.add.at(imp, row[ok], (tw * w[..., None])[ok])
    i1 = np.arange(1, idx.shape[1] + 1, dtype=np.float64)[None, :]
    dw = 7 * U * (i1 - 1) * alpha + 6 * U
    np.add.at(bud, row[ok], (tw * dw[..., None] + QUANT)[ok])
    return dict(imp=imp, budget=bud * (1 + 2.0 ** -10), idx=idx, valid=valid, alpha=alpha, w=w, Tn=Tn)


def importance_ratio(got_fixed, ref):
    """max over the rows of |got - reference| / budget (got: int64 sums in units of 2^-40); a row with a zero budget must be exactly 0"""
    got = np.asarray(got_fixed, np.float64) * 2.0 ** -SHIFT
    zero = ref["budget"] == 0
    if (got[zero] != 0).any():
        return np.inf
    return float((np.abs(got - ref["imp"])[~zero] / ref["budget"][~zero]).max()) if (~zero).any() else 0.0


def forward32_all(G, sig, idx, t_stop=0.0):
    """the fp32 recurrence (numpy's expm1 for expm1f) -> (w, T before each sample, w formed AFTER the T update: T_new alpha, valid)"""
    alpha, w, Tn, valid = GR.forward(G, sig, idx, F, t_stop)
    Tb = np.concatenate([np.ones((Tn.shape[0], 1), F), Tn[:, :-1]], axis=1)
    return w, Tb, (Tn * alpha).astype(F), valid


def recurrence32(alpha, K):
    """w_0 .. w_(K-1) of the fp32 recurrence with one GIVEN alpha (the slab): w = T alpha, T = T - w, each rounded"""
    alpha = F(alpha)
    T, w = F(1), np.zeros(K, F)
    for i in range(K):
        w[i] = F(T * alpha)
        T = F(T - w[i])
    return w


def importance_loops(f, ci, w, slot, n):
    """Rule VI with scalar loops over given contributing samples: f [M, 3] fp32, ci [M, 3], w [M] fp32 -> imp [n] as Python ints"""
    nx, ny, nz = slot.shape
    imp = [0] * n
    for s in range(len(w)):
        fx, fy, fz = (float(f[s, a]) for a in range(3))
        for c in range(8):
            di, dj, dk = (c >> 2) & 1, (c >> 1) & 1, c & 1
            r = int(slot[ci[s, 0] + di, ci[s, 1] + dj, ci[s, 2] + dk])
            if r < 0 or r >= n:
                continue
            tw = ((fx if di else 1.0 - fx) * (fy if dj else 1.0 - fy)) * (fz if dk else 1.0 - fz)
            imp[r] += int(fix(tw * float(w[s]), SHIFT))
    return imp


# ---- volume.vq_classes ----

def classes(imp, prune_share=None, keep_share=0.0, rows=None):
    imp = np.asarray(imp, np.int64)
    n = imp.size
    cls = np.ones(n, np.uint8)
    if n:
        order = np.argsort(imp, kind="stable")
        srt = imp[order]
        cs = np.cumsum(srt)
        total = int(cs[-1])
        cls[order[(total - cs) + srt <= int(Fraction(keep_share) * total)]] = 2
        if prune_share is not None:
            cls[order[cs <= int(Fraction(prune_share) * total)]] = 0
    if rows is not None:
        r = np.asarray(rows, F)
        with np.errstate(all="ignore"):
            cls[~(np.isfinite(r) & (np.abs(r) <= MAX_WORD)).all(1)] = 2
    return cls


def classes_loops(imp, prune_share=None, keep_share=0.0, rows=None):
    imp = [int(x) for x in imp]
    n = len(imp)
    order = sorted(range(n), key=lambda r: (imp[r], r))
    total = sum(imp)
    cls = [1] * n
    run = 0
    for r in reversed(order):                      # from the top
        run += imp[r]
        if run > (Fraction(keep_share) * total).__floor__():
            break
        cls[r] = 2
    if prune_share is not None:
        run = 0
        for r in order:                            # from the bottom
            run += imp[r]
            if run > (Fraction(prune_share) * total).__floor__():
                break
            cls[r] = 0
    if rows is not None:
        for r in range(n):
            if any(not np.isfinite(x) or abs(float(x)) > MAX_WORD for x in np.asarray(rows[r], F)):
                cls[r] = 2
    return np.asarray(cls, np.uint8)


# ---- rule VQ-A ----

def distances(rows, codebook):
    """d [m, K] fp32: the running sum over w of (q_w - c_w)^2, every difference, product and sum rounded"""
    q, c = np.asarray(rows, F), np.asarray(codebook, F)
    d = None
    with np.errstate(all="ignore"):
        for w in range(q.shape[1]):
            t = (q[:, None, w] - c[None, :, w]).astype(F)
            tt = (t * t).astype(F)
            d = tt if d is None else (d + tt).astype(F)
    return d


def assign(rows, codebook):
    """-> (code [m] int32, dist [m] fp32): the ascending strict scan from +inf -- the first minimum, a NaN never, 0 if nothing wins"""
    d = distances(rows, codebook)
    d = np.where(np.isnan(d), INF, d)
    code = np.argmin(d, axis=1).astype(np.int32)   # the first of equal minima; all +inf -> 0
    return code, d[np.arange(d.shape[0]), code].astype(F)


def assign_loops(rows, codebook):
    q, c = np.asarray(rows, F), np.asarray(codebook, F)
    code, dist = np.zeros(q.shape[0], np.int32), np.full(q.shape[0], INF, F)
    with np.errstate(all="ignore"):
        for r in range(q.shape[0]):
            for j in range(c.shape[0]):
                d = None
                for w in range(q.shape[1]):
                    t = F(q[r, w] - c[j, w])
                    d = F(t * t) if d is None else F(d + F(t * t))
                if d < dist[r]:
                    dist[r], code[r] = d, j
    return code, dist


# ---- rule VQ-U ----

def weights(weight, m):
    """u [m] fp64 and imax"""
    if weight is None:
        return np.ones(m), 0
    weight = np.asarray(weight, np.int64)
    imax = int(weight.max()) if m else 0
    return (weight.astype(np.float64) / np.float64(imax) if imax > 0 else np.ones(m)), imax


def accumulate(rows, weight, code, K):
    """-> (S [K, W], N [K]) int64"""
    q = np.asarray(rows, F)
    u, _ = weights(weight, q.shape[0])
    S, N = np.zeros((K, q.shape[1]), np.int64), np.zeros(K, np.int64)
    ok = (code >= 0) & (code < K)
    np.add.at(S, code[ok], fix(u[ok, None] * q[ok].astype(np.float64), VQ_SHIFT))
    np.add.at(N, code[ok], fix(u[ok], VQ_SHIFT))
    return S, N


def accumulate_loops(rows, weight, code, K):
    q = np.asarray(rows, F)
    u, _ = weights(weight, q.shape[0])
    S, N = [[0] * q.shape[1] for _ in range(K)], [0] * K
    for r in range(q.shape[0]):
        j = int(code[r])
        if j < 0 or j >= K:
            continue
        for w in range(q.shape[1]):
            S[j][w] += int(fix(float(u[r]) * float(q[r, w]), VQ_SHIFT))
        N[j] += int(fix(float(u[r]), VQ_SHIFT))
    return np.asarray(S, np.int64).reshape(K, q.shape[1]), np.asarray(N, np.int64)


def update(codebook, S, N):
    """-> the new codebook (fp32); a code with N <= 0 keeps its words"""
    c = np.asarray(codebook, F).copy()
    on = N > 0
    c[on] = (S[on].astype(np.float64) / N[on].astype(np.float64)[:, None]).astype(F)
    return c


def update_loops(codebook, S, N):
    c = np.asarray(codebook, F).copy()
    for j in range(c.shape[0]):
        if N[j] > 0:
            for w in range(c.shape[1]):
                c[j, w] = F(np.float64(S[j, w]) / np.float64(N[j]))
    return c


def init(rows, weight, K):
    """codebook[j] = the row at position (j m) // K' of the order (weight descending, row ascending), K' = min(K, m)"""
    q = np.asarray(rows, F)
    m = q.shape[0]
    Kp = min(K, m)
    order = np.arange(m) if weight is None else np.lexsort((np.arange(m), -np.asarray(weight, np.int64)))
    return q[order[(np.arange(Kp) * m) // Kp]].copy()


def init_loops(rows, weight, K):
    q = np.asarray(rows, F)
    m = q.shape[0]
    Kp = min(K, m)
    order = sorted(range(m), key=lambda r: (0 if weight is None else -int(weight[r]), r))
    return np.stack([q[order[(j * m) // Kp]] for j in range(Kp)]) if Kp else q[:0].copy()


def kmeans(rows, weight, K, iters):
    """-> (codebook [K', W] fp32, code [m] int32, the codebooks after the init and after every iteration)"""
    q = np.asarray(rows, F)
    c = init(q, weight, K)
    trail = [c.copy()]
    for _ in range(iters):
        code, _ = assign(q, c)
        S, N = accumulate(q, weight, code, c.shape[0])
        c = update(c, S, N)
        trail.append(c.copy())
    return c, assign(q, c)[0], trail


def objective(rows, weight, codebook):
    """sum_r u_r min_j |q_r - c_j|^2 in fp64"""
    q, c = np.asarray(rows, np.float64), np.asarray(codebook, np.float64)
    u, _ = weights(weight, q.shape[0])
    return float((u * ((q[:, None, :] - c[None, :, :]) ** 2).sum(-1).min(1)).sum())


# ---- rule VQ-D and volume.quantize ----

def decode(cls, code, kept, codebook):
    """-> the fp16 rows [n, S]"""
    cls = np.asarray(cls)
    S = codebook.shape[1] if codebook.size or not kept.size else kept.shape[1]
    out = np.zeros((cls.size, S), H)
    out[cls == 1] = codebook[np.asarray(code, np.int64)]
    out[cls == 2] = kept
    return out


def decode_loops(cls, code, kept, codebook):
    S = codebook.shape[1] if codebook.size or not kept.size else kept.shape[1]
    out = np.zeros((len(cls), S), H)
    nc = nk = 0
    for r in range(len(cls)):
        if cls[r] == 1:
            out[r] = codebook[int(code[nc])]
            nc += 1
        elif cls[r] == 2:
            out[r] = kept[nk]
            nk += 1
    return out


def quantize(sigma_rows, coef_words, imp, K, iters, prune_share=None, keep_share=0.0):
    """volume.quantize on rows: sigma_rows [n] fp32, coef_words [n, W] fp32 (fp16 rows widened) -> dict(sigma, cls, code uint16, kept,
    codebook: fp16 rows of rule VC)"""
    q = np.asarray(coef_words, F)
    imp = np.asarray(imp, np.int64)
    cls = classes(imp, prune_share, keep_share, rows=q)
    coded = cls == 1
    c, code, _ = kmeans(q[coded], imp[coded], K, iters) if coded.any() else (q[:0], np.zeros(0, np.int32), None)
    return dict(sigma=np.where(cls == 0, F(0), np.asarray(sigma_rows, F)).astype(F), cls=cls, code=code.astype(np.uint16),
                kept=X.rows(q[cls == 2], True), codebook=X.rows(c, True))


# ---- the scene both test files use ----

DT = F(0.04)


def scene(shape, seed=11, nrays=300, degree=2):
    """make_volume with garbage at its inactive points, make_rays, the compact form's slots and rows, the geometry of the rays"""
    sigma, coef, lo, step = R.make_volume(shape, seed=seed)
    garbage, inactive = X.with_garbage(sigma, coef)
    o, d, tmin, tmax = R.make_rays(nrays, 5, lo, step, shape)
    index = R.active(garbage)
    nc = (degree + 1) ** 2
    words = np.ascontiguousarray(coef[..., :nc, :]).reshape(-1, 3 * nc)[index]
    G = GR.geometry(garbage, coef, lo, step, o, d, tmin, tmax, DT)
    zs, _ = X.zeroed(garbage, coef, inactive)
    sig = R._tri(R._corners(zs, G.ci), G.f)
    sig = np.where(G.inside, sig, F(0)).astype(F)
    return dict(sigma=garbage, coef=coef, lo=lo, step=step, o=o, d=d, tmin=tmin, tmax=tmax, index=index, slot=X.slots(index, shape),
                sigma_rows=garbage.reshape(-1)[index].copy(), words=words.astype(F), G=G, sig=sig, n=len(index))
