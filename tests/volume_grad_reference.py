"""numpy restatements of rules VG and VU of include/nerf_hip.h (the gradient of the SH volume march and the Adam step over the baked
active list), vectorised over rays, and the word-by-word error budget the device accumulators have to meet against the fp64
restatement.  Shared by tests/test_volume_grad_cpu.py and tests/test_gpu_volume_grad.py.  Built on volume_reference (make_volume,
make_rays, ray_samples, cells and its interpolation helpers).

THE RESTATEMENT.  ``geometry`` fixes what does not depend on the volume's values: every ray's samples (t_k, cell, f: rule VR / VL in
fp32).  ``lookup32`` is rule VL in fp32 at all samples at once, before the clamp.  ``forward`` is the compositing recurrence over the
contributing samples in fp32 (what the device computes) or in fp64 (the reference, on the rule's own fp32 sample values), and ``vg`` is
rule VG's closed form in fp64 on whatever (w, T, c, mask) it is given.

THE BUDGET (derived, never fitted).  u = 2^-24.  The device evaluates VG in fp64 on ITS fp32 (w_i, T_(i+1)); the reference evaluates it
on the fp64 recurrence over the same fp32 (sigma_s, c_i, t_i).  volume_reference's THE BOUND gives, for the error e_i of T after i
contributing samples and the error dw_i of w_i,
      e_i <= 7 u i,        |dw_i| <= e_(i-1) alpha_i + 6 u <= 7 u (i - 1) alpha_i + 6 u        (sum_i |dw_i| <= 13 u n).
c_i, t_i, f, Y_m(d), dt and the upstream values are the same numbers on both sides, and v_i depends on none of (w, T).  So
  * a coefficient contribution (tw Y_m) (w_i g_ch) errs by at most |tw Y_m g_ch| |dw_i|;
  * a sigma contribution tw dt (T_(i+1) v_i - sum_(j>i) w_j v_j) errs by at most tw dt (|v_i| e_i + sum_(j>i) |dw_j| |v_j|);
  * each contribution is rounded to a multiple of 2^-40: 2^-41 more per contribution;
and a word's budget is the sum of these over what it received, times (1 + 2^-10) for the second-order terms and the fp64 roundings.
It inherits volume_reference's ASSUMPTION that expm1f is good to 2 ulp (the project carries no copy of the HIP math accuracy table):
an assumption, not a documented figure.
"""
import numpy as np

import volume_reference as R

F = np.float32
U = R.U
SHIFT = 40
QUANT = 2.0 ** -(SHIFT + 1)


class Geo:
    pass


def geometry(sigma, coef, lo, step, o, d, tmin, tmax, dt):
    """The samples of every ray, concatenated: rid [M] (the ray), tk [M] fp32, ci [M, 3], f [M, 3] fp32, inside [M]; Y [N, 9] fp32.
    (sigma and coef only feed volume_reference.ray_samples; nothing kept here depends on their values.)"""
    o, d = np.asarray(o, F).reshape(-1, 3), np.asarray(d, F).reshape(-1, 3)
    N = o.shape[0]
    tmin, tmax = np.broadcast_to(np.asarray(tmin, F), (N,)), np.broadcast_to(np.asarray(tmax, F), (N,))
    rid, tk, x = [], [], []
    for r in range(N):
        s = R.ray_samples(sigma, coef, lo, step, o[r], d[r], tmin[r], tmax[r], dt)
        if s is None or s["K"] == 0:
            continue
        rid.append(np.full(s["K"], r))
        tk.append(s["tk"])
        with np.errstate(all="ignore"):
            x.append((o[r][None, :] + (s["tk"][:, None] * d[r][None, :]).astype(F)).astype(F))
    G = Geo()
    G.N, G.shape, G.dt = N, tuple(sigma.shape), F(dt)
    G.rid = np.concatenate(rid) if rid else np.zeros(0, np.int64)
    G.tk = np.concatenate(tk) if tk else np.zeros(0, F)
    xs = np.concatenate(x) if x else np.zeros((0, 3), F)
    G.inside, G.ci, G.f = R.cells(xs, lo, step, sigma.shape)
    G.d = d
    with np.errstate(all="ignore"):
        G.Y = R.basis32(d)
    return G


def lookup32(sigma, coef, G):
    """Rule VL in fp32 at every sample of G -> (sigma_s [M], raw [M, 3]: the colour BEFORE its clamp); zeros outside the lattice."""
    nc = coef.shape[3]
    s = R._tri(R._corners(np.asarray(sigma, F), G.ci), G.f)
    Y = G.Y[G.rid][:, :nc]
    cc = R._corners(np.asarray(coef, F), G.ci)
    with np.errstate(all="ignore"):
        val = (Y[:, None, None, None, 0, None] * cc[..., 0, :]).astype(F)
        for m in range(1, nc):
            val = (val + (Y[:, None, None, None, m, None] * cc[..., m, :]).astype(F)).astype(F)
        raw = R._tri(val, G.f)
    return np.where(G.inside, s, F(0)).astype(F), np.where(G.inside[:, None], raw, F(0)).astype(F)


def clamp_mask(raw):
    """-> (c = fmin(fmax(raw, 0), 1), mask = raw in [0, 1], both ends included)"""
    with np.errstate(all="ignore"):
        return np.fmin(np.fmax(raw, F(0)), F(1)).astype(raw.dtype), (raw >= 0) & (raw <= 1)


def pad(G, sig, limit=None, drop=None):
    """The contributing samples (sigma_s > 0) of every ray, in order -> idx [N, Mx] into G's samples, -1 beyond a ray's last one.
    limit [N]: at most that many per ray.  drop = (ray, ordinal): that contributing sample is left out (the tests' teeth)."""
    con = np.flatnonzero(sig > 0)
    rid = G.rid[con]
    first = np.searchsorted(rid, np.arange(G.N))
    ordn = np.arange(con.size) - first[rid]
    if drop is not None:
        keep = ~((rid == drop[0]) & (ordn == drop[1]))
        con, rid = con[keep], rid[keep]
        first = np.searchsorted(rid, np.arange(G.N))
        ordn = np.arange(con.size) - first[rid]
    if limit is not None:
        keep = ordn < np.asarray(limit)[rid]
        con, rid, ordn = con[keep], rid[keep], ordn[keep]
    idx = np.full((G.N, int(ordn.max()) + 1 if con.size else 1), -1, np.int64)
    idx[rid, ordn] = con
    return idx


def forward(G, sig, idx, dtype, t_stop=0.0, dt=None):
    """Rule VR's recurrence over the padded contributing samples in ``dtype`` (np.float32: as the device; np.float64: the reference)
    -> (alpha, w, Tn = T after the sample, valid) [N, Mx]; a ray ends after the sample that brings T below t_stop."""
    T_ = dtype
    dt = T_(G.dt if dt is None else dt)
    N, Mx = idx.shape
    alpha, w, Tn = np.zeros((N, Mx), T_), np.zeros((N, Mx), T_), np.zeros((N, Mx), T_)
    valid = np.zeros((N, Mx), bool)
    T = np.ones(N, T_)
    alive = np.ones(N, bool)
    for i in range(Mx):
        on = alive & (idx[:, i] >= 0)
        s = sig[np.maximum(idx[:, i], 0)].astype(T_)
        with np.errstate(all="ignore"):
            a = (-np.expm1((-((s * dt).astype(T_))).astype(T_))).astype(T_)
            wi = (T * a).astype(T_)
            Tnew = (T - wi).astype(T_)
        alpha[:, i], w[:, i], Tn[:, i] = np.where(on, a, 0), np.where(on, wi, 0), np.where(on, Tnew, 0)
        valid[:, i] = on
        T = np.where(on, Tnew, T).astype(T_)
        alive = on & ~(T < T_(t_stop))
    return alpha, w, Tn, valid


def composite(G, idx, valid, w, c, bg):
    """-> rgb [N, 3], maps [N, 2] fp64 of the given weights"""
    j = np.maximum(idx, 0)
    wv = np.where(valid, w.astype(np.float64), 0.0)
    C = (wv[..., None] * c[j].astype(np.float64)).sum(1)
    A = wv.sum(1)
    D = (wv * G.tk[j].astype(np.float64)).sum(1)
    return C + (1.0 - A)[:, None] * np.asarray(bg, np.float64), np.stack([D, A], 1)


def _corner_terms(G, idx):
    """per padded sample and corner c = di * 4 + dj * 2 + dk: tw [N, Mx, 8] fp64 and the corner's linear index [N, Mx, 8]"""
    j = np.maximum(idx, 0)
    f = G.f[j].astype(np.float64)
    ci = G.ci[j]
    nx, ny, nz = G.shape
    tw, lin = [], []
    for c in range(8):
        di, dj, dk = (c >> 2) & 1, (c >> 1) & 1, c & 1
        wx = f[..., 0] if di else 1.0 - f[..., 0]
        wy = f[..., 1] if dj else 1.0 - f[..., 1]
        wz = f[..., 2] if dk else 1.0 - f[..., 2]
        tw.append((wx * wy) * wz)
        lin.append(((ci[..., 0] + di) * ny + (ci[..., 1] + dj)) * nz + (ci[..., 2] + dk))
    return np.stack(tw, -1), np.stack(lin, -1)


def _upstream(G, g_rgb, g_maps, bg, no_bg=False):
    g = np.asarray(g_rgb, np.float64).reshape(G.N, 3)
    gm = np.zeros((G.N, 2)) if g_maps is None else np.asarray(g_maps, np.float64).reshape(G.N, 2)
    ok = np.isfinite(g).all(1) & np.isfinite(gm).all(1)
    g, gm = np.where(ok[:, None], g, 0.0), np.where(ok[:, None], gm, 0.0)
    bgv = np.asarray(bg, np.float64)
    gA1 = gm[:, 1] - (0.0 if no_bg else ((g[:, 0] * bgv[0] + g[:, 1] * bgv[1]) + g[:, 2] * bgv[2]))
    return g, gm[:, 0], gA1, ok


def vg(G, idx, valid, w, Tn, c, mask, g_rgb, g_maps, bg, nc, dt=None, mutate=None):
    """Rule VG's closed form in fp64 on the given (w, Tn [N, Mx]; c, mask [M, 3]) -> (d_sigma [npts], d_coef [npts, nc, 3]) fp64,
    unquantised.  mutate: None, or one of the wrong versions the budget has to reject: "P_exclusive" (P_i without sample i's own
    term), "no_mask" (the clamp mask ignored), "no_bg" (the background term of gA' left out)."""
    dt = np.float64(G.dt if dt is None else dt)
    j = np.maximum(idx, 0)
    g, gD, gA1, ok = _upstream(G, g_rgb, g_maps, bg, no_bg=mutate == "no_bg")
    valid = valid & ok[:, None]
    w64, T64 = np.where(valid, w.astype(np.float64), 0.0), Tn.astype(np.float64)
    c64 = c[j].astype(np.float64)
    v = (((g[:, None, 0] * c64[..., 0] + g[:, None, 1] * c64[..., 1]) + g[:, None, 2] * c64[..., 2]) + gD[:, None] * G.tk[j].astype(np.float64)) + gA1[:, None]
    wv = w64 * v
    P = np.cumsum(wv, axis=1)
    S = P[:, -1:]
    Pi = P - wv if mutate == "P_exclusive" else P
    dsig = np.where(valid, dt * (T64 * v - (S - Pi)), 0.0)
    m = np.ones_like(mask[j]) if mutate == "no_mask" else mask[j]
    dc = np.where(valid[..., None] & m, w64[..., None] * g[:, None, :], 0.0)
    tw, lin = _corner_terms(G, idx)
    npts = int(np.prod(G.shape))
    dS, dC = np.zeros(npts), np.zeros((npts, nc, 3))
    Y = G.Y.astype(np.float64)[:, :nc]
    sel = valid
    for cnr in range(8):
        np.add.at(dS, lin[..., cnr][sel], (tw[..., cnr] * dsig)[sel])
        term = (tw[..., cnr][..., None] * Y[:, None, :])[..., None] * dc[..., None, :]      # [N, Mx, nc, 3]
        np.add.at(dC, lin[..., cnr][sel], term[sel])
    return dS, dC


def budget(G, idx, valid, alpha64, c, mask, g_rgb, g_maps, bg, nc):
    """THE BUDGET of the module docstring, word by word -> (b_sigma [npts], b_coef [npts, nc, 3]); 0 where a word received nothing."""
    dt = np.float64(G.dt)
    j = np.maximum(idx, 0)
    g, gD, gA1, ok = _upstream(G, g_rgb, g_maps, bg)
    valid = valid & ok[:, None]
    c64 = c[j].astype(np.float64)
    v = np.abs((((g[:, None, 0] * c64[..., 0] + g[:, None, 1] * c64[..., 1]) + g[:, None, 2] * c64[..., 2]) + gD[:, None] * G.tk[j].astype(np.float64)) + gA1[:, None])
    i1 = np.arange(1, idx.shape[1] + 1, dtype=np.float64)[None, :]            # the 1-based ordinal
    e = 7 * U * i1
    dw = np.where(valid, 7 * U * (i1 - 1) * alpha64.astype(np.float64) + 6 * U, 0.0)
    dwv = dw * np.where(valid, v, 0.0)
    later = dwv[:, ::-1].cumsum(1)[:, ::-1] - dwv                             # sum over j > i
    bs = np.where(valid, dt * (v * e + later), 0.0)
    bc = np.where(valid[..., None] & mask[j], dw[..., None] * np.abs(g)[:, None, :], 0.0)
    tw, lin = _corner_terms(G, idx)
    npts = int(np.prod(G.shape))
    bS, bC = np.zeros(npts), np.zeros((npts, nc, 3))
    Y = np.abs(G.Y.astype(np.float64)[:, :nc])
    for cnr in range(8):
        np.add.at(bS, lin[..., cnr][valid], (tw[..., cnr] * bs + QUANT)[valid])
        term = (tw[..., cnr][..., None] * Y[:, None, :])[..., None] * bc[..., None, :] + QUANT
        np.add.at(bC, lin[..., cnr][valid], term[valid])
    return bS * (1 + 2.0 ** -10), bC * (1 + 2.0 ** -10)


def reference(sigma, coef, G, g_rgb, g_maps, bg, t_stop=0.0, limit=None):
    """The fp64 restatement of VG for a volume and the rays of G, with its budget -> dict(dS, dC, bS, bC, idx, valid, ...); limit [N]:
    every ray truncated at that many contributing samples (the device forward's own steps[:, 0])."""
    nc = coef.shape[3]
    sig, raw = lookup32(sigma, coef, G)
    c, mask = clamp_mask(raw)
    idx = pad(G, sig, limit=limit)
    alpha, w, Tn, valid = forward(G, sig, idx, np.float64, t_stop)
    dS, dC = vg(G, idx, valid, w, Tn, c, mask, g_rgb, g_maps, bg, nc)
    bS, bC = budget(G, idx, valid, alpha, c, mask, g_rgb, g_maps, bg, nc)
    return dict(dS=dS, dC=dC, bS=bS, bC=bC, idx=idx, valid=valid, sig=sig, raw=raw, c=c, mask=mask, alpha=alpha, w=w, Tn=Tn)


def worst_ratio(got_S, got_C, ref):
    """max over the words of |got - reference| / budget (got in gradient units); a word with a zero budget must be exactly zero"""
    worst = 0.0
    for got, want, b in ((got_S, ref["dS"], ref["bS"]), (got_C, ref["dC"], ref["bC"])):
        got = np.asarray(got, np.float64).reshape(want.shape)
        zero = b == 0
        if (got[zero] != 0).any():
            return np.inf
        if (~zero).any():
            worst = max(worst, float((np.abs(got - want)[~zero] / b[~zero]).max()))
    return worst


# ---- VU ----

def pow_by_squaring(beta, step):
    p, b, e = 1.0, float(beta), int(step)
    while e > 0:
        if e & 1:
            p = p * b
        b = b * b
        e >>= 1
    return p


def vu_step(sigma, coef, index, acc_sigma, acc_coef, m, v, grad_scale, step, lr_sigma, lr_coef, beta1=0.9, beta2=0.999, eps=1e-8):
    """Rule VU in numpy, IN PLACE on sigma [nx, ny, nz], coef [nx, ny, nz, nc, 3] (fp32), m, v [n, 1 + 3 nc] (fp32) and the
    accumulators (int64, or fp64 holding unrounded sums in the same 2^-40 units), which are zeroed over the list."""
    nc = coef.shape[3]
    sg, cf = sigma.reshape(-1), coef.reshape(-1, 3 * nc)
    aS, aC = acc_sigma.reshape(-1), acc_coef.reshape(-1, 3 * nc)
    c1, c2 = 1.0 - pow_by_squaring(beta1, step), 1.0 - pow_by_squaring(beta2, step)
    index = np.asarray(index, np.int64)
    x = np.concatenate([sg[index][:, None], cf[index]], axis=1).astype(np.float64)
    acc = np.concatenate([aS[index][:, None], aC[index]], axis=1).astype(np.float64)
    lr = np.concatenate([[float(lr_sigma)], np.full(3 * nc, float(lr_coef))])[None, :]
    g = (acc * 2.0 ** -SHIFT) * float(grad_scale)
    with np.errstate(all="ignore"):
        m1 = (beta1 * m.astype(np.float64) + (1.0 - beta1) * g).astype(F)
        v1 = (beta2 * v.astype(np.float64) + (1.0 - beta2) * (g * g)).astype(F)
        x1 = (x - lr * ((m1.astype(np.float64) / c1) / (np.sqrt(v1.astype(np.float64) / c2) + eps))).astype(F)
        x1[:, 0] = np.fmax(x1[:, 0], F(0))
    live = np.ones(x.shape, bool)
    live[:, 0] = sg[index] > 0                       # a dead sigma keeps x, m and v
    m[...] = np.where(live, m1, m)
    v[...] = np.where(live, v1, v)
    xn = np.where(live, x1, x.astype(F)).astype(F)
    sg[index] = xn[:, 0]
    cf[index] = xn[:, 1:]
    aS[index] = 0
    aC[index] = 0


# ---- the learning case both test files run ----

LEARN_SHAPE = (9, 8, 7)
LEARN_DT = F(0.04)
LEARN_BG = (0.25, 0.5, 1.0)
LEARN_STEPS = 25


def learning_case():
    """lattice (9, 8, 7): make_volume(seed=11) as teacher; the first 64 of make_rays(.., 5, ..); the student is the teacher with sigma
    x U(0.6, 1.4) and coefficients + N(0, 0.2) on the active points -> dict(teacher, student, rays, G, target [64, 3] fp32: the
    restatement's fp64 render of the teacher, rounded)."""
    sigma, coef, lo, step = R.make_volume(LEARN_SHAPE, seed=11)
    o, d, tmin, tmax = R.make_rays(300, 5, lo, step, LEARN_SHAPE)
    o, d, tmin, tmax = o[:64], d[:64], tmin[:64], tmax[:64]
    rng = np.random.default_rng(23)
    index = R.active(sigma)
    s2 = (sigma * rng.uniform(0.6, 1.4, sigma.shape)).astype(F)
    c2 = coef.copy().reshape(-1, coef.shape[3], 3)
    c2[index] = (c2[index] + rng.normal(0.0, 0.2, c2[index].shape)).astype(F)
    c2 = c2.reshape(coef.shape)
    G = geometry(sigma, coef, lo, step, o, d, tmin, tmax, LEARN_DT)
    target = render64(sigma, coef, G, LEARN_BG)[0].astype(F)
    return dict(sigma=sigma, coef=coef, lo=lo, step=step, o=o, d=d, tmin=tmin, tmax=tmax, index=index, s2=s2, c2=c2, G=G, target=target)


def render64(sigma, coef, G, bg, t_stop=0.0):
    sig, raw = lookup32(sigma, coef, G)
    c, _ = clamp_mask(raw)
    idx = pad(G, sig)
    _, w, _, valid = forward(G, sig, idx, np.float64, t_stop)
    return composite(G, idx, valid, w, c, bg)


def learn(case, steps=LEARN_STEPS, lr_sigma=0.1, lr_coef=0.01):
    """Finetuner.step in the restatement: fp32 lookups, the fp64 composite, VG's closed form (unquantised), VU -> the losses [steps + 1]
    (the last one after the final update) and the final (sigma, coef)."""
    G, bg = case["G"], LEARN_BG
    sigma, coef = case["s2"].copy(), case["c2"].copy()
    nc = coef.shape[3]
    index = case["index"]
    m, v = np.zeros((index.size, 1 + 3 * nc), F), np.zeros((index.size, 1 + 3 * nc), F)
    target = case["target"].astype(np.float64)
    losses = []
    for it in range(steps + 1):
        sig, raw = lookup32(sigma, coef, G)
        c, mask = clamp_mask(raw)
        idx = pad(G, sig)
        _, w, Tn, valid = forward(G, sig, idx, np.float64, 0.0)
        rgb = composite(G, idx, valid, w, c, bg)[0].astype(F).astype(np.float64)
        diff = rgb - target
        losses.append(float((diff * diff).mean()))
        if it == steps:
            break
        dS, dC = vg(G, idx, valid, w, Tn, c, mask, (2.0 * diff).astype(F), None, bg, nc)
        vu_step(sigma, coef, index, dS * 2.0 ** SHIFT, dC.reshape(-1) * 2.0 ** SHIFT, m, v, 1.0 / (3 * G.N), it + 1, lr_sigma, lr_coef)
    return np.asarray(losses), sigma, coef
