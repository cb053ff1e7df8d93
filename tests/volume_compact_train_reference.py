"""numpy restatements of rules VCG, VCU and VCT of include/nerf_hip.h -- rules VG, VU and VT over the rows of a compact volume, the
accumulators and the moments one per row --, beside the restatements they are held against: volume_grad_reference (V: VG, VU),
volume_refine_reference (RF: VT) and volume_compact_reference (X: pack, unpack).  Shared by tests/test_volume_compact_train_cpu.py
and tests/test_gpu_volume_compact_train.py.

VCG is V.vg with every corner looked up through its slot: ``lookup32`` fetches a sample's corner values row by row (a corner whose
slot lies outside [0, n) gives +0), ``vcg`` forms V.vg's fp64 contributions in V.vg's order and adds a corner's to the row its slot
names, dropping those of a corner without a row.  The contributions of one word arrive in the order V.vg's arrive at the row's lattice
point, so the fp64 sums are the same bits.  VCU is V.vu_step with the rows as the list.  VCT is written as the kernel is: per row, its
own three Q_a and the up to three Q_a of its backward neighbours, every neighbour reached through the slot lattice; the terms are int64.
"""
import numpy as np

import volume_grad_reference as V
import volume_reference as R
import volume_refine_reference as RF

F = np.float32


def row_points(c):
    """index[n] int32: the lattice point whose slot is r, -1 where no point names row r"""
    flat = c.slot.reshape(-1)
    n = c.sigma.shape[0]
    pts = np.flatnonzero((flat >= 0) & (flat < n))
    index = np.full(n, -1, np.int32)
    index[flat[pts]] = pts
    return index


def _rows_of(c, ci, di, dj, dk):
    """the rows of the corner (di, dj, dk) of the cells ci [M, 3] -> (row [M] clipped to an address, ok [M])"""
    n = c.sigma.shape[0]
    s = c.slot[ci[:, 0] + di, ci[:, 1] + dj, ci[:, 2] + dk].astype(np.int64)
    ok = (s >= 0) & (s < n)
    return np.where(ok, s, 0), ok


def lookup32(c, G):
    """V.lookup32 through the slots: rule VC-L in fp32 at every sample of G -> (sigma_s [M], raw [M, 3] before the clamp)"""
    nc = (c.degree + 1) ** 2
    M = G.ci.shape[0]
    sv = np.zeros((M, 2, 2, 2), F)
    cv = np.zeros((M, 2, 2, 2, nc, 3), F)
    if c.sigma.shape[0]:
        for di in (0, 1):
            for dj in (0, 1):
                for dk in (0, 1):
                    r, ok = _rows_of(c, G.ci, di, dj, dk)
                    sv[:, di, dj, dk] = np.where(ok, c.sigma[r], F(0))
                    cv[:, di, dj, dk] = np.where(ok[:, None, None], c.coef[r, :nc * 3].astype(F).reshape(M, nc, 3), F(0))
    s = R._tri(sv, G.f)
    Y = G.Y[G.rid][:, :nc]
    with np.errstate(all="ignore"):
        val = (Y[:, None, None, None, 0, None] * cv[..., 0, :]).astype(F)
        for m in range(1, nc):
            val = (val + (Y[:, None, None, None, m, None] * cv[..., m, :]).astype(F)).astype(F)
        raw = R._tri(val, G.f)
    return np.where(G.inside, s, F(0)).astype(F), np.where(G.inside[:, None], raw, F(0)).astype(F)


def vcg(c, G, idx, valid, w, Tn, col, mask, g_rgb, g_maps, bg):
    """Rule VCG's closed form in fp64 (V.vg's brackets) -> (d_sigma_rows [n], d_coef_rows [n, nc, 3]) fp64, unquantised"""
    nc = (c.degree + 1) ** 2
    n = c.sigma.shape[0]
    dt = np.float64(G.dt)
    j = np.maximum(idx, 0)
    g, gD, gA1, ok = V._upstream(G, g_rgb, g_maps, bg)
    valid = valid & ok[:, None]
    w64, T64 = np.where(valid, w.astype(np.float64), 0.0), Tn.astype(np.float64)
    c64 = col[j].astype(np.float64)
    v = (((g[:, None, 0] * c64[..., 0] + g[:, None, 1] * c64[..., 1]) + g[:, None, 2] * c64[..., 2]) + gD[:, None] * G.tk[j].astype(np.float64)) + gA1[:, None]
    wv = w64 * v
    P = np.cumsum(wv, axis=1)
    S = P[:, -1:]
    dsig = np.where(valid, dt * (T64 * v - (S - P)), 0.0)
    dc = np.where(valid[..., None] & mask[j], w64[..., None] * g[:, None, :], 0.0)
    tw, _ = V._corner_terms(G, idx)
    dS, dC = np.zeros(n), np.zeros((n, nc, 3))
    Y = G.Y.astype(np.float64)[:, :nc]
    ci = G.ci[j]
    for cnr in range(8):
        row, has = _rows_of(c, ci.reshape(-1, 3), (cnr >> 2) & 1, (cnr >> 1) & 1, cnr & 1)
        row, sel = row.reshape(idx.shape), valid & has.reshape(idx.shape)      # a corner without a row receives nothing
        np.add.at(dS, row[sel], (tw[..., cnr] * dsig)[sel])
        term = (tw[..., cnr][..., None] * Y[:, None, :])[..., None] * dc[..., None, :]
        np.add.at(dC, row[sel], term[sel])
    return dS, dC


def reference(c, G, g_rgb, g_maps, bg, t_stop=0.0):
    """V.reference over the compact volume c (fp32 rows) -> dict(dS [n], dC [n, nc, 3], sig, idx, valid)"""
    sig, raw = lookup32(c, G)
    col, mask = V.clamp_mask(raw)
    idx = V.pad(G, sig)
    _, w, Tn, valid = V.forward(G, sig, idx, np.float64, t_stop)
    dS, dC = vcg(c, G, idx, valid, w, Tn, col, mask, g_rgb, g_maps, bg)
    return dict(dS=dS, dC=dC, sig=sig, idx=idx, valid=valid)


def vcu_step(sigma_rows, coef_rows, acc_sigma, acc_coef, m, v, grad_scale, step, lr_sigma, lr_coef, beta1=0.9, beta2=0.999, eps=1e-8):
    """Rule VCU IN PLACE on sigma_rows [n], coef_rows [n, 3 nc] (fp32), m, v [n, 1 + 3 nc] and the accumulators [n], [n, 3 nc]: rule VU
    with the rows as the list -- the rows seen as a lattice n x 1 x 1 whose active list is every point in order."""
    n, nc = sigma_rows.shape[0], coef_rows.shape[1] // 3
    V.vu_step(sigma_rows.reshape(n, 1, 1), coef_rows.reshape(n, 1, 1, nc, 3), np.arange(n), acc_sigma, acc_coef, m, v, grad_scale, step,
              lr_sigma, lr_coef, beta1, beta2, eps)


def _tv_terms(c, X, shape, ijk, row, w, eps):
    """rule VT's Q_x, Q_y, Q_z [3][k, W] int64 at the members ijk [k, 3] whose rows are row [k]; X [n, W] fp64 are the rows' words"""
    n = X.shape[0]
    x0 = X[row]
    d = np.zeros((3,) + x0.shape)
    for a in range(3):
        far = ijk.copy()
        far[:, a] += 1
        inside = far[:, a] < shape[a]
        far[:, a] = np.minimum(far[:, a], shape[a] - 1)
        s = c.slot[far[:, 0], far[:, 1], far[:, 2]].astype(np.int64)
        ok = inside & (s >= 0) & (s < n)                                       # the slot is compared with n before it is used
        with np.errstate(all="ignore"):
            d[a] = np.where(ok[:, None], X[np.where(ok, s, 0)] - x0, 0.0)
    tau = RF.tv_tau(d, eps)
    with np.errstate(all="ignore"):
        return [RF.fix(w * (d[a] / tau)) for a in range(3)]


def vct(c, point, w_sigma, w_coef, eps, acc_sigma, acc_coef):
    """Rule VCT IN PLACE on the int64 accumulators acc_sigma [n], acc_coef [n, 3 nc]: per row, a gather through the slot lattice"""
    n = c.sigma.shape[0]
    nc = (c.degree + 1) ** 2
    shape = c.slot.shape
    point = np.asarray(point, np.int64)
    flat = c.slot.reshape(-1)
    rows = np.flatnonzero((point >= 0) & (point < flat.size))
    s = flat[point[rows]]
    rows = rows[(s >= 0) & (s < n) & (s == rows)]                              # the row's point is a member, and names this row
    if rows.size == 0 or (w_sigma == 0 and w_coef == 0):
        return
    X = np.concatenate([c.sigma[:, None], c.coef[:, :3 * nc].astype(F)], axis=1).astype(np.float64)
    w = np.concatenate([[float(w_sigma)], np.full(3 * nc, float(w_coef))])
    ijk = np.stack(np.unravel_index(point[rows], shape), axis=1)
    Q = _tv_terms(c, X, shape, ijk, rows, w, eps)
    total = -Q[0] - Q[1] - Q[2]
    for a in range(3):
        back = ijk.copy()
        back[:, a] -= 1
        inside = back[:, a] >= 0
        back[:, a] = np.maximum(back[:, a], 0)
        sb = c.slot[back[:, 0], back[:, 1], back[:, 2]].astype(np.int64)
        ok = inside & (sb >= 0) & (sb < n)
        if ok.any():
            total[ok] += _tv_terms(c, X, shape, back[ok], sb[ok], w, eps)[a]
    acc_sigma[rows] += total[:, 0]                                             # (a weight of 0 gives terms of 0)
    acc_coef.reshape(n, -1)[rows] += total[:, 1:]


def gather(dense_sigma_like, dense_coef_like, index):
    """the words of the lattice points index [n] of dense arrays -> ([n], [n, 3 nc])"""
    index = np.asarray(index, np.int64)
    nw = int(np.prod(dense_coef_like.shape[3:]))
    return dense_sigma_like.reshape(-1)[index], dense_coef_like.reshape(-1, nw)[index]
