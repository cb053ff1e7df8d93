"""numpy restatements of rules VM, VT, VX and VP of include/nerf_hip.h (the member mask, the total-variation prior added to rule VG's
integer accumulators, the x2 refinement and the prune), the bound a refined lookup has to meet against the coarse one, and the
level-by-level learning loop.  Shared by tests/test_volume_refine_cpu.py and tests/test_gpu_volume_refine.py.  Built on
volume_reference (R) and volume_grad_reference (V).

VT is restated over the WHOLE lattice: a point that is not a member has all its differences 0, so its Q_a are 0 and it receives
nothing; ``vt`` then adds the totals of the rows of ``index`` only (a chunk of the list adds its own rows).  The arithmetic is fp64 as
the rule brackets it and the terms are int64, so the restatement is bit for bit what the device must hold.

THE LOOKUP BOUND (derived, never fitted).  u = 2^-24.  Take a point x inside the box; its coarse cell has the fraction f per axis
and the fine lattice the fraction f' = 2 f or 2 f - 1 of one half of that cell.  In exact arithmetic the fine lookup IS the coarse
one: the refined values are the trilinear interpolant at the half points and a trilinear function restricted to an octant is the
trilinear interpolant of its corner values.  What differs are roundings.  With M the largest corner magnitude, every intermediate
of a lerp chain is a value of the interpolant up to rounding, so |b - a| <= 2 M and each lerp a + f (b - a) commits three roundings
(the difference, the product, the sum) of quantities <= 2 M: at most 3 x 2 M u = 6 M u, and passes on the errors of its two inputs
with weights (1 - f) + f = 1.
  * a refined value is at most three lerps deep:                           3 x 6 M u = 18 M u
  * the fine lookup is three lerps deep on values wrong by <= 18 M u:      18 M u + 18 M u = 36 M u
  * the coarse lookup is three lerps deep on exact values:                 18 M u
  * f and f' are themselves rounded: g = (x - lo) / step is two roundings of a number <= n, and the fine g' = 2 g exactly when the
    same (x - lo) is divided by step / 2 (a power-of-two scaling), so f' = g' - i' is the same real number as 2 f (- 1) and the
    subtraction of the integer part is exact in both (Sterbenz / an integer below 2^24): NO term.
So |fine - coarse| <= 54 M u for sigma, within the issue's loose count of 64 M u: LOOKUP_ULPS = 64 is used, times (1 + 2^-10) for
second order.  A colour corner value s = sum_m Y_m c_m is the same expression on both sides, but on the fine side its inputs are
refined coefficients: nc products and nc - 1 sums, each <= u times a partial sum <= Ysum C (Ysum = sum_m |Y_m|, C the largest
coefficient magnitude), so the corner value errs by <= 18 C u Ysum (the refined coefficients' own error through the sum) and the two
evaluations of the sum each commit <= (2 nc - 1) u Ysum C.  With M_c = Ysum C bounding every corner colour:
|fine - coarse| <= (64 + 2 (2 nc - 1)) M_c u (1 + 2^-10) before the clamp, and the clamp to [0, 1] does not increase a difference.
"""
import numpy as np

import volume_grad_reference as V
import volume_reference as R

F = np.float32
U = R.U
SHIFT = V.SHIFT
LOOKUP_ULPS = 64


# ---- VM ----

def member_mask(index, shape):
    npts = int(np.prod(shape))
    index = np.asarray(index, np.int64).reshape(-1)
    m = np.zeros(npts, np.uint8)
    m[index[(index >= 0) & (index < npts)]] = 1
    return m.reshape(shape)


# ---- VT ----

def fix(x):
    """Rule VG's fixed point of the fp64 array x -> int64"""
    with np.errstate(all="ignore"):
        y = np.clip(x * 2.0 ** SHIFT, -2.0 ** 62, 2.0 ** 62)
        return np.where(np.isnan(x), 0.0, np.rint(y)).astype(np.int64)


def words(sigma, coef):
    """[nx, ny, nz, 1 + 3 nc]: a point's words, sigma first"""
    return np.concatenate([np.asarray(sigma)[..., None], np.asarray(coef).reshape(sigma.shape + (-1,))], axis=-1)


def _axis_slices(a):
    near = [slice(None)] * 3
    far = [slice(None)] * 3
    near[a], far[a] = slice(None, -1), slice(1, None)
    return tuple(near), tuple(far)


def tv_differences(X, member, mutate=None):
    """d [3, nx, ny, nz, W] fp64: rule VT's differences of the words X (fp64) over the mask.  mutate "no_far_member": the far end's
    membership is not tested (a planted mistake)."""
    mem = np.asarray(member).astype(bool)
    d = np.zeros((3,) + X.shape)
    for a in range(3):
        near, far = _axis_slices(a)
        ok = mem[near] if mutate == "no_far_member" else mem[near] & mem[far]
        with np.errstate(all="ignore"):
            d[a][near] = np.where(ok[..., None], X[far] - X[near], 0.0)
    return d


def tv_tau(d, eps, mutate=None):
    with np.errstate(all="ignore"):
        ss = ((d[0] * d[0]) + (d[1] * d[1])) + (d[2] * d[2])
        return np.sqrt(ss) + eps if mutate == "eps_outside" else np.sqrt(ss + eps)


def tv_totals(sigma, coef, member, w_sigma, w_coef, eps, mutate=None):
    """What every word of the lattice receives from rule VT -> int64 [nx, ny, nz, W].  mutate: None, "no_far_member", "eps_outside",
    or "no_backward" (the +Q_a(p - e_a) terms dropped): the planted mistakes."""
    X = words(sigma, coef).astype(np.float64)
    W = X.shape[-1]
    w = np.concatenate([[float(w_sigma)], np.full(W - 1, float(w_coef))])
    mem = np.asarray(member).astype(bool)
    d = tv_differences(X, member, mutate)
    tau = tv_tau(d, eps, mutate)
    total = np.zeros(X.shape, np.int64)
    for a in range(3):
        with np.errstate(all="ignore"):
            Q = np.where(mem[..., None], fix(w * (d[a] / tau)), 0)
        total -= Q
        if mutate != "no_backward":
            near, far = _axis_slices(a)
            total[far] += Q[near]
    return total


def tv_loss(sigma, coef, member, w_sigma, w_coef, eps):
    """The loss rule VT differentiates, in fp64: w_sigma sum_p tau_sigma(p) + w_coef sum_p sum_words tau(p) over the members"""
    X = words(sigma, coef).astype(np.float64)
    tau = tv_tau(tv_differences(X, member), eps)
    mem = np.asarray(member).astype(bool)
    return float(w_sigma) * tau[..., 0][mem].sum() + float(w_coef) * tau[..., 1:][mem].sum()


def vt(sigma, coef, index, member, w_sigma, w_coef, eps, acc_sigma, acc_coef, mutate=None):
    """Rule VT IN PLACE on the int64 accumulators (sigma's and coef's shapes) for the rows of ``index``"""
    total = tv_totals(sigma, coef, member, w_sigma, w_coef, eps, mutate).reshape(-1, 1 + 3 * coef.shape[3])
    npts = total.shape[0]
    index = np.asarray(index, np.int64).reshape(-1)
    index = index[(index >= 0) & (index < npts)]
    index = index[np.asarray(member).reshape(-1)[index] != 0]
    aS, aC = acc_sigma.reshape(-1), acc_coef.reshape(npts, -1)
    aS[index] += total[index, 0]
    aC[index] += total[index, 1:]


# ---- VX ----

def _up_axis(v, axis, f=0.5):
    v = np.moveaxis(np.asarray(v, F), axis, 0)
    out = np.empty((2 * v.shape[0] - 1,) + v.shape[1:], F)
    out[0::2] = v
    with np.errstate(all="ignore"):
        out[1::2] = (v[:-1] + (F(f) * (v[1:] - v[:-1]).astype(F)).astype(F)).astype(F)
    return np.moveaxis(out, 0, axis)


def vx(sigma, coef, f=0.5):
    """Rule VX as the three separable passes, z first, then y, then x -> (sigma2, coef2).  f != 0.5 is a planted mistake."""
    for axis in (2, 1, 0):
        sigma, coef = _up_axis(sigma, axis, f), _up_axis(coef, axis, f)
    return np.ascontiguousarray(sigma), np.ascontiguousarray(coef)


def up_shape(shape):
    return tuple(2 * n - 1 for n in shape)


def half_step(step):
    return (np.asarray(step, F) * F(0.5)).astype(F)


def lookup_bounds(sigma, coef, d):
    """-> (bound of |fine - coarse| sigma lookups, the same for colours along the directions d [M, 3] -> [M]): the module docstring's"""
    nc = coef.shape[3]
    Ms = float(np.abs(np.asarray(sigma, np.float64)).max())
    C = float(np.abs(np.asarray(coef, np.float64)).max())
    Ysum = np.abs(R.basis32(d).astype(np.float64))[:, :nc].sum(1)
    k = 1 + 2.0 ** -10
    return LOOKUP_ULPS * Ms * U * k, (LOOKUP_ULPS + 2 * (2 * nc - 1)) * (Ysum * C) * U * k


# ---- VP ----

def vp(sigma, coef, threshold):
    """Rule VP on copies -> (sigma', coef')"""
    sigma = np.asarray(sigma, F)
    with np.errstate(all="ignore"):
        s = np.where(sigma > F(threshold), sigma, F(0)).astype(F)
    act = R.active(s)
    c = np.zeros(coef.shape, F).reshape(-1, coef.shape[3], 3)
    c[act] = np.asarray(coef, F).reshape(c.shape)[act]
    return s, c.reshape(coef.shape)


# ---- the learning loop, level by level ----

def learn_levels(case, steps=V.LEARN_STEPS, upsample_at=(), tv=(0.0, 0.0), prune=None, lr_sigma=0.1, lr_coef=0.01, tv_eps=1e-9):
    """Finetuner / finetune in the restatement on volume_grad_reference.learning_case: fp32 lookups, the fp64 composite, VG's closed
    form (unquantised) plus VT's integers, VU; at every step count of ``upsample_at`` the volume is pruned (``prune`` not None) and
    refined, and a fresh level starts (a new active list, zero moments, the bias correction at step 1).  The march keeps the case's
    dt on every level, so a level switch only re-expresses the same samples on the finer lattice.
    -> dict(losses [steps + 1] (the last one after the final update), switches = [(the coarse state's loss, the refined state's)],
    sigma, coef, lo, step, levels = [dict(index, sigma0)] per level)."""
    bg = V.LEARN_BG
    sigma, coef = case["s2"].copy(), case["c2"].copy()
    lo, step = np.asarray(case["lo"], F), np.asarray(case["step"], F)
    nc = coef.shape[3]
    target = case["target"].astype(np.float64)
    rays = (case["o"], case["d"], case["tmin"], case["tmax"])

    def level(sigma, coef, step):
        index = R.active(sigma)
        return dict(index=index, member=member_mask(index, sigma.shape), m=np.zeros((index.size, 1 + 3 * nc), F),
                    v=np.zeros((index.size, 1 + 3 * nc), F), G=V.geometry(sigma, coef, lo, step, *rays, V.LEARN_DT), t=0,
                    sigma0=sigma.copy())

    def evaluate(L):
        G = L["G"]
        sig, raw = V.lookup32(sigma, coef, G)
        c, mask = V.clamp_mask(raw)
        idx = V.pad(G, sig)
        _, w, Tn, valid = V.forward(G, sig, idx, np.float64, 0.0)
        diff = V.composite(G, idx, valid, w, c, bg)[0].astype(F).astype(np.float64) - target
        return float((diff * diff).mean()), (idx, valid, w, Tn, c, mask, diff)

    L = level(sigma, coef, step)
    levels, losses, switches = [L], [], []
    for it in range(steps + 1):
        if it in tuple(upsample_at):
            before = evaluate(L)[0]
            if prune is not None:
                sigma, coef = vp(sigma, coef, prune)
            sigma, coef = vx(sigma, coef)
            step = half_step(step)
            L = level(sigma, coef, step)
            levels.append(L)
            switches.append((before, evaluate(L)[0]))
        loss, (idx, valid, w, Tn, c, mask, diff) = evaluate(L)
        losses.append(loss)
        if it == steps:
            break
        G = L["G"]
        dS, dC = V.vg(G, idx, valid, w, Tn, c, mask, (2.0 * diff).astype(F), None, bg, nc)
        aS, aC = dS * 2.0 ** SHIFT, dC.reshape(-1) * 2.0 ** SHIFT
        n = L["index"].size
        if (tv[0] > 0 or tv[1] > 0) and n:
            k = 3.0 * G.N / n
            tS, tC = np.zeros(sigma.shape, np.int64), np.zeros(coef.shape, np.int64)
            vt(sigma, coef, L["index"], L["member"], tv[0] * k, tv[1] * k, tv_eps, tS, tC)
            aS, aC = aS + tS.reshape(-1).astype(np.float64), aC + tC.reshape(-1).astype(np.float64)
        L["t"] += 1
        V.vu_step(sigma, coef, L["index"], aS, aC, L["m"], L["v"], 1.0 / (3 * G.N), L["t"], lr_sigma, lr_coef)
    return dict(losses=np.asarray(losses), switches=switches, sigma=sigma, coef=coef, lo=lo, step=step, levels=levels)
