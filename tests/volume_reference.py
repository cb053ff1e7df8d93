"""numpy restatements of the SH radiance volume rules of include/nerf_hip.h (VA, VS, VO, VL, VR), in fp32 with every product, sum and
division rounded on its own -- bit for bit wherever no exp is involved --, an fp64 composite of the fp32 rule's own sample values, and
the bound the fp32 march has to meet against that composite.  Shared by tests/test_volume_cpu.py and tests/test_gpu_volume.py.

THE BOUND.  u = 2^-24 is the unit roundoff of fp32.  The composite takes the rule's own (t_k, sigma_s, rgb_k) of the N contributing
samples, so the only differences are the roundings of the compositing recurrence.  All of T, alpha, w, A, rgb lie in [0, 1].
  alpha = -expm1f(-(sigma_s dt)): the product's rounding moves x = sigma_s dt by x u and alpha by x e^-x u <= u; expm1f itself is taken
      as 2 ulp = 4 u alpha <= 4 u.  (The project carries no copy of ROCm's HIP math accuracy table, so 2 ulp is an ASSUMPTION, not
      a documented figure.)  So |d alpha| <= 5 u.
  w = T alpha (one rounding) and T' = T - w (one rounding): with e_n the error of T after n samples,
      e_n <= e_(n-1) (1 - alpha_n) + 7 u     and     |d w_n| <= e_(n-1) alpha_n + 6 u.
      Since e_(n-1) alpha_n = e_(n-1) - e_(n-1) (1 - alpha_n) <= e_(n-1) - e_n + 7 u, the sum telescopes: sum_n |d w_n| <= 13 u N.
  Every output adds one product and one sum per sample (A: the sum only), each at most u times a value <= 1 (times t for D):
      |dA| <= 14 u N,    |dC_ch| <= 15 u N,    |dD| <= 15 u N max t_k.
  The final rgb = C + (1 - A) bg adds |bg| (14 u N + u) + 2 u (1 + |bg|).
OPS = 15 roundings per contributing sample (4 of them expm1f's); second-order terms are covered by the factor (1 + 2^-10).
bound(N) = OPS N u (1 + 2^-10) + 4 u, times (1 + max |background|) for rgb and times max(1, max t_k) for D.  It is derived, never fitted
to a kernel's output.
"""
import numpy as np

F = np.float32
U = 2.0 ** -24
OPS = 15
MAX_STEPS = 65536
SH_C64 = (np.sqrt(1 / (4 * np.pi)), np.sqrt(3 / (4 * np.pi)), np.sqrt(15 / (4 * np.pi)), np.sqrt(5 / (16 * np.pi)), np.sqrt(15 / (16 * np.pi)))
SH_C32 = tuple(F(c) for c in SH_C64)


def bound(n_contrib):
    """|fp32 march - fp64 composite| for A (and, scaled as the docstring says, rgb and D) with n_contrib contributing samples."""
    return OPS * np.asarray(n_contrib, np.float64) * U * (1 + 2.0 ** -10) + 4 * U


# ---- VS ----

def basis64(d):
    """Y_0 .. Y_8 at d [..., 3] in fp64 with the unrounded constants."""
    d = np.asarray(d, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    C = SH_C64
    return np.stack([C[0] + 0 * x, C[1] * y, C[1] * z, C[1] * x, C[2] * (x * y), C[2] * (y * z), C[3] * (3 * (z * z) - 1), C[2] * (x * z),
                     C[4] * (x * x - y * y)], axis=-1)


def basis32(d):
    """Rule VS's basis at d [..., 3] in fp32, as the kernels evaluate it."""
    d = np.asarray(d, F)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    C = SH_C32
    with np.errstate(all="ignore"):
        return np.stack([np.full_like(x, C[0]), C[1] * y, C[1] * z, C[1] * x, C[2] * (x * y), C[2] * (y * z),
                         C[3] * ((F(3) * (z * z)) - F(1)), C[2] * (x * z), C[4] * ((x * x) - (y * y))], axis=-1).astype(F)


def sh_tables():
    """-> (dirs [12, 3] fp32, b [12, 9] fp32): the icosahedron's vertices in the header's order and b_km = fp32(w Y_m(d_k)), zeros +0."""
    phi = (1 + np.sqrt(np.float64(5))) / 2
    V = []
    for c in range(3):
        for s1 in (1.0, -1.0):
            for s2 in (1.0, -1.0):
                v = np.zeros(3)
                v[(c + 1) % 3] = s1
                v[(c + 2) % 3] = s2 * phi
                V.append(v / np.sqrt(1 + phi * phi))
    dirs = np.asarray(V).astype(F)
    b = (4 * np.pi / 12) * basis64(dirs.astype(np.float64))
    return dirs, (b + 0.0).astype(F) + F(0)


def sh_project(rgbs, index, shape, degree):
    """coef [nx, ny, nz, ncoef, 3]: rgbs[k] [n, 3] fp32 = the colour of the points index[n] along direction k, accumulated in k order."""
    _, b = sh_tables()
    nc = (degree + 1) ** 2
    coef = np.zeros((int(np.prod(shape)), nc, 3), F)
    for k in range(12):
        term = (b[k, :nc, None] * np.asarray(rgbs[k], F)[:, None, :]).astype(F)
        coef[index] = (coef[index] + term).astype(F)
    return coef.reshape(*shape, nc, 3)


# ---- VA, VO ----

def active(sigma):
    """The linear indices of the ACTIVE points, ascending."""
    pos = np.pad(np.asarray(sigma) > 0, 1)
    nx, ny, nz = sigma.shape
    a = np.zeros(sigma.shape, bool)
    for di in range(3):
        for dj in range(3):
            for dk in range(3):
                a |= pos[di:di + nx, dj:dj + ny, dk:dk + nz]
    return np.flatnonzero(a.reshape(-1))


def lattice_points(index, shape, lo, step):
    i, j, k = np.unravel_index(np.asarray(index, np.int64), shape)
    lo, step = np.asarray(lo, F), np.asarray(step, F)
    return np.stack([lo[0] + i.astype(F) * step[0], lo[1] + j.astype(F) * step[1], lo[2] + k.astype(F) * step[2]], axis=-1).astype(F)


def block_dims(shape, B):
    return tuple((n - 1 + B - 1) // B for n in shape)


def blocks(sigma, B):
    nb = block_dims(sigma.shape, B)
    occ = np.zeros(nb, np.uint8)
    pos = np.asarray(sigma) > 0
    for x in range(nb[0]):
        for y in range(nb[1]):
            for z in range(nb[2]):
                sl = tuple(slice(b * B, min((b + 1) * B, n - 1) + 1) for b, n in zip((x, y, z), sigma.shape))
                occ[x, y, z] = 1 if pos[sl].any() else 0
    return occ


# ---- VL ----

def cells(x, lo, step, shape):
    """x [M, 3] fp32 -> (inside [M] bool, ci [M, 3] int64, f [M, 3] fp32)."""
    x = np.asarray(x, F).reshape(-1, 3)
    lo, step = np.asarray(lo, F), np.asarray(step, F)
    n = np.asarray(shape)
    with np.errstate(all="ignore"):
        g = ((x - lo) / step).astype(F)
        inside = ((F(0) <= g) & (g <= (n - 1).astype(F))).all(axis=1)
        fi = np.fmin(np.fmax(np.floor(g), F(0)), (n - 2).astype(F)).astype(F)
        f = (g - fi).astype(F)
    return inside, fi.astype(np.int64), f


def _lerp(a, b, f):
    with np.errstate(all="ignore"):
        return (a + (f * (b - a).astype(F)).astype(F)).astype(F)


def _tri(v, f):
    """v [M, 2, 2, 2, ...] corner values, f [M, 3] -> [M, ...]: z first, then y, then x."""
    ex = (slice(None),) + (None,) * (v.ndim - 4)
    c = _lerp(v[:, :, :, 0], v[:, :, :, 1], f[:, 2][ex][:, None, None])
    c = _lerp(c[:, :, 0], c[:, :, 1], f[:, 1][ex][:, None])
    return _lerp(c[:, 0], c[:, 1], f[:, 0][ex])


def _corners(a, ci):
    """a [nx, ny, nz, ...] -> [M, 2, 2, 2, ...]"""
    i, j, k = ci[:, 0], ci[:, 1], ci[:, 2]
    return np.stack([np.stack([np.stack([a[i + di, j + dj, k + dk] for dk in (0, 1)], axis=1) for dj in (0, 1)], axis=1) for di in (0, 1)], axis=1)


def lookup(sigma, coef, lo, step, x, d):
    """Rule VL at points x [M, 3] along d [M, 3] -> (sigma_s [M], rgb [M, 3]) fp32."""
    x = np.asarray(x, F).reshape(-1, 3)
    d = np.asarray(d, F).reshape(-1, 3)
    inside, ci, f = cells(x, lo, step, sigma.shape)
    s = _tri(_corners(np.asarray(sigma, F), ci), f)
    nc = coef.shape[3]
    Y = basis32(d)[:, :nc]                                  # [M, nc]
    cc = _corners(np.asarray(coef, F), ci)                  # [M, 2, 2, 2, nc, 3]
    with np.errstate(all="ignore"):
        val = (Y[:, None, None, None, 0, None] * cc[..., 0, :]).astype(F)
        for m in range(1, nc):
            val = (val + (Y[:, None, None, None, m, None] * cc[..., m, :]).astype(F)).astype(F)
        rgb = np.fmin(np.fmax(_tri(val, f), F(0)), F(1)).astype(F)
    s = np.where(inside, s, F(0)).astype(F)
    rgb = np.where(inside[:, None], rgb, F(0)).astype(F)
    return s, rgb


# ---- VR ----

def ray_samples(sigma, coef, lo, step, o, d, tmin, tmax, dt):
    """Everything rule VR computes along one ray before the compositing: None for a miss, else a dict with K, tk [K], inside [K],
    ci [K, 3], sig [K], rgb [K, 3] (rule VL's at every sample), t_a, t_b."""
    o, d = np.asarray(o, F).reshape(3), np.asarray(d, F).reshape(3)
    tmin, tmax, dt = F(tmin), F(tmax), F(dt)
    lo, step = np.asarray(lo, F), np.asarray(step, F)
    if not (np.isfinite(o).all() and np.isfinite(d).all() and np.isfinite(tmin) and np.isfinite(tmax)):
        return None
    ta, tb = tmin, tmax
    with np.errstate(all="ignore"):
        for a in range(3):
            hi = F(lo[a] + F(F(sigma.shape[a] - 1) * step[a]))
            if d[a] == 0:
                if not (lo[a] <= o[a] <= hi):
                    return None
            else:
                t1, t2 = F((lo[a] - o[a]) / d[a]), F((hi - o[a]) / d[a])
                ta, tb = np.fmax(ta, np.fmin(t1, t2)), np.fmin(tb, np.fmax(t1, t2))
        if not (ta < tb):
            return None
        K = int(np.fmin(np.ceil(F(F(tb - ta) / dt)), F(MAX_STEPS)))
        k = np.arange(K, dtype=np.int64)
        tk = (ta + ((k.astype(F) + F(0.5)) * dt).astype(F)).astype(F)
        x = (o[None, :] + (tk[:, None] * d[None, :]).astype(F)).astype(F)
    inside, ci, _ = cells(x, lo, step, sigma.shape)
    sig, rgb = lookup(sigma, coef, lo, step, x, np.broadcast_to(d, x.shape))
    return dict(K=K, tk=tk, inside=inside, ci=ci, sig=sig, rgb=rgb, ta=ta, tb=tb, o=o, d=d, dt=dt)


def walk(s, occ, B, shape, lo, step):
    """The samples the marcher LOOKS AT for block edge B, following csrc/volume.hip's jump (estimate from the exit planes, verified on
    the candidate sample and the one before it) -> the list of evaluated sample numbers, ascending."""
    lo, step = np.asarray(lo, F), np.asarray(step, F)
    K, o, d, dt, ta = s["K"], s["o"], s["d"], s["dt"], s["ta"]
    out, k = [], 0
    while k < K:
        out.append(k)
        nxt = k + 1
        if s["inside"][k]:
            ci = s["ci"][k]
            b = [min(int(ci[a]) // B, occ.shape[a] - 1) for a in range(3)]
            if occ[b[0], b[1], b[2]] == 0:
                c0 = [b[a] * B for a in range(3)]
                c1 = [min((b[a] + 1) * B, shape[a] - 1) for a in range(3)]
                te = F(np.inf)
                with np.errstate(all="ignore"):
                    for a in range(3):
                        if d[a] > 0:
                            te = np.fmin(te, F(F(F(lo[a] + F(F(c1[a]) * step[a])) - o[a]) / d[a]))
                        if d[a] < 0:
                            te = np.fmin(te, F(F(F(lo[a] + F(F(c0[a]) * step[a])) - o[a]) / d[a]))
                    kf = np.fmin(np.floor(F(F(F(te - ta) / dt) - F(0.5))), F(K - 1))
                ke = int(kf) if kf > F(k) else k
                for _ in range(2):
                    if ke <= k:
                        break
                    ce = s["ci"][ke]
                    if s["inside"][ke] and all(c0[a] <= ce[a] < c1[a] for a in range(3)):
                        nxt = ke + 1
                        break
                    ke -= 1
        k = nxt
    return out


def composite32(s, evaluated, t_stop, bg, drop=None):
    """Rule VR's recurrence in fp32 over the evaluated samples -> (rgb [3], (D, A), (contributing, evaluated), the contributing sample
    numbers).  drop: the ordinal of one contributing sample to leave out (the tests' teeth)."""
    dt, bg, t_stop = s["dt"], np.asarray(bg, F), F(t_stop)
    T, C, D, A = F(1), np.zeros(3, F), F(0), F(0)
    used, looked, seen = [], 0, 0
    with np.errstate(all="ignore"):
        for k in evaluated:
            looked += 1
            if not (s["sig"][k] > 0):
                continue
            seen += 1
            if drop is not None and seen - 1 == drop:
                continue
            alpha = F(-np.expm1(F(-F(s["sig"][k] * dt))))
            w = F(T * alpha)
            C = (C + (w * s["rgb"][k]).astype(F)).astype(F)
            D = F(D + F(w * s["tk"][k]))
            A = F(A + w)
            T = F(T - w)
            used.append(k)
            if T < t_stop:
                break
        rgb = (C + (F(F(1) - A) * bg).astype(F)).astype(F)
    return rgb, np.asarray([D, A], F), np.asarray([len(used), looked], np.int32), used


def composite64(s, used, bg, dt=None):
    """The same recurrence in float64 on the fp32 rule's own sample values (t_k, sigma_s, rgb) of the contributing samples ``used``."""
    dt = np.float64(s["dt"] if dt is None else dt)
    bg = np.asarray(bg, np.float64)
    T, C, D, A = 1.0, np.zeros(3), 0.0, 0.0
    for k in used:
        alpha = -np.expm1(-(np.float64(s["sig"][k]) * dt))
        w = T * alpha
        C = C + w * s["rgb"][k].astype(np.float64)
        D = D + w * np.float64(s["tk"][k])
        A = A + w
        T = T - w
    return C + (1.0 - A) * bg, np.asarray([D, A])


def march(sigma, coef, occ, B, lo, step, origins, dirs, tmin, tmax, dt, t_stop=0.0, bg=(0, 0, 0)):
    """Rule VR over rays -> (rgb [N, 3], maps [N, 2], steps [N, 2] int32, per-ray (samples dict or None, contributing sample numbers))."""
    origins, dirs = np.asarray(origins, F).reshape(-1, 3), np.asarray(dirs, F).reshape(-1, 3)
    N = origins.shape[0]
    tmin, tmax = np.broadcast_to(np.asarray(tmin, F), (N,)), np.broadcast_to(np.asarray(tmax, F), (N,))
    rgb, maps, steps, info = np.zeros((N, 3), F), np.zeros((N, 2), F), np.zeros((N, 2), np.int32), []
    for r in range(N):
        s = ray_samples(sigma, coef, lo, step, origins[r], dirs[r], tmin[r], tmax[r], dt)
        if s is None:
            rgb[r] = np.asarray(bg, F)
            info.append((None, []))
            continue
        rgb[r], maps[r], steps[r], used = composite32(s, walk(s, occ, B, sigma.shape, lo, step), t_stop, bg)
        info.append((s, used))
    return rgb, maps, steps, info


# ---- the hand-made inputs the CPU and GPU tests share ----

BLOB = np.asarray([0.5, 0.3, 0.2], F)   # the centre of the dense blob: the low corner's blocks stay empty up to an edge of 4 cells

def make_volume(shape, seed, degree=2, empty_half=True):
    """A lattice over a box of about 2 x 1.6 x 1.2 with sigma in [0.5, 6) on a blob and 0 elsewhere (so that some blocks are empty), and
    coefficients that give colours inside and outside [0, 1] (the clamp is exercised)."""
    rng = np.random.default_rng(seed)
    lo = np.asarray([-1.0, -0.8, -0.6], F)
    ext = np.asarray([2.0, 1.6, 1.2], F)
    step = (ext / (np.asarray(shape) - 1).astype(F)).astype(F)
    ijk = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), axis=-1)
    p = lo + ijk.astype(F) * step
    r = np.sqrt((((p - BLOB) / np.asarray([0.42, 0.42, 0.34], F)) ** 2).sum(-1))
    sigma = (rng.uniform(0.5, 6.0, shape) * (r < 1.0 if empty_half else True)).astype(F)
    nc = (degree + 1) ** 2
    coef = rng.normal(0.0, 0.35, shape + (nc, 3)).astype(F)
    coef[..., 0, :] = rng.uniform(0.2, 4.2, shape + (3,)).astype(F)
    return sigma, coef, lo, step


def make_rays(n, seed, lo, step, shape):
    """n >= 1 rays around the box of the lattice; the first seven are the special ones: a NaN origin, a start inside the box, a zero
    direction component, a ray lying in a face of the box, a window that begins beyond the exit, and two plain hits; every seventh of
    the rest points away from the box.  -> (origins, dirs, tmin, tmax) fp32."""
    rng = np.random.default_rng(seed)
    lo = np.asarray(lo, F)
    hi = (lo + (np.asarray(shape) - 1).astype(F) * np.asarray(step, F)).astype(F)
    c = ((lo + hi) / 2).astype(F)
    o = np.zeros((max(n, 7), 3), F)
    d = np.zeros_like(o)
    tmin = np.zeros(o.shape[0], F)
    tmax = np.full(o.shape[0], 8.0, F)
    u = rng.normal(size=o.shape)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o[:] = c + 3.0 * u
    target = BLOB + rng.uniform(-0.3, 0.3, o.shape)
    d[:] = target - o
    away = (np.arange(o.shape[0]) % 7 == 6) & (np.arange(o.shape[0]) >= 7)
    d[away] = -d[away]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d.astype(F)
    o[0, 1] = np.nan                                         # a NaN origin
    o[1] = BLOB + np.asarray([-0.05, 0.05, 0.02], F)         # starts inside the box (and the blob)
    o[2], d[2] = (BLOB[0], BLOB[1], lo[2] - 1.0), (0.0, 0.0, 1.0)         # two zero direction components
    o[3], d[3] = (lo[0] - 1.0, c[1] + 0.1, hi[2]), (1.0, 0.0, 0.0)        # lies in the face z = hi: it grazes the box
    tmin[4] = 7.5                                            # the window begins beyond the exit
    return o[:n].copy(), d[:n].copy(), tmin[:n].copy(), tmax[:n].copy()


def slab_case():
    """constant sigma_0 and a constant degree-0 colour over the whole box; axis-parallel rays whose window is a whole number of steps
    strictly inside the box, so every sample is inside and contributes"""
    shape = (5, 4, 3)
    lo = np.asarray([-1.0, -0.75, -0.5], F)
    step = np.asarray([0.5, 0.5, 0.5], F)
    sigma0, c = F(1.75), np.asarray([0.25, 0.5, 0.875], F)
    sigma = np.full(shape, sigma0, F)
    coef = np.zeros(shape + (1, 3), F)
    coef[..., 0, :] = c / SH_C32[0]
    o = np.asarray([[-3.0, 0.0, 0.0], [0.25, -3.0, 0.25], [0.5, 0.5, 3.0]], F)
    d = np.asarray([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0]], F)
    dt = F(0.0625)
    tmin = np.asarray([2.25, 2.5, 2.625], F)       # inside the box: x = -0.75, y = -0.5, z = 0.375
    K = np.asarray([20, 12, 10])
    tmax = (tmin + K.astype(F) * dt).astype(F)     # exact in fp32: x = 0.5, y = 0.25, z = -0.25
    return sigma, coef, lo, step, o, d, tmin, tmax, dt, K, float(sigma0), c


def check_slab(rgb, maps, steps, K, sigma0, c, dt):
    A = 1.0 - np.exp(-np.float64(sigma0) * K * np.float64(dt))
    assert np.array_equal(steps[:, 0], K) and np.array_equal(steps[:, 1], K)
    b = bound(K)
    assert (np.abs(maps[:, 1] - A) <= b).all(), (maps[:, 1] - A, b)
    # the colour: Y_0 (c / Y_0) is c to one rounding of the division and one of the product (2 u, c <= 1)
    assert (np.abs(rgb - c[None, :].astype(np.float64) * A[:, None]) <= (b + 2 * U)[:, None]).all()
