"""numpy restatements of rule T of include/nerf_hip.h (TSDF fusion of depth images, nerf_hip_tsdf_integrate): a vectorised model, a scalar
loops model of the same rule, and the scenes the TSDF tests share -- look-at cameras with a made-up K_inv, analytic depth and opacity
images of a sphere along the unit rays, and a random case with every kind of bad depth.  Nothing here needs a device."""
import functools

import numpy as np

F32, F64 = np.float32, np.float64


# ---- cameras (the project's ray rule: pixel (x, y), x the row; p_j = (x K[j] + y K[3 + j]) + K[6 + j]; world direction R p) ----

def look_at(cam, target, near=0.5, far=6.0):
    """a pose row [17] fp32: the camera at cam looking at target (the third column of R is the viewing direction of k_inv's rays)"""
    cam, target = np.asarray(cam, F64), np.asarray(target, F64)
    fwd = (target - cam) / np.linalg.norm(target - cam)
    right = np.cross(fwd, [0.0, 0.3, 1.0] if abs(fwd[2]) < 0.9 else [0.0, 1.0, 0.3])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    P = np.zeros((3, 5))
    P[:, 0], P[:, 1], P[:, 2], P[:, 3] = right, up, fwd, cam
    return np.concatenate((P.reshape(-1), [near, far])).astype(F32)


def k_inv(H, W, s):
    """pixel (x, y) -> p = (s (x - H / 2), s (y - W / 2), 1)"""
    return np.array([[s, 0, 0], [0, s, 0], [-s * H / 2, -s * W / 2, 1]], F32)


def camera_q(pose17, K):
    """-> (Q [3, 3] fp64 = inverse(R K^T), cam_o [3] fp32): mesh.camera_q's rule"""
    P = np.asarray(pose17, F32).reshape(17)[:15].reshape(3, 5)
    return np.linalg.inv(P[:, :3].astype(F64) @ np.asarray(K, F32).reshape(3, 3).astype(F64).T), P[:, 3].copy()


def unit_rays(pose17, K, H, W):
    """-> (o [3], u [H, W, 3]) in fp64: the unit world direction of every pixel's ray"""
    P = np.asarray(pose17, F32).reshape(17)[:15].reshape(3, 5).astype(F64)
    Kd = np.asarray(K, F32).reshape(3, 3).astype(F64)
    x, y = np.meshgrid(np.arange(H, dtype=F64), np.arange(W, dtype=F64), indexing="ij")
    p = x[..., None] * Kd[0] + y[..., None] * Kd[1] + Kd[2]
    d = p @ P[:, :3].T
    return P[:, 3], d / np.linalg.norm(d, axis=-1, keepdims=True)


def sphere_images(pose17, K, H, W, radius):
    """-> (depth [H, W] fp32: the distance along the unit ray to the sphere of ``radius`` about 0, +inf where the ray misses it;
    opacity [H, W] fp32: 1 where it hits, 0 elsewhere)"""
    o, u = unit_rays(pose17, K, H, W)
    b = u @ o
    disc = b * b - (o @ o - radius * radius)
    t = np.where(disc > 0, -b - np.sqrt(np.maximum(disc, 0.0)), np.inf)
    return t.astype(F32), (disc > 0).astype(F32)


# ---- the rule ----

def lattice(lo, step, shape):
    """the lattice points [nx, ny, nz, 3] fp32: per coordinate one fp32 product and one fp32 sum"""
    lo, step = np.asarray(lo, F32), np.asarray(step, F32)
    idx = np.meshgrid(*[np.arange(n, dtype=F32) for n in shape], indexing="ij")
    return np.stack([lo[a] + idx[a] * step[a] for a in range(3)], -1).astype(F32)


def integrate(T, Wt, lo, step, depth, opacity, cams, trunc, min_opacity=0.5, carve=True):
    """Rule T, vectorised over the voxels: T, Wt fp32 [nx, ny, nz] (not modified), depth [n, H, W] fp32, opacity the same or None, cams a
    list of (Q [3, 3] fp64, cam_o [3] fp32) -> the new (T, Wt)."""
    T, Wt = np.array(T, F32), np.array(Wt, F32)
    P = lattice(lo, step, T.shape).astype(F64)
    depth = np.asarray(depth, F32)
    n, H, W = depth.shape
    trunc, min_opacity = F64(trunc), F32(min_opacity)
    with np.errstate(all="ignore"):
        for c, (Q, o) in enumerate(cams):
            Q = np.asarray(Q, F64).reshape(3, 3)
            w = P - np.asarray(o, F32).astype(F64)
            wx, wy, wz = w[..., 0], w[..., 1], w[..., 2]
            m = [(Q[i, 0] * wx + Q[i, 1] * wy) + Q[i, 2] * wz for i in range(3)]
            x, y = np.floor(m[0] / m[2] + 0.5), np.floor(m[1] / m[2] + 0.5)
            view = (m[2] > 0) & (0 <= x) & (x <= H - 1) & (0 <= y) & (y <= W - 1)
            xi, yi = np.where(view, x, 0).astype(np.int64), np.where(view, y, 0).astype(np.int64)
            r = np.sqrt((wx * wx + wy * wy) + wz * wz)
            d = depth[c][xi, yi].astype(F64)
            fg = np.ones_like(view) if opacity is None else np.asarray(opacity, F32)[c][xi, yi] >= min_opacity
            sdf = d - r
            obs = view & fg & np.isfinite(d) & (d > 0) & (sdf >= -trunc)
            val = np.minimum(1.0, sdf / trunc)
            if carve:
                bg = view & ~fg
                val = np.where(bg, 1.0, val)
                obs = obs | bg
            T64, W64 = T.astype(F64), Wt.astype(F64)
            T = np.where(obs, (((T64 * W64) + val) / (W64 + 1.0)).astype(F32), T)
            Wt = np.where(obs, (W64 + 1.0).astype(F32), Wt)
    return T, Wt


def integrate_loops(T, Wt, lo, step, depth, opacity, cams, trunc, min_opacity=0.5, carve=True):
    """Rule T once more, one voxel and one view at a time in numpy scalars, written from the header's text alone."""
    T, Wt = np.array(T, F32), np.array(Wt, F32)
    lo, step, depth = np.asarray(lo, F32), np.asarray(step, F32), np.asarray(depth, F32)
    n, H, W = depth.shape
    trunc, one, half = F64(trunc), F64(1.0), F64(0.5)
    with np.errstate(all="ignore"):
        for i in range(T.shape[0]):
            for j in range(T.shape[1]):
                for k in range(T.shape[2]):
                    p = [F64(F32(lo[a] + F32(F32(q) * step[a]))) for a, q in enumerate((i, j, k))]
                    t, wt = T[i, j, k], Wt[i, j, k]
                    for c, (Q, o) in enumerate(cams):
                        Q = np.asarray(Q, F64).reshape(9)
                        w = [p[a] - F64(F32(o[a])) for a in range(3)]
                        m = [(Q[3 * r] * w[0] + Q[3 * r + 1] * w[1]) + Q[3 * r + 2] * w[2] for r in range(3)]
                        x, y = np.floor(m[0] / m[2] + half), np.floor(m[1] / m[2] + half)
                        if not (m[2] > 0 and 0 <= x <= H - 1 and 0 <= y <= W - 1):
                            continue
                        xi, yi = int(x), int(y)
                        if opacity is None or F32(opacity[c][xi, yi]) >= F32(min_opacity):
                            d = F64(depth[c, xi, yi])
                            r = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
                            sdf = d - r
                            if not (np.isfinite(d) and d > 0 and sdf >= -trunc):
                                continue
                            val = min(one, sdf / trunc)
                        elif carve:
                            val = one
                        else:
                            continue
                        t = F32(((F64(t) * F64(wt)) + val) / (F64(wt) + one))
                        wt = F32(F64(wt) + one)
                    T[i, j, k], Wt[i, j, k] = t, wt
    return T, Wt


def grid(T, Wt, unseen="solid"):
    """mesh.tsdf_grid's rule: -T where Wt > 0, elsewhere +1 (solid) or -1 (empty)"""
    return np.where(Wt > 0, -T, F32(1.0 if unseen == "solid" else -1.0)).astype(F32)


def crossings(G, P):
    """the points where the lattice edges cross G == 0 (inside = G > 0), linearly interpolated: [m, 3] fp64"""
    out = []
    P = np.asarray(P, F64)
    for ax in range(3):
        a_, b_ = [slice(None)] * 3, [slice(None)] * 3
        a_[ax], b_[ax] = slice(0, -1), slice(1, None)
        a, b = G[tuple(a_)].astype(F64), G[tuple(b_)].astype(F64)
        m = (a > 0) != (b > 0)
        t = (0.0 - a[m]) / (b[m] - a[m])
        out.append(P[tuple(a_)][m] + t[:, None] * (P[tuple(b_)][m] - P[tuple(a_)][m]))
    return np.concatenate(out)


# ---- the scenes ----

SPHERE_R = 0.6
SPHERE_CAMS = ([2.5, 0, 0], [-2.5, 0, 0], [0, 2.5, 0], [0, -2.5, 0], [0, 0, 2.5], [0, 0, -2.5], [1.5, 1.5, 1.5], [-1.5, -1.5, -1.5])


@functools.lru_cache(maxsize=None)
def sphere_scene(shape=(24, 25, 26), H=48, W=64):
    """A sphere of radius 0.6 seen by eight cameras (six on the axes at distance 2.5, two on the diagonal) over a lattice on [-1, 1]^3
    -> dict(shape, lo, step, trunc, poses [8, 17], K, H, W, depth [8, H, W], opacity [8, H, W], cams).  Cached: treat as read-only."""
    lo = np.full(3, -1.0, F32)
    step = ((np.full(3, 1.0, F32) - lo) / np.asarray([n - 1 for n in shape], F32)).astype(F32)
    K = k_inv(H, W, 1.0 / (0.9 * min(H, W)))
    poses = np.stack([look_at(c, (0.0, 0.0, 0.0)) for c in SPHERE_CAMS])
    imgs = [sphere_images(p, K, H, W, SPHERE_R) for p in poses]
    out = dict(shape=tuple(shape), lo=lo, step=step, trunc=4.0 * float(step.max()), poses=poses, K=K, H=H, W=W,
               depth=np.stack([d for d, _ in imgs]), opacity=np.stack([a for _, a in imgs]), cams=[camera_q(p, K) for p in poses])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def sphere_fused(carve=True):
    """the reference's (T, Wt) of sphere_scene() from zero (computed once per carve; read-only)"""
    s = sphere_scene()
    z = np.zeros(s["shape"], F32)
    T, Wt = integrate(z, z, s["lo"], s["step"], s["depth"], s["opacity"], s["cams"], s["trunc"], 0.5, carve)
    T.setflags(write=False)
    Wt.setflags(write=False)
    return T, Wt


def random_case(n=3, H=8, W=12, shape=(5, 6, 7), seed=0):
    """A small lattice on [-1, 1]^3 and n cameras around it with random depth images that carry +inf, NaN, 0 and negative entries and
    random opacities -> dict(shape, lo, step, trunc, poses, K, H, W, depth, opacity, cams)."""
    rng = np.random.default_rng(seed)
    lo = np.array([-1.0, -0.9, -1.1], F32)
    step = (np.array([2.0, 1.8, 2.2], F32) / np.asarray([m - 1 for m in shape], F32)).astype(F32)
    K = k_inv(H, W, 1.4 / min(H, W))
    dirs = rng.normal(size=(n, 3))
    poses = np.stack([look_at(d / np.linalg.norm(d) * rng.uniform(2.2, 3.0), rng.uniform(-0.2, 0.2, 3)) for d in dirs])
    depth = rng.uniform(1.0, 4.0, (n, H, W)).astype(F32)
    bad = rng.random((n, H, W))
    depth[bad < 0.05] = np.inf
    depth[(bad >= 0.05) & (bad < 0.10)] = np.nan
    depth[(bad >= 0.10) & (bad < 0.15)] = 0.0
    depth[(bad >= 0.15) & (bad < 0.20)] = -1.5
    depth[(bad >= 0.20) & (bad < 0.22)] = -np.inf
    opacity = rng.random((n, H, W)).astype(F32)
    opacity[rng.random((n, H, W)) < 0.03] = np.nan
    return dict(shape=tuple(shape), lo=lo, step=step, trunc=4.0 * float(step.max()), poses=poses, K=K, H=H, W=W, depth=depth,
                opacity=opacity, cams=[camera_q(p, K) for p in poses])
